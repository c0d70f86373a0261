"""Haplotype dosages (expected copies of caller-given haplotypes) by exhaustive
enumeration.

Built on enumeration.estep alone: `priors[{h0, h1}]` over every phasing of an
individual, exact rationals; dividing by their total gives post({h0, h1}).  A
pattern is (start, A, B): a window start .. start + len(A) - 1 with two rows of
allele symbols, -1 = any allele, B = None = all -1.  M(x, y) holds when x
matches row A and y row B at every locus of the window, and

    d[i][p] = sum over pairs {h0, h1} of post({h0, h1}) ([M(h0, h1)] + [M(h1, h0)])

— two terms always, also when h0 == h1.  No forward-backward pass, no lattice,
no labels, no slots.  This module imports neither the product nor the
restatement.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import enumeration as en

ANY = -1
ABSENT = 0x7FFFFFF0  # a symbol no allele table holds


def row_matches(h, start: int, row) -> bool:
    return all(r == ANY or h[start + k] == r for k, r in enumerate(row))


def matches(x, y, start: int, A, B) -> bool:
    """M(x, y): x against row A, y against row B."""
    return row_matches(x, start, A) and (B is None or row_matches(y, start, B))


def dosages_exact(alleles: np.ndarray, pt: dict, head_len: int, patterns) -> list:
    """Per individual the list of d[i][p] as Fractions (None for the
    individuals the enumeration does not cover, HEAD_QUIRK).  The priors are
    first summed per window over the pairs' two ordered restrictions to it, so
    a pattern meets each distinct restricted pair once."""
    pats = [(int(s), tuple(int(x) for x in A), None if B is None else tuple(int(x) for x in B)) for s, A, B in patterns]
    for s, A, B in pats:
        assert len(A) >= 1 and 0 <= s and s + len(A) <= alleles.shape[2] and (B is None or len(B) == len(A))
    windows = sorted({(s, len(A)) for s, A, _ in pats})
    out = []
    for e in en.estep(alleles, pt, head_len):
        if e is None:
            out.append(None)
            continue
        tot = sum(e["priors"].values(), Fraction(0))
        assert tot == e["total"] > 0
        ordered = {}  # window: {(x restricted, y restricted): posterior summed over both orientations of every pair}
        for s, n in windows:
            acc = {}
            for (h0, h1), p in e["priors"].items():
                for x, y in ((h0, h1), (h1, h0)):  # two terms, also when h0 == h1
                    k = (x[s:s + n], y[s:s + n])
                    acc[k] = acc.get(k, Fraction(0)) + p
            ordered[s, n] = acc
        row = []
        for s, A, B in pats:
            acc = ordered[s, len(A)]
            if B is not None and ANY not in A and ANY not in B:
                d = acc.get((A, B), Fraction(0))
            else:
                d = sum((p for (x, y), p in acc.items() if matches(x, y, 0, A, B)), Fraction(0))
            row.append(d / tot)
        out.append(row)
    return out


def panel_patterns(alleles: np.ndarray, pt: dict, head_len: int) -> list:
    """The pattern set of the enumeration tests: for every window of length 1,
    2, 3 and L at every start, every window haplotype that occurs in any
    enumerated pair, one-sided; one pattern with an absent symbol; one with -1
    in its middle (windows of three loci or more); and the two-sided specs of
    every enumerated pair of the first two covered individuals."""
    L = alleles.shape[2]
    est = en.estep(alleles, pt, head_len)
    covered = [i for i, e in enumerate(est) if e is not None]
    pats = []
    for n in sorted({1, 2, 3, L}):
        for s in range(L - n + 1):
            haps = sorted({h[s:s + n] for e in est if e is not None for pair in e["priors"] for h in pair})
            pats += [(s, h, None) for h in haps]
            bad = list(haps[0])
            bad[n // 2] = ABSENT
            pats.append((s, tuple(bad), None))
            if n >= 3:
                mid = list(haps[-1])
                mid[n // 2] = ANY
                pats.append((s, tuple(mid), None))
            two = sorted({(x[s:s + n], y[s:s + n]) for i in covered[:2] for h0, h1 in est[i]["priors"]
                          for x, y in ((h0, h1), (h1, h0))})
            pats += [(s, x, y) for x, y in two]
    return pats


def mixed_values(exact: list) -> tuple:
    """(values in (0.05, 0.95) or (1.05, 1.95), individuals that have one)."""
    lo, hi = Fraction(5, 100), Fraction(95, 100)
    n, who = 0, set()
    for i, row in enumerate(exact):
        if row is None:
            continue
        k = sum(1 for d in row if lo < d < hi or 1 + lo < d < 1 + hi)
        n += k
        if k:
            who.add(i)
    return n, len(who)
