"""Window phasings (the distinct haplotype pairs over a window of loci, each
with its posterior summed over everything outside the window, ranked) by
exhaustive enumeration.

Built on enumeration.estep alone: `priors[{h0, h1}]` over every phasing of an
individual, exact rationals.  Per window the priors are summed over the pairs'
two ordered restrictions to it — the accumulation dosage_enumeration.
dosages_exact forms — and folded to unordered window pairs:

    post({x, y}) = sum over pairs {h0, h1} restricted to {x, y} of post({h0, h1})
                 = acc[x, y] / total          for x != y  (acc[x, y] = acc[y, x])
                 = acc[x, x] / (2 total)      for x == y  (every such pair adds both of its orders)

ranked by posterior descending, among equals by (x, y) with x <= y: symbols
sort as allele-table indices do.  No forward-backward pass, no lattice, no
configuration codes.  This module imports neither the product nor the
restatement.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import enumeration as en


def windows_of(L: int) -> list:
    """Every (start, len) with len in {1, 2, 3, ceil(L / 2), L}."""
    return [(s, n) for n in sorted({1, 2, 3, (L + 1) // 2, L}) if n <= L for s in range(L - n + 1)]


def config_count(g: np.ndarray, table_of_alleles, start: int, n: int) -> int:
    """C: the ordered configurations of genotype g[2][L] over the window — the
    product over its loci of the ordered allele pairs the genotype allows (1 at
    a locus with both alleles present and equal)."""
    c = 1
    for k in range(start, start + n):
        c *= len(en.locus_options(g, k, [s for s, f in table_of_alleles[k] if f > 0]))
    return c


def window_exact(alleles: np.ndarray, pt: dict, head_len: int, windows) -> list:
    """Per individual (None where the enumeration does not cover it,
    HEAD_QUIRK): {(start, len): [((x, y), posterior)]} over every unordered
    window pair x <= y of the enumeration, ranked."""
    wins = sorted({(int(s), int(n)) for s, n in windows})
    for s, n in wins:
        assert n >= 1 and 0 <= s and s + n <= alleles.shape[2]
    key = ("window", en._digest(alleles), en.Table(pt).key, head_len, tuple(wins))
    return en.memo(key, lambda: _window_exact(alleles, pt, head_len, wins))


def _window_exact(alleles, pt, head_len, wins):
    out = []
    for e in en.estep(alleles, pt, head_len):
        if e is None:
            out.append(None)
            continue
        tot = sum(e["priors"].values(), Fraction(0))
        assert tot == e["total"] > 0
        per = {}
        for s, n in wins:
            acc = {}
            for (h0, h1), p in e["priors"].items():
                for x, y in ((h0, h1), (h1, h0)):  # two terms, also when h0 == h1
                    k = (x[s:s + n], y[s:s + n])
                    acc[k] = acc.get(k, Fraction(0)) + p
            rows = {}
            for (x, y), p in acc.items():
                if x > y:
                    assert acc[y, x] == p
                    continue
                rows[x, y] = p / tot / (2 if x == y else 1)
            per[s, n] = sorted(rows.items(), key=lambda kv: (-kv[1], kv[0]))
        out.append(per)
    return out


def positive(ranked: list) -> int:
    return sum(1 for _, p in ranked if p > 0)


def restrictions(g: np.ndarray, table_of_alleles, start: int, n: int) -> set:
    """Every unordered window pair (x <= y) that is the restriction of a phasing of genotype g."""
    out = {((), ())}
    for k in range(start, start + n):
        opts = en.locus_options(g, k, [s for s, f in table_of_alleles[k] if f > 0])
        out = {(x + (a,), y + (b,)) for x, y in out for a, b in opts}
    return {(x, y) if x <= y else (y, x) for x, y in out}
