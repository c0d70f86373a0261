"""The most probable haplotype pair by exhaustive enumeration, and the
acceptance predicate of a MAP phaser against it.

Built on draw_enumeration.pair_posteriors_exact alone (exact rationals over
every phasing of an individual); this module imports neither the product nor
the restatement.

Acceptance.  A max-product sweep compares computed path values, not exact
ones.  A computed path value is the path's product with one rounding per
record for the state's product of two transition probabilities and one for
multiplying it into the running value, at most 2L + 2 roundings over the head
record and the L - head_len above it (the doublings are exact), so it lies
within a factor 1 +- gamma(2L + 2) of the pair's exact value.  The pair the
sweep returns, c, had the largest computed value, in particular one no smaller
than the computed value of an exact maximiser m:
    e_c (1 + g) >= computed(c) >= computed(m) >= e* (1 - g),   g = gamma(2L + 2),
and dividing both exact values by the same P(genotype) changes nothing:
    e_c >= e* (1 - g) / (1 + g).
Every pair that passes is a legitimate answer; the bound is derived, not tuned.
"""
from __future__ import annotations

from fractions import Fraction

import draw_enumeration as de
import enumeration as en


def map_pairs_exact(alleles, pt: dict, head_len: int) -> list:
    """Per individual (None where the enumeration does not cover it,
    HEAD_QUIRK): dict(best = the largest exact posterior of any pair, argmax =
    the set of pairs that attain it, post = {pair: posterior})."""
    out = []
    for d in de.pair_posteriors_exact(alleles, pt, head_len):
        if d is None:
            out.append(None)
            continue
        best = max(d.values())
        out.append(dict(best=best, argmax={k for k, p in d.items() if p == best}, post=d))
    return out


def map_roundings(L: int) -> int:
    return 2 * L + 2


def map_floor(best: Fraction, L: int) -> Fraction:
    """The smallest exact posterior a returned pair may have."""
    g = en.gamma(map_roundings(L))
    return best * (1 - g) / (1 + g)


def accepts(e_c, best: Fraction, L: int) -> bool:
    """The predicate: a pair of exact posterior e_c is an acceptable MAP answer."""
    return e_c >= map_floor(best, L)


def second_best(entry: dict):
    """(pair, posterior) of the best pair outside the argmax set, or None."""
    rest = {k: p for k, p in entry["post"].items() if k not in entry["argmax"]}
    if not rest:
        return None
    k = max(rest, key=lambda x: (rest[x], x))
    return k, rest[k]
