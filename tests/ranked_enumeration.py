"""The haplotype pairs of an individual ranked by exact posterior, by exhaustive
enumeration, and the acceptance predicate of a ranked phaser against them.

Built on draw_enumeration.pair_posteriors_exact alone (exact rationals over
every phasing of an individual, every unordered pair once); this module imports
neither the product nor the restatement.

Acceptance of k returned rows c_0 .. c_{count-1} against the exact posteriors e:
  distinct   no pair is listed twice;
  count      count = min(k, the pairs of positive posterior) — a computed value
             is a product of positive doubles far above the subnormals on these
             panels, so it is positive exactly where the posterior is;
  rows       e(c_r) >= e*_r (1 - g) / (1 + g),  g = gamma(2L + 2),
             where e*_r is the (r + 1)-th largest exact posterior counted with
             multiplicity.
Derivation of the row bound.  A list sweep ranks computed pair values, each the
pair's exact value times at most 2L + 2 roundings (map_enumeration: one per
record for the state's product of two transition probabilities and one for
multiplying it into the running value; doublings are exact), so within a factor
1 +- g of it.  The r + 1 exact leaders each have a computed value >=
e*_r (1 - g).  The sweep returns the r + 1 largest computed values, so the
computed value of its row r is at least the smallest of those, >= e*_r (1 - g);
and a computed value is <= e (1 + g).  Dividing every exact value by the same
P(genotype) changes nothing.  Pairs tied at the cut pass by construction:
whichever of them is returned has the posterior e*_r.  The bound is derived,
not tuned.
"""
from __future__ import annotations

from fractions import Fraction

import draw_enumeration as de
import enumeration as en


def ranked_exact(alleles, pt: dict, head_len: int) -> list:
    """Per individual (None where the enumeration does not cover it,
    HEAD_QUIRK): [(pair, posterior)] over every pair of the enumeration, by
    posterior descending, among equals by pair."""
    out = []
    for d in de.pair_posteriors_exact(alleles, pt, head_len):
        out.append(None if d is None else sorted(d.items(), key=lambda kv: (-kv[1], kv[0])))
    return out


def roundings(L: int) -> int:
    return 2 * L + 2


def row_floor(e_star: Fraction, L: int) -> Fraction:
    """The smallest exact posterior the row whose exact counterpart has e_star may have."""
    g = en.gamma(roundings(L))
    return e_star * (1 - g) / (1 + g)


def positive(ranked: list) -> int:
    return sum(1 for _, p in ranked if p > 0)


def reject_reason(keys: list, count: int, k: int, ranked: list, L: int):
    """None if the `count` returned pairs `keys` (row order) are an acceptable
    answer for k rows against `ranked` (ranked_exact of the individual), else
    what is wrong."""
    if count != min(k, positive(ranked)):
        return ("count", count, min(k, positive(ranked)))
    if len(keys) != count:
        return ("rows", len(keys), count)
    if len(set(keys)) != len(keys):
        return ("duplicate", [x for x in keys if keys.count(x) > 1][0])
    post = dict(ranked)
    for r, key in enumerate(keys):
        e_c = post.get(key, Fraction(0))
        if not e_c >= row_floor(ranked[r][1], L):
            return ("row", r, key, float(e_c), float(ranked[r][1]))
    return None


def accepts(keys: list, count: int, k: int, ranked: list, L: int) -> bool:
    return reject_reason(keys, count, k, ranked, L) is None


def het_behind_hom_first(pair) -> bool:
    """A heterozygous pair whose first locus is homozygous: two mirror lattice paths."""
    return pair[0] != pair[1] and pair[0][0] == pair[1][0]
