"""Pair phase posteriors (cis / trans for any two heterozygous loci of an
individual) by exhaustive enumeration.

Built on enumeration.estep alone: `priors[{h0, h1}]` over every phasing of an
individual, exact rationals.  A query is (individual, a, b) with a < b, both
loci heterozygous in the input (both alleles present and different), any
distance apart; every phasing carries the same two alleles at such a locus,
one on each haplotype.  Grouping the priors by whether the haplotype with the
lower allele at a also has the lower allele at b (cis) or not (trans) and
dividing by their total gives the two posteriors, exactly as
switch_enumeration.switch_posteriors groups them for consecutive loci — no
forward-backward pass, no lattice, no labels, no slots.  "Lower" is by symbol
value, which is the order of the allele table (enumeration.allele_table).
This module imports neither the product nor the restatement.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import enumeration as en


def het_loci(g: np.ndarray) -> list:
    """Loci of genotype g[2][L] with both alleles present and different."""
    return [k for k in range(g.shape[1]) if g[0, k] >= 0 and g[1, k] >= 0 and g[0, k] != g[1, k]]


def span_list(alleles: np.ndarray, span: int) -> list:
    """(individual, h_q, h_q+d) for 1 <= d <= span, h1 < h2 < ... the
    individual's heterozygous loci: individual-major, a ascending, then b."""
    assert span >= 1
    out = []
    for i in range(alleles.shape[0]):
        h = het_loci(alleles[i])
        out += [(i, h[q], h[q + d]) for q in range(len(h)) for d in range(1, span + 1) if q + d < len(h)]
    return out


def all_pairs(alleles: np.ndarray) -> list:
    """Every pair of heterozygous loci of every individual (span_list with no limit)."""
    return span_list(alleles, max(1, alleles.shape[2]))


def max_overlap(queries) -> int:
    """The largest number of anchor intervals [a, largest b asked for a] of one
    individual that are open between two adjacent loci: the slots a sweep
    needs to answer the individual's queries in one round."""
    far = {}
    for i, a, b in queries:
        far[i, a] = max(far.get((i, a), b), b)
    worst = 0
    for (i, a), b in far.items():
        # intervals of i open just after locus a (an interval that ends at a is freed before a is anchored)
        worst = max(worst, sum(1 for (i2, a2), b2 in far.items() if i2 == i and a2 <= a < b2))
    return worst


def pair_posteriors(alleles: np.ndarray, pt: dict, head_len: int, queries) -> dict:
    """{(individual, a, b): (cis, trans)} as Fractions for the given queries of
    the individuals the enumeration covers (not HEAD_QUIRK)."""
    est = en.estep(alleles, pt, head_len)
    out = {}
    for i, a, b in queries:
        het = het_loci(alleles[i])
        assert a < b and a in het and b in het, (i, a, b)
        e = est[i]
        if e is None:
            continue
        tot = sum(e["priors"].values(), Fraction(0))
        assert tot == e["total"] > 0
        cis = trans = Fraction(0)
        for (h0, h1), p in e["priors"].items():
            assert h0[a] != h1[a] and h0[b] != h1[b]
            if (h0[a] < h1[a]) == (h0[b] < h1[b]):
                cis += p
            else:
                trans += p
        out[i, a, b] = (cis / tot, trans / tot)
    return out
