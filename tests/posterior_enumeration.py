"""Genotype posteriors at missing loci by exhaustive enumeration.

Built on enumeration.estep alone: `priors[{h0, h1}]` over every phasing of an
individual and `total`, exact rationals.  Grouping the priors by the
unordered pair of symbols the two haplotypes carry at a locus and dividing by
the total is the posterior of that pair at that locus — no forward-backward
pass, no lattice.  This module imports neither the product nor the restatement.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import enumeration as en


def sites(alleles: np.ndarray) -> list:
    """(individual, locus) with at least one input allele missing,
    individual-major, loci ascending."""
    N, _, L = alleles.shape
    return [(i, k) for i in range(N) for k in range(L) if alleles[i, 0, k] < 0 or alleles[i, 1, k] < 0]


def site_posteriors(alleles: np.ndarray, pt: dict, head_len: int) -> dict:
    """{(individual, locus): {(lo symbol, hi symbol): Fraction}} for every site
    of every individual the enumeration covers (not HEAD_QUIRK).  Pairs of
    probability 0 are listed with 0 when some phasing carries them."""
    est = en.estep(alleles, pt, head_len)
    out = {}
    for i, k in sites(alleles):
        e = est[i]
        if e is None:
            continue
        assert e["total"] > 0
        row: dict = {}
        for (h0, h1), p in e["priors"].items():
            x, y = int(h0[k]), int(h1[k])
            key = (x, y) if x <= y else (y, x)
            row[key] = row.get(key, Fraction(0)) + p
        out[i, k] = {key: p / e["total"] for key, p in row.items()}
    return out
