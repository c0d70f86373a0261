"""Switch posteriors between consecutive heterozygous loci by exhaustive
enumeration.

Built on enumeration.estep alone: `priors[{h0, h1}]` over every phasing of an
individual, exact rationals.  A site of an individual is a pair (a, b) of
consecutive loci at which both of its input alleles are present and differ;
every phasing carries the same two alleles at such a locus, one on each
haplotype.  Grouping the priors by whether the haplotype with the lower allele
at a also has the lower allele at b (cis) or not (trans) and dividing by their
total gives the two posteriors — no forward-backward pass, no lattice, no
labels.  "Lower" is by symbol value, which is the order of the allele table
(enumeration.allele_table, GenoData.cpp:78-118).  This module imports neither
the product nor the restatement.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import enumeration as en


def het_loci(g: np.ndarray) -> list:
    """Loci of genotype g[2][L] with both alleles present and different."""
    return [k for k in range(g.shape[1]) if g[0, k] >= 0 and g[1, k] >= 0 and g[0, k] != g[1, k]]


def sites(alleles: np.ndarray) -> list:
    """(individual, locus a, locus b), individual-major, a ascending."""
    out = []
    for i in range(alleles.shape[0]):
        h = het_loci(alleles[i])
        out += [(i, a, b) for a, b in zip(h, h[1:])]
    return out


def switch_posteriors(alleles: np.ndarray, pt: dict, head_len: int) -> dict:
    """{(individual, a, b): (cis, trans)} as Fractions, for every site of every
    individual the enumeration covers (not HEAD_QUIRK)."""
    est = en.estep(alleles, pt, head_len)
    out = {}
    for i, a, b in sites(alleles):
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
