"""Posterior of whole haplotype pairs by exhaustive enumeration, and the
statistical check of a sampler against it.

Built on enumeration.estep alone: `priors[{h0, h1}]` over every phasing of an
individual, exact rationals; dividing by their total gives the posterior of
each unordered pair — what one posterior draw is a sample of.  This module
imports neither the product nor the restatement.

check_frequencies: a sampler that draws D independent pairs from the posterior
p gives each pair a Binomial(D, p) count.  Bernstein's inequality for a sum of
D independent terms bounded by 1 with variance p (1 - p) each,
    P(|count - D p| > t) <= 2 exp(-t^2 / (2 D p (1 - p) + 2 t / 3)),
solved for a two-sided tail of delta with lambda = ln(2 / delta):
    t = lambda / 3 + sqrt((lambda / 3)^2 + 2 D p (1 - p) lambda).
With delta = 1e-12 and at most about 1e5 comparisons in a whole run a correct
sampler fails with probability below 1e-6 — once and for all, since the seeds
are fixed.  The bound is derived, not tuned.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import enumeration as en

DELTA = 1e-12


def pair_posteriors_exact(alleles: np.ndarray, pt: dict, head_len: int) -> list:
    """Per individual {unordered pair (h0 <= h1): priors / total} as Fractions
    (None for the individuals the enumeration does not cover, HEAD_QUIRK)."""
    out = []
    for e in en.estep(alleles, pt, head_len):
        if e is None:
            out.append(None)
            continue
        tot = sum(e["priors"].values(), Fraction(0))
        assert tot == e["total"] > 0
        out.append({k: p / tot for k, p in e["priors"].items()})
    return out


def bernstein_t(D: int, p: float, delta: float = DELTA) -> float:
    lam = math.log(2.0 / delta)
    return lam / 3.0 + math.sqrt((lam / 3.0) ** 2 + 2.0 * D * p * (1.0 - p) * lam)


class FrequencyMismatch(AssertionError):
    """A pair's count is outside Bernstein's bound of D times its posterior."""


def check_frequencies(counts: dict, D: int, exact: dict, delta: float = DELTA) -> int:
    """counts[key] draws out of D against exact[key] (Fractions or floats that
    sum to 1): |count - D p| <= t(p) for every key of `exact`, count 0 where
    p = 0, and no draw outside `exact`.  Returns the number of comparisons."""
    for k, c in counts.items():
        if c and not exact.get(k, 0) > 0:
            raise FrequencyMismatch(("drawn with posterior 0", k, c))
    assert sum(counts.values()) == D, (sum(counts.values()), D)
    n = 0
    for k, p in exact.items():
        c = counts.get(k, 0)
        n += 1
        if p == 0:
            continue  # (count 0: checked above)
        t = bernstein_t(D, float(p), delta)
        if abs(c - D * float(p)) > t:
            raise FrequencyMismatch((k, c, D * float(p), t))
    return n


def mixed_individuals(post: list, lo=Fraction(5, 100), hi=Fraction(95, 100)) -> list:
    """Individuals with two or more pairs of posterior in (lo, hi)."""
    return [i for i, d in enumerate(post) if d is not None and sum(1 for p in d.values() if lo < p < hi) >= 2]


def pair_key(h0, h1) -> tuple:
    """The unordered pair of two haplotypes (sequences of symbols) as estep keys it."""
    a, b = tuple(int(x) for x in h0), tuple(int(x) for x in h1)
    return (a, b) if a <= b else (b, a)
