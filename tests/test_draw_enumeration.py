"""What tests/test_gpu_posterior_draws.py holds the sampler against, checked
without a GPU: the enumerated pair posteriors (tests/draw_enumeration.py) on
the panels of tests/test_enumeration_oracle.py are distributions with mixed
individuals; the generator of the draws (philox.hpp, through
hmc_test_draw_uniform) equals a second, pure-Python Philox4x32-10 written from
the published algorithm, and Random123's known-answer vectors; and the
statistical checker passes true posterior draws and raises on two wrong
samplers at the GPU tests' number of draws.

Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1);
ten times: (hi0, lo0) = 0xD2511F53 x c0, (hi1, lo1) = 0xCD9E8D57 x c2 as 64-bit
products, counter <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); between rounds
the key grows by (0x9E3779B9, 0xBB67AE85) mod 2^32.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hmc_amd  # noqa: E402

import draw_enumeration as de  # noqa: E402
import enumeration as en  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402
from test_switch_enumeration import COUNTS  # noqa: E402

GPU_DRAWS = 16384  # D of tests/test_gpu_posterior_draws.py
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0 = (k0 + 0x9E3779B9) & M32
            k1 = (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def draw_uniform(seed, indiv, draw, step):
    w = philox4x32_10((step, draw, indiv, 0), (seed & M32, seed >> 32))
    return ((w[0] >> 5) * (1 << 26) + (w[1] >> 6)) * 2.0 ** -53


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_library_generator_equals_the_python_one():
    f = hmc_amd.lib().hmc_test_draw_uniform
    imax = 2 ** 31 - 1
    tuples = [(0, 0, 0, 0), (0, imax, imax, imax), (2 ** 64 - 1, imax, imax, imax), (1 << 32, 0, 0, 0), (1, 0, 0, 0),
              ((1 << 63) + 12345, 7, imax, 3), (0xDEADBEEFCAFEF00D, imax, 5, 1), (3, 1, 2, imax)]
    rng = np.random.default_rng(20260)
    for _ in range(300):
        seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        if rng.random() < 0.3:
            seed &= M32  # seeds below 2^32 as well as above
        tuples.append((seed, *(int(x) for x in rng.integers(0, 2 ** 31, 3))))
    assert sum(1 for t in tuples if t[0] >= 2 ** 32) > 100
    seen = set()
    for seed, i, d, s in tuples:
        u = f(seed, i, d, s)
        assert u == draw_uniform(seed, i, d, s), (seed, i, d, s)
        assert 0.0 <= u < 1.0 and u * 2.0 ** 53 == int(u * 2.0 ** 53)
        seen.add(u)
    assert len(seen) == len(set(tuples))
    # the counter's fields are not interchangeable
    assert len({f(9, 1, 2, 3), f(9, 2, 1, 3), f(9, 3, 2, 1), f(9, 1, 3, 2)}) == 4


def m0_posteriors(oracle_mod, name):
    a = build_panel(name)
    hl = head_len(name)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    assert o.head_len() == hl
    return a, hl, de.pair_posteriors_exact(a, o.patterns(), hl)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_enumerated_pair_posteriors(oracle_mod, name):
    a, hl, post = m0_posteriors(oracle_mod, name)
    quirk = en.head_quirk(a, hl)
    ta = en.allele_table(a)
    assert [p is None for p in post] == quirk.tolist()
    for i, d in enumerate(post):
        if d is None:
            continue
        assert sum(d.values()) == 1 and all(p >= 0 for p in d.values())
        for h0, h1 in d:  # every pair is a phasing of the genotype
            assert h0 <= h1
            for k in range(a.shape[2]):
                assert (h0[k], h1[k]) in en.locus_options(a[i], k, [s for s, f in ta[k] if f > 0])
    # the rows swapped: the same distribution
    assert de.pair_posteriors_exact(np.ascontiguousarray(a[:, ::-1]), make_pt(oracle_mod, name, a), hl) == post
    mixed = de.mixed_individuals(post)
    print(name, "individuals with two or more pairs in (0.05, 0.95):", mixed)
    assert len(mixed) >= 1  # the GPU test's statistical part is not vacuous on this panel


def make_pt(oracle_mod, name, a):
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    return o.patterns()


def test_two_locus_known_answer():
    """The table of test_switch_enumeration.test_two_locus_known_answer:
    P(11) = 3/8, P(12) = 1/8, P(22) = 1/4, P(21) = 1/4, so the genotype
    {1, 2} {1, 2} has the pairs {11, 22} of prior 3/16 and {12, 21} of prior
    1/16: posteriors 3/4 and 1/4."""
    one, two = ord("1"), ord("2")
    a = np.array([[[one, one], [two, two]]], np.int32)
    pats = [((one,), 0.5, 1.0), ((two,), 0.5, 1.0), ((one, one), 0.0, 0.75), ((one, two), 0.0, 0.25),
            ((two, two), 0.0, 0.5), ((two, one), 0.0, 0.5)]
    al = np.full((len(pats), 2), -1, np.int32)
    for i, (s, _, _) in enumerate(pats):
        al[i, :len(s)] = s
    pt = dict(start=np.zeros(len(pats), np.int32), len=np.array([len(s) for s, _, _ in pats], np.int32), alleles=al,
              freq=np.array([f for _, f, _ in pats]), tp=np.array([t for _, _, t in pats]))
    assert de.pair_posteriors_exact(a, pt, 1) == [{((one, one), (two, two)): Fraction(3, 4),
                                                   ((one, two), (two, one)): Fraction(1, 4)}]


def test_bernstein_bound():
    """t solves Bernstein's tail for delta: exp(-t^2 / (2 D p q + 2 t / 3)) = delta / 2."""
    import math
    for D, p in ((16384, 0.5), (16384, 0.05), (4096, 0.3), (4096, 1e-4)):
        t = de.bernstein_t(D, p)
        assert math.isclose(2 * math.exp(-t * t / (2 * D * p * (1 - p) + 2 * t / 3)), de.DELTA, rel_tol=1e-9)
    assert de.bernstein_t(16384, 0.5) < 0.03 * 16384  # the bound resolves a few percent at the GPU tests' D


def sample_counts(rng, keys, probs, D):
    c = rng.multinomial(D, probs)
    return {k: int(x) for k, x in zip(keys, c)}


@pytest.mark.parametrize("name", ["snp", "a3"])
def test_checker_has_teeth(oracle_mod, name):
    """numpy draws at the GPU tests' D: from the enumerated posterior they
    pass for every individual; from the uniform distribution over the
    genotype's pairs, and from the posterior with heterozygous pairs at half
    weight (the homozygous-prefix mistake: each of the two lattice paths into
    such a pair taken for the whole pair), the checker raises."""
    a, hl, post = m0_posteriors(oracle_mod, name)
    rng = np.random.default_rng(7)
    raised = {"uniform": [], "half": []}
    differs = []
    for i, d in enumerate(post):
        if d is None:
            continue
        keys = sorted(d)
        p = np.array([float(d[k]) for k in keys])
        de.check_frequencies(sample_counts(rng, keys, p, GPU_DRAWS), GPU_DRAWS, d)
        half = np.array([float(d[k]) * (0.5 if k[0] != k[1] else 1.0) for k in keys])
        half /= half.sum()
        if np.abs(half - p).max() > 0.05:
            differs.append(i)
        for what, q in (("uniform", np.full(len(keys), 1.0 / len(keys))), ("half", half)):
            try:
                de.check_frequencies(sample_counts(rng, keys, q, GPU_DRAWS), GPU_DRAWS, d)
            except de.FrequencyMismatch:
                raised[what].append(i)
    print(name, "raised:", raised, "half-weight distribution differs by > 0.05 for", differs)
    assert len(raised["uniform"]) >= 1
    assert set(differs) <= set(raised["half"])
    if (a < 0).any():
        assert len(raised["half"]) >= 1
    else:
        # snp has no missing allele: an individual's pairs are all heterozygous or it has one pair only, so
        # halving the heterozygous ones and renormalising is the posterior itself — the mistake cannot show in
        # this panel's frequencies (it shows in `prob`, which the GPU test holds against enumeration)
        assert name == "snp" and not differs and not raised["half"]
    # a draw of a pair the posterior excludes raises whatever its count
    i = de.mixed_individuals(post)[0]
    keys = sorted(post[i])
    bogus = dict(sample_counts(rng, keys, np.array([float(post[i][k]) for k in keys]), GPU_DRAWS - 1))
    bogus[((0,), (0,))] = 1
    with pytest.raises(de.FrequencyMismatch):
        de.check_frequencies(bogus, GPU_DRAWS, post[i])
