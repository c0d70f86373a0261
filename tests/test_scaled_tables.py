"""Underflow at enumerable sizes: the scaled tables the extended-range tests
(tests/test_gpu_extended_range.py) run on.  No GPU here: this file holds the
trick itself and guards that those tests are not vacuous.

The enumerated prior of a haplotype is freq[head] x the product of one tp per
further locus (enumeration.Table.chain_prob), so with head_len = 1 every
haplotype of an L-locus panel has L factors.  Multiplying every pattern's freq
and tp by 2^-c is exact in double (the smallest tp of these panels is 0.05:
nothing comes near the subnormal range) and multiplies every phasing's prior
P(h0) P(h1) by the same 2^(-2 c L): every total scales by exactly that power
and every posterior — a ratio of such sums — is unchanged.  With c large enough
the totals leave the range of a double while the panel stays enumerable in
exact rationals: the regular posterior family gives such a panel up (status 1
where P(genotype) is 0 as a double, status 2 where it is subnormal), the
extended range must not.

Asserted below for the five panels with head_len 1 (an injected table needs
head_len 1), individuals without the head quirk:
  ZERO_C = 100     every total is 0 as a double;
  SUBNORMAL_C      every total is positive and below 2^-1022 as a double:
                   snp 52 (12 of 12), short 52 (11 of 11), a3 64 (9 of 9),
                   hom 64 (10 of 10), a4 86 (7 of 7; L = 6: 2^-1032 times totals
                   between 2^-4.8 and 2^-12.3).
"""
from fractions import Fraction

import numpy as np
import pytest

import enumeration as en
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle

ZERO_C = 100
SUBNORMAL_C = {"snp": 52, "short": 52, "a3": 64, "hom": 64, "a4": 86}
# individuals without the head quirk: all of them have a subnormal total at SUBNORMAL_C and a zero one at ZERO_C
INDIVIDUALS = {"snp": 12, "short": 11, "a3": 9, "hom": 10, "a4": 7}
SCALED_PANELS = sorted(SUBNORMAL_C)
DBL_MIN = Fraction(1, 2 ** 1022)


def scaled(pt, c):
    """The table with every freq and tp times 2^-c (exact: asserted)."""
    out = {k: v.copy() for k, v in pt.items()}
    f = 2.0 ** -c
    out["freq"] = pt["freq"] * f
    out["tp"] = pt["tp"] * f
    for k in ("freq", "tp"):
        assert all(Fraction(float(y)) * 2 ** c == Fraction(float(x)) for x, y in zip(pt[k], out[k])), k
        assert all(y == 0 or abs(y) >= 2.0 ** -1022 for y in out[k]), k  # nothing subnormal in the table itself
    return out


def prior_shift(c, L, hl=1):
    """log2 of the factor between a phasing's prior on the table and on scaled(table, c)."""
    return 2 * c * (L - hl + 1)


def test_panels_have_head_len_one():
    for name in SCALED_PANELS:
        assert head_len(name) == 1
    assert sorted(n for n in PANELS if head_len(n) == 1) == SCALED_PANELS


@pytest.mark.parametrize("name", SCALED_PANELS)
def test_scaling_is_exact_and_underflows(oracle_mod, name):
    a = build_panel(name)
    L = a.shape[2]
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    pt = o.patterns()
    assert float(pt["tp"][pt["tp"] > 0].min()) >= 0.05
    base = en.estep(a, pt, 1)
    live = [i for i, e in enumerate(base) if e is not None]
    assert len(live) == INDIVIDUALS[name]
    assert all(base[i]["total"] > 0 for i in live)
    seen = {}
    for c in (SUBNORMAL_C[name], ZERO_C):
        sc = en.estep(a, scaled(pt, c), 1)
        k = 2 ** prior_shift(c, L)
        for i in live:
            assert sc[i]["M"] == base[i]["M"]
            assert sc[i]["total"] * k == base[i]["total"]
            assert sc[i]["priors"].keys() == base[i]["priors"].keys()
            assert all(sc[i]["priors"][h] * k == p for h, p in base[i]["priors"].items())
        as_double = [float(sc[i]["total"]) for i in live]
        seen[c] = (sum(1 for t in as_double if t == 0.0), sum(1 for t, i in zip(as_double, live) if 0 < sc[i]["total"] < DBL_MIN and t > 0))
    print(name, "L", L, "individuals", len(live), {c: dict(zero=z, subnormal=s) for c, (z, s) in seen.items()},
          "log2 total", [round(float(np.log2(float(base[i]["total"]))), 1) for i in live])
    assert seen[ZERO_C] == (len(live), 0)
    assert seen[SUBNORMAL_C[name]] == (0, len(live))
