"""What tests/test_gpu_map_phase.py holds hmc_map_phase against, checked
without a GPU: the enumerated maximum a-posteriori pairs
(tests/map_enumeration.py) on panels of tests/test_enumeration_oracle.py, and
the acceptance predicate: it accepts every exact maximiser and rejects the
second-best pair wherever the top two posteriors are further apart than the
bound — which happens on every panel used, so the GPU test is not vacuous.
Also where the E-step's k-best beam misses the maximiser (the restatement's
resolutions against the enumerator): on none of the seven panel / sample-size
cases the GPU test shares with the posterior draws, on two individuals of
"hom" at sample size 1, the case the GPU test adds for it.
"""
import os
import sys
from fractions import Fraction

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import draw_enumeration as de  # noqa: E402
import enumeration as en  # noqa: E402
import map_enumeration as me  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402


def m0_table(oracle_mod, name, S):
    a = build_panel(name)
    o = make_oracle(oracle_mod, name, S, a)
    o.find_patterns()
    assert o.head_len() == head_len(name)
    return a, o


@pytest.mark.parametrize("name", ["snp", "a3", "hom"])
def test_enumerated_map_and_predicate(oracle_mod, name):
    a, o = m0_table(oracle_mod, name, PANELS[name]["S"][0])
    hl, L = head_len(name), a.shape[2]
    mp = me.map_pairs_exact(a, o.patterns(), hl)
    assert [e is None for e in mp] == en.head_quirk(a, hl).tolist()
    g = en.gamma(me.map_roundings(L))
    assert 0 < g < Fraction(1, 10 ** 14)
    separated = []
    for i, e in enumerate(mp):
        if e is None:
            continue
        assert e["argmax"] and 0 < e["best"] <= 1 and sum(e["post"].values()) == 1
        assert e["best"] == max(e["post"].values())
        for k in e["argmax"]:  # every exact maximiser is accepted
            assert me.accepts(e["post"][k], e["best"], L)
        assert me.map_floor(e["best"], L) < e["best"]
        sb = me.second_best(e)
        if sb is None:
            assert len(e["argmax"]) == len(e["post"])
            continue
        k2, p2 = sb
        assert k2 not in e["argmax"] and p2 < e["best"]
        if p2 < me.map_floor(e["best"], L):  # further apart than the bound: rejected
            assert not me.accepts(p2, e["best"], L)
            separated.append(i)
        assert not me.accepts(Fraction(0), e["best"], L)
    print(name, "individuals whose second-best pair the predicate rejects:", separated)
    assert len(separated) >= 1


def beam_misses(oracle_mod, name, S):
    a, o = m0_table(oracle_mod, name, S)
    pt = o.patterns()
    o.resolve_all()
    res = o.resolutions()
    miss, ratio = [], Fraction(1)
    for i, e in enumerate(me.map_pairs_exact(a, pt, head_len(name))):
        if e is None:
            continue
        k = de.pair_key(res[i][0], res[i][1])
        p = e["post"].get(k, 0)
        assert p > 0
        if k not in e["argmax"]:
            miss.append(i)
            ratio = max(ratio, e["best"] / p)
    return miss, float(ratio)


def test_where_the_beam_misses_the_map_pair(oracle_mod):
    """The best pair of the k-best list (resolutions) against the enumerated
    maximiser: found on every one of the draws' seven cases, missed on "hom"
    with one state kept per locus."""
    from_draws = [("snp", 2), ("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5), ("minlen2", 10)]
    for name, S in from_draws:
        assert beam_misses(oracle_mod, name, S) == ([], 1.0), (name, S)
    miss, ratio = beam_misses(oracle_mod, "hom", 1)
    print("hom, S = 1: beam misses individuals", miss, "largest e* / e(selected) =", ratio)
    assert miss == [1, 2] and 1.5 < ratio < 1.52
