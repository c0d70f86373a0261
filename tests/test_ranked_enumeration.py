"""What tests/test_gpu_ranked_phasings.py holds hmc_ranked_phasings against,
checked without a GPU: the enumerated ranking (tests/ranked_enumeration.py) on
the panels of tests/test_enumeration_oracle.py and the acceptance predicate —
it accepts the exact list and rejects a list with a duplicate, with a wrong
count, and with a row replaced by a pair further below its exact counterpart
than the bound — and that the panels give the GPU test its cases: individuals
with fewer pairs than rows and with more, heterozygous pairs behind a
homozygous first locus inside the top rows (a sweep that lists both mirror
paths fails there on distinctness), and exact ties inside the top rows.
"""
import os
import sys
from fractions import Fraction

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enumeration as en  # noqa: E402
import ranked_enumeration as re_  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402

K_TOP = 8
NAMES = ["snp", "a3", "a4", "hom", "mc", "short", "minlen2"]
FULL_AT_8 = ("a3", "a4")  # panels on which every enumerated individual has at least 8 pairs
_cache = {}


def ranked_of(oracle_mod, name):
    if name not in _cache:
        a = build_panel(name)
        o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
        o.find_patterns()
        assert o.head_len() == head_len(name)
        _cache[name] = (a, re_.ranked_exact(a, o.patterns(), head_len(name)))
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_predicate(oracle_mod, name):
    a, ranked = ranked_of(oracle_mod, name)
    L = a.shape[2]
    assert [e is None for e in ranked] == en.head_quirk(a, head_len(name)).tolist()
    g = en.gamma(re_.roundings(L))
    assert 0 < g < Fraction(1, 10 ** 14)
    rejected_rows = 0
    for i, e in enumerate(ranked):
        if e is None:
            continue
        assert sum(p for _, p in e) == 1 and all(e[r][1] >= e[r + 1][1] for r in range(len(e) - 1))
        npos = re_.positive(e)
        for k in (1, 4, 8, 16):
            cnt = min(k, npos)
            keys = [key for key, _ in e[:cnt]]
            assert re_.reject_reason(keys, cnt, k, e, L) is None  # the exact list
            if cnt >= 2:  # a duplicate
                assert re_.reject_reason([keys[0]] + keys[:-1], cnt, k, e, L)[0] == "duplicate"
            # a wrong count: a row short, and (where there is a pair to add) a row too many
            if cnt >= 1:
                assert re_.reject_reason(keys[:-1], cnt - 1, k, e, L)[0] == "count"
            if cnt < len(e):
                assert re_.reject_reason(keys + [e[cnt][0]], cnt + 1, k, e, L)[0] == "count"
            # row r replaced by the first pair outside the list that is further below e*_r than the bound
            for r in range(cnt):
                worse = [key for key, p in e[cnt:] if p < re_.row_floor(e[r][1], L)]
                if worse:
                    bad = keys[:r] + [worse[0]] + keys[r + 1:]
                    assert re_.reject_reason(bad, cnt, k, e, L)[:2] == ("row", r)
                    rejected_rows += 1
        # ties at the cut pass: any permutation among equal posteriors is accepted
        keys = [key for key, _ in e[:min(K_TOP, npos)]]
        for r in range(len(keys) - 1):
            if e[r][1] == e[r + 1][1]:
                sw = keys[:r] + [keys[r + 1], keys[r]] + keys[r + 2:]
                assert re_.accepts(sw, len(keys), K_TOP, e, L)
    print(name, "replaced rows the predicate rejected:", rejected_rows)
    assert rejected_rows >= 1


def test_panels_give_the_gpu_test_its_cases(oracle_mod):
    ties = {}
    for name in NAMES:
        a, ranked = ranked_of(oracle_mod, name)
        sizes = [len(e) for e in ranked if e is not None]
        assert min(sizes) >= 1
        # at k = 8: individuals with more pairs than rows on every panel, with fewer on every panel but
        # "a3" (its smallest individual has 10 pairs: fewer than rows at k = 16 only) and "a4" (56: never)
        assert any(re_.positive(e) > K_TOP for e in ranked if e is not None), name
        fewer = any(re_.positive(e) < K_TOP for e in ranked if e is not None)
        assert fewer == (name not in FULL_AT_8), name
        if name == "a3":
            assert any(re_.positive(e) < 16 for e in ranked if e is not None)
        # a heterozygous pair behind a homozygous first locus inside the exact top 8
        mirrors = {i: sum(re_.het_behind_hom_first(key) for key, p in e[:K_TOP] if p > 0)
                   for i, e in enumerate(ranked) if e is not None}
        assert max(mirrors.values()) >= 1, name
        ties[name] = [i for i, e in enumerate(ranked) if e is not None
                      and any(e[r][1] == e[r + 1][1] > 0 for r in range(min(K_TOP, len(e)) - 1))]
        print(name, "pairs per individual", min(sizes), "..", max(sizes), "; mirror pairs in the top 8:", mirrors,
              "; individuals with ties in the top 8:", ties[name])
    # exact ties inside the top 8: several individuals over the panels
    assert sum(len(v) for v in ties.values()) >= 2
