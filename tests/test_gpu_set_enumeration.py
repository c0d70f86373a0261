"""The library's pattern *sets* against tests/set_enumeration.py: the cases of
tests/test_set_enumeration_oracle.py with hmc_amd.HaploModel in place of the
CPU restatement, which this file never touches.

The exact M-step (`exact_estimate`: candidate rounds on the host, frequencies
from the device trie walk) and findPatternByNum (`num_patterns`: the device
candidate tree replayed on the host) each choose which patterns stay and in
which order; both choices are compared with the reference's rules applied to
exactly enumerated frequencies.  After every exact M-step one more E-step
runs on the new table and is held to enumeration too.

Every panel is at most 12 individuals x 10 loci; the enumeration is cached
across cases.
"""
import time
from fractions import Fraction

import numpy as np
import pytest

import hmc_amd

import enumeration as en
import set_enumeration as sen
from test_enumeration_oracle import PANELS, build_panel, head_len, mining_params
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_set_enumeration_oracle import (BYNUM_CASES, BYNUM_MAX_LEN, BYNUM_MIN_LEN, BYNUM_S, SEEDED, bynum_panel,
                                         check_bynum, check_estep_after, check_exact_step, hand_panel, seeded_table)

pytestmark = pytest.mark.gpu


def bynum_model(a, num, S=BYNUM_S, max_len=BYNUM_MAX_LEN, exact=False):
    m = hmc_amd.HaploModel()
    m.sample_size = S
    m.min_pattern_len = BYNUM_MIN_LEN
    m.max_pattern_len = max_len
    m.num_patterns = num
    m.exact_estimate = exact
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * a.shape[2]))
    return m


def exact_step(m):
    """One exact M-step on the last E-step; (table, stats)."""
    assert m.exact_estimate
    m.find_patterns()
    return m.patterns(), m.exact_stats()


def assert_estimated(stats, info):
    """The library estimated what the definition estimated: as many rounds
    with something to estimate, as many candidates."""
    assert stats["rounds"] == info["rounds"], (stats["rounds"], info["rounds"])
    assert stats["candidates"] == info["candidates"], (stats["candidates"], info["candidates"])


@pytest.mark.parametrize("name", sorted(PANELS))
def test_exact_mstep_set(name):
    """Two consecutive exact M-steps after M0 and E1: set, order, successors
    and numbers of each table, and the E-step on it."""
    t0 = time.time()
    a = build_panel(name, quirk=False)
    S, hl = PANELS[name]["S"][-1], head_len(name)
    m = gpu_model(name, S, a)
    m.exact_estimate = True
    m.find_patterns()
    params = mining_params(name, a.shape[0])
    m.resolve_all()
    for step in (1, 2):
        prev = m.patterns()
        new, stats = exact_step(m)
        tag = f"{name} step {step}:"
        info = check_exact_step(tag, new, a, prev, hl, params, True)
        assert_estimated(stats, info)
        if PANELS[name].get("model") == "MC":
            assert sen.table_keys(new) == sen.table_keys(prev)
        else:
            assert info["added"][-1] == 0 and info["candidates"] > len(prev["start"])
        check_estep_after(tag, gpu_view(m), a, new, hl, S)
    print(name, "%.1f s" % (time.time() - t0))


@pytest.mark.parametrize("name,seam", [("a3", "last_symbols"), ("a3", "spelled"), ("minlen2", "spelled")])
def test_exact_mstep_set_from_short_table(name, seam):
    """From a table cut to its patterns of length <= head_len, through
    set_patterns: three estimation rounds, work left for the second
    extendPatterns.  A table of single alleles goes through either seam; with
    head_len 2 the heads' strings are needed, which only the spelled one has."""
    t0 = time.time()
    a = build_panel(name, quirk=False)
    S, hl = PANELS[name]["S"][-1], head_len(name)
    m0 = gpu_model(name, S, a)
    m0.find_patterns()
    cut = seeded_table(m0.patterns(), a, hl)
    m = gpu_model(name, S, a)
    m.exact_estimate = True
    if seam == "spelled":
        m.set_patterns_spelled(cut)
    else:
        feed(m, cut)
    assert sen.table_keys(m.patterns()) == sen.table_keys(cut)
    m.resolve_all()
    new, stats = exact_step(m)
    info = check_exact_step(f"{name} seeded ({seam}):", new, a, cut, hl, mining_params(name, a.shape[0]), True)
    assert info["rounds"] == 3 and info["added"][1] >= 1 and info["added"][2] == 0
    assert_estimated(stats, info)
    assert stats["rounds"] == 3
    check_estep_after(f"{name} seeded ({seam}):", gpu_view(m), a, new, hl, S)
    print(name, seam, "%.1f s" % (time.time() - t0))


@pytest.mark.parametrize("panel,num", BYNUM_CASES)
def test_find_patterns_by_num(panel, num):
    """M0 from the genotypes and M1 from the samples of E1."""
    t0 = time.time()
    a = bynum_panel(panel)
    m = bynum_model(a, num)
    m.find_patterns()
    _, i0 = check_bynum(f"{panel} {num} M0:", m.patterns(), a, num)
    _, H, _ = m.resolve_all()
    al, w, _ = m.samples(H)
    m.find_patterns()
    _, i1 = check_bynum(f"{panel} {num} M1:", m.patterns(), a, num, samples=(al, w))
    if (panel, num) == ("miss", 25):
        assert i0["rounds"] == i1["rounds"] == 11 and i0["cut_gap"] is None and i1["cut_gap"] is None
    if (panel, num) == ("miss", 60):
        assert (i0["rounds"], i1["rounds"]) == (23, 24) and i0["cut_gap"] is not None and i1["cut_gap"] is not None
    print(panel, num, "%.1f s" % (time.time() - t0))


def test_exact_mstep_after_find_patterns_by_num():
    """The exact M-step after findPatternByNum filters by the search's last
    threshold."""
    t0 = time.time()
    panel, num = "miss", 60
    a = bynum_panel(panel, quirk=False)
    m = bynum_model(a, num, exact=True)
    m.find_patterns()
    prev = m.patterns()
    _, info = check_bynum(f"{panel} {num} (locus 0 complete) M0:", prev, a, num)
    assert info["rounds"] > 2 and info["last_threshold"] < 0.5
    m.resolve_all()
    new, stats = exact_step(m)
    minfo = check_exact_step(f"{panel} {num} after ByNum:", new, a, prev, 1,
                             (Fraction(info["last_threshold"]), BYNUM_MIN_LEN, BYNUM_MAX_LEN), True)
    assert_estimated(stats, minfo)
    check_estep_after(f"{panel} {num} after ByNum:", gpu_view(m), a, new, 1, BYNUM_S)
    print(panel, num, "%.1f s" % (time.time() - t0))


def test_exact_mstep_after_exhausted_search():
    """A search that runs out of candidates below max_num patterns leaves the
    threshold at 1e-38 (PatternManager.cpp:58-62), and the exact M-step after
    it keeps every candidate of positive frequency."""
    a, _ = hand_panel()
    m = bynum_model(a, 10, S=2, exact=True)
    m.find_patterns()
    prev = m.patterns()
    _, info = check_bynum("hand 10 M0:", prev, a, 10)
    assert info["patterns"] == 8 and info["last_threshold"] <= 1e-38
    m.resolve_all()
    new, stats = exact_step(m)
    minfo = check_exact_step("hand 10 after an exhausted search:", new, a, prev, 1,
                             (Fraction(info["last_threshold"]), 1, 30), True)
    assert_estimated(stats, minfo)
    assert minfo["kept"] == 28


def test_negative_control():
    """The check raises on the library's own table with one kept pattern
    removed (successors rebuilt, so only the set is at fault)."""
    name = "a3"
    a = build_panel(name, quirk=False)
    m = gpu_model(name, PANELS[name]["S"][-1], a)
    m.exact_estimate = True
    m.find_patterns()
    prev = m.patterns()
    m.resolve_all()
    new, _ = exact_step(m)
    kept, info = sen.estimate_patterns_set(a, prev, 1, *mining_params(name, a.shape[0]))
    sen.check_pattern_set(new, kept, info, a)
    longest = max(range(len(kept)), key=lambda i: len(kept[i][1]))
    bad = {k: np.ascontiguousarray(np.delete(v, longest, axis=0)) for k, v in new.items()}
    succ = en.rebuild_successors(bad, en.allele_table(a), a.shape[2])
    bad["succ"] = np.pad(succ, ((0, 0), (0, new["succ"].shape[1] - succ.shape[1])), constant_values=-1)
    with pytest.raises(AssertionError):
        sen.check_pattern_set(bad, kept, info, a)
