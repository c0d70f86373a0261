"""The CPU restatement's pattern *sets* against tests/set_enumeration.py.

test_enumeration_oracle.py pins freq / prefix / tp of whatever patterns an
exact M-step kept; which patterns it keeps and in which order, and the whole
of findPatternByNum, were library against restatement only.  Here both
selection rules are held to definitions that share nothing with either: the
seed rule, the four-level extension rounds on inherited frequencies and the
final filter of PatternManager::estimatePatterns (PatternManager.cpp:364-438),
and the thresholds, reserved candidates, sorted tail and cut of
findPatternByNum (:44-70), on exactly enumerated frequencies.
tests/test_gpu_set_enumeration.py runs the same cases on the library.

A set decided by exact frequencies can be demanded of an implementation that
decides in doubles only where no candidate is near a threshold; those
conditions are asserted (set_enumeration.check_pattern_set), and the panels
and sizes are chosen so that the enumeration alone meets them.
"""
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enumeration as en  # noqa: E402
import set_enumeration as sen  # noqa: E402
from hmc_amd import synth  # noqa: E402
from test_enumeration_oracle import (PANELS, build_panel, head_len, make_oracle, mining_params,  # noqa: E402
                                     oracle_view)

# On `snp` (no missing data) twelve candidates of the seeded table equal min_freq = 1/16 exactly,
# and the fixed-point walk cannot be expected to land on the threshold: not usable for the set.
SEEDED = ["a3", "minlen2"]
# findPatternByNum: (panel, num_patterns).  `miss` reaches 11 rounds without a cut (num 25) and 23
# (M0) / 24 (M1) rounds with a sorted, cut tail (num 60).  Panels without missing data and without
# monomorphic stretches are degenerate — every length-min_len pattern is stored unextended in round
# 1 and nothing is reserved — so `full` is one case.
BYNUM_PANELS = {
    "miss": dict(N=12, L=10, A=2, K=3, rho=0.1, missing=0.08, seed=7),
    "full": dict(N=12, L=10, A=2, K=3, rho=0.1, missing=0.0, seed=5),
}
BYNUM_CASES = [("miss", 25), ("miss", 60), ("full", 20)]
BYNUM_S, BYNUM_MIN_LEN, BYNUM_MAX_LEN = 5, 1, 30


def bynum_panel(name, quirk=True):
    """alleles[N][2][L]; without `quirk` the missing alleles of locus 0 are put
    back from the same mosaic drawn without missing data (the exact M-step
    sums over everyone: no enumeration.HEAD_QUIRK individuals)."""
    g = BYNUM_PANELS[name]
    a = synth.founder_mosaic(**g).alleles.copy()
    if not quirk:
        a[:, :, 0] = synth.founder_mosaic(**dict(g, missing=0.0)).alleles[:, :, 0]
        assert not en.head_quirk(a, 1).any() and (a < 0).any()
    ta = en.allele_table(a)
    assert max(en.phasing_count(a[i], ta) for i in range(a.shape[0])) <= en.MAX_PHASINGS
    return a


def seeded_table(pt, a, hl):
    """The patterns of length <= head_len of a mined table, successors rebuilt
    by the rule: every extension the E-step needs is missing, so the exact
    M-step has to grow the table back over several rounds."""
    keep = [i for i in range(len(pt["len"])) if pt["len"][i] <= hl]
    assert 0 < len(keep) < len(pt["len"])
    cut = {k: np.ascontiguousarray(v[keep]) for k, v in pt.items()}
    cut["succ"] = en.rebuild_successors(cut, en.allele_table(a), a.shape[2])
    if cut["succ"].shape[1] < pt["succ"].shape[1]:
        cut["succ"] = np.pad(cut["succ"], ((0, 0), (0, pt["succ"].shape[1] - cut["succ"].shape[1])), constant_values=-1)
    return cut


def check_exact_step(tag, new, a, prev, hl, params, fixed_point, t0=None):
    """One exact M-step's table: the enumerated set and order, the successors,
    and the numbers (check_mstep).  Returns the enumeration's info."""
    t0 = time.time() if t0 is None else t0
    kept, info = sen.estimate_patterns_set(a, prev, hl, *params)
    sen.check_pattern_set(new, kept, info, a)
    worst = en.check_mstep(new, a, prev, hl, fixed_point=fixed_point)
    assert worst["loosest_rel_bound"] <= 1e-9
    print(tag, "rounds", info["rounds"], "added", info["added"], "candidates", info["candidates"], "kept", info["kept"],
          "margin %.2g" % info["margin"], "equal", info["equal"], "loosest bound %.2g" % worst["loosest_rel_bound"],
          "%.1f s" % (time.time() - t0))
    return info


def check_estep_after(tag, view, a, new, hl, S):
    """The E-step on an exactly estimated table, against enumeration; on such
    a table the successor chain need not equal the global longest match."""
    t0 = time.time()
    out = en.check_estep(view, a, new, hl, S)
    print(tag, "E-step on the new table:", {k: (round(v, 2) if isinstance(v, float) else v) for k, v in out.items()},
          "chain != global for", en.check_chain_equals_global(a, new, hl), "haplotypes", "%.1f s" % (time.time() - t0))


def print_bynum(tag, info, t0):
    print(tag, "rounds", info["rounds"], "visited", info["visited"], "patterns", info["patterns"], "last_size",
          info["last_size"], "last threshold %.6g" % info["last_threshold"], "margin %.2g" % info["margin"], "equal",
          info["equal"], "equal at 1.0", info["equal_at_one"], "cut gap", info["cut_gap"], "tail gap", info["tail_gap"],
          "%.1f s" % (time.time() - t0))


# ------------------------------------------------- the definitions themselves ----
def hand_panel():
    """Four homozygous individuals over four loci: haplotypes 0000, 0001, 0010,
    1111.  Each has one phasing, so whatever the previous table, a pattern's
    expectation is the number of individuals whose haplotype has it.  The
    previous table: the eight single alleles, in (start, symbol) order."""
    haps = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 1, 1, 1)]
    a = np.array([[h, h] for h in haps], np.int32)
    ta = en.allele_table(a)
    keys = [(k, (s,)) for k in range(4) for s in (0, 1)]
    fr = np.array([float(dict(ta[k])[s[0]]) for k, s in keys])
    prev = dict(start=np.array([k for k, _ in keys], np.int32), len=np.ones(8, np.int32),
                alleles=np.array([[s[0]] for _, s in keys], np.int32), freq=fr, prefix=np.ones(8), tp=fr.copy())
    return a, prev


def test_estimate_patterns_set_by_hand():
    """min_freq = 3/8: a pattern passes with two individuals or more.

    Candidates in creation order: each single allele of loci 0-2 followed by
    its two extensions (the successor, a single allele, starts elsewhere: a
    seed), then the two of locus 3: 8 + 12 = 20.  Counts of the seeds: (0,00)
    3, (0,01) 0, (0,10) 0, (0,11) 1, (1,00) 2, (1,01) 1, (1,10) 0, (1,11) 1,
    (2,00) (2,01) (2,10) (2,11) 1 each.  Round 1: level 1 extends (0,00) and
    (1,00) to (0,000) (0,001) (1,000) (1,001); level 2 extends (0,000) *and*
    (0,001) — count 1, below min_freq, but it carries (0,00)'s 3/4 — to
    (0,0000) (0,0001) (0,0010) (0,0011); (1,000) and (1,001) end at L.  Eight
    added, none of them extensible: round 2 adds nothing.  Of the added only
    (0,000) has two individuals; the single alleles stay by length, (0,1) with
    1/4 included."""
    a, prev = hand_panel()
    kept, info = sen.estimate_patterns_set(a, prev, 1, Fraction(3, 8), 1, 30)
    assert kept == [(0, (0,)), (0, (0, 0)), (0, (1,)), (1, (0,)), (1, (0, 0)), (1, (1,)), (2, (0,)), (2, (1,)),
                    (3, (0,)), (3, (1,)), (0, (0, 0, 0))]
    assert info == dict(rounds=2, added=[8, 0], candidates=28, kept=11, equal=0, margin=float(Fraction(1, 3)))
    # the level-2 extension of a parent below min_freq was created (it is estimated: in the memo) and dropped
    ex = en.mstep(a, prev, 1, [(0, (0, 0, 1)), (0, (0, 0, 1, 0))])
    assert ex[0, (0, 0, 1)] == (1, 3) and ex[0, (0, 0, 1, 0)] == (1, 1)
    assert (0, (0, 0, 1, 0)) not in kept
    # max_len 3 stops level 2; min_len 2 drops nothing more (every single allele is <= min_len)
    kept3, info3 = sen.estimate_patterns_set(a, prev, 1, Fraction(3, 8), 1, 3)
    assert kept3 == kept and info3["added"] == [4, 0] and info3["candidates"] == 24
    # an equal candidate is counted: min_freq = 1/2 is (0,000)'s and (1,00)'s frequency, and four single alleles'
    assert sen.estimate_patterns_set(a, prev, 1, Fraction(1, 2), 1, 30)[1]["equal"] == 6
    # min_freq < 0: estimateFrequency, in place
    assert sen.estimate_patterns_set(a, prev, 1, Fraction(-1), 1, 30)[0] == sen.table_keys(prev)


def test_find_patterns_by_num_by_hand():
    """On the same panel with min_len 1 no single allele reaches 1.0: the first
    search stores all eight unextended (length == min_len) and reserves
    nothing, so although (0,00) has frequency 3/4 and max_num asks for more,
    no later threshold finds it; the thresholds run down to 1e-38.  Roots and
    alleles are popped from the back: start 3 first, symbol 1 before 0."""
    a, _ = hand_panel()
    pats, info = sen.find_patterns_by_num(a, 10, 1, 30)
    assert [k for k, _ in pats] == [(k, (s,)) for k in (3, 2, 1, 0) for s in (1, 0)]
    assert [f for _, f in pats] == [Fraction(c, 4) for c in (2, 2, 2, 2, 1, 3, 1, 3)]
    assert info["last_size"] == 8 and info["sorted_from"] is None and info["cut_gap"] is None
    assert info["last_threshold"] <= 1e-38 < info["last_threshold"] / 0.9 and info["rounds"] > 800
    assert info["margin"] == 0.25 and info["equal"] == 0  # 3/4 against 1.0
    # min_len 2: the single alleles are extended whatever their frequency and every pair of symbols
    # is stored in round 1 (length == min_len), those no haplotype has included
    pats2, _ = sen.find_patterns_by_num(a, 1, 2, 30)
    assert sorted(k for k, _ in pats2) == sorted((s, (x, y)) for s in range(3) for x in (0, 1) for y in (0, 1))
    assert dict(pats2)[0, (0, 1)] == 0
    # max_num below the first round's size: max(max_num, size), nothing cut
    assert len(sen.find_patterns_by_num(a, 3, 1, 30)[0]) == 8
    # a locus everyone shares reaches 1.0 and is extended in round 1: (0,00) with 3/4 and (0,01) with
    # 1/4 are reserved, and (0,00) comes in at the first threshold below it, 0.9^3 = 0.729 in doubles
    b = a.copy()
    b[:, :, 0] = 0
    pats3, info3 = sen.find_patterns_by_num(b, 8, 1, 30)
    assert [k for k, _ in pats3] == [(3, (1,)), (3, (0,)), (2, (1,)), (2, (0,)), (1, (1,)), (1, (0,)), (0, (0,)),
                                     (0, (0, 0))]
    assert info3["equal_at_one"] == 1 and info3["equal"] == 0 and info3["rounds"] == 4 and info3["last_size"] == 7
    assert info3["last_threshold"] == 1.0 * 0.9 * 0.9 * 0.9 and info3["sorted_from"] is None


def test_thresholds_are_the_reference_doubles():
    th = sen.thresholds()
    seq = [next(th) for _ in range(4)]
    assert seq == [1.0, 0.9, 0.9 * 0.9, 0.9 * 0.9 * 0.9]
    assert Fraction(seq[3]) != Fraction(729, 1000)


# ------------------------------------------------------------ exact M-step ----
@pytest.mark.parametrize("mode", ["reference", "device"])
@pytest.mark.parametrize("name", sorted(PANELS))
def test_exact_mstep_set(oracle_mod, name, mode):
    """Two consecutive exact M-steps after M0 and E1: the kept set and its
    order at each, in both summation orders.  MC re-estimates in place."""
    a = build_panel(name, quirk=False)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][-1], a)
    o.set_exact_order(mode)
    o.find_patterns()
    params = mining_params(name, a.shape[0])
    S, hl = PANELS[name]["S"][-1], head_len(name)
    o.resolve_all()
    for step in (1, 2):
        prev = o.patterns()
        o.estimate_patterns()
        new = o.patterns()
        tag = f"{name} {mode} step {step}:"
        info = check_exact_step(tag, new, a, prev, hl, params, mode == "device")
        if PANELS[name].get("model") == "MC":
            assert sen.table_keys(new) == sen.table_keys(prev)
        else:
            assert info["added"][-1] == 0 and info["candidates"] > len(prev["start"])
        check_estep_after(tag, oracle_view(o, o.resolve_all()), a, new, hl, S)


@pytest.mark.parametrize("mode", ["reference", "device"])
@pytest.mark.parametrize("name", SEEDED)
def test_exact_mstep_set_from_short_table(oracle_mod, name, mode):
    """From a table cut to its patterns of length <= head_len the M-step needs
    three estimation rounds: the second extendPatterns, which starts from the
    last level of the first alone, still has work."""
    a = build_panel(name, quirk=False)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][-1], a)
    o.set_exact_order(mode)
    o.find_patterns()
    cut = seeded_table(o.patterns(), a, head_len(name))
    o.set_patterns(cut)
    o.resolve_all()
    o.estimate_patterns()
    new = o.patterns()
    info = check_exact_step(f"{name} {mode} seeded:", new, a, cut, head_len(name), mining_params(name, a.shape[0]),
                            mode == "device")
    assert info["rounds"] == 3 and info["added"][1] >= 1 and info["added"][2] == 0
    check_estep_after(f"{name} {mode} seeded:", oracle_view(o, o.resolve_all()), a, new, head_len(name),
                      PANELS[name]["S"][-1])


# -------------------------------------------------------- findPatternByNum ----
def bynum_oracle(oracle_mod, a, num):
    o = oracle_mod.Oracle(a, "S" * a.shape[2], min_len=BYNUM_MIN_LEN, max_len=BYNUM_MAX_LEN, sample_size=BYNUM_S)
    o.set_num_patterns(num)
    return o


def check_bynum(tag, pt, a, num, samples=None, max_len=BYNUM_MAX_LEN):
    t0 = time.time()
    pats, info = sen.find_patterns_by_num(a, num, BYNUM_MIN_LEN, max_len, samples=samples)
    sen.check_pattern_set(pt, pats, info, a, allow_equal=samples is None and not (a < 0).any())
    print_bynum(tag, info, t0)
    return pats, info


@pytest.mark.parametrize("panel,num", BYNUM_CASES)
def test_find_patterns_by_num(oracle_mod, panel, num):
    """M0 from the genotypes and M1 from the samples of E1."""
    a = bynum_panel(panel)
    o = bynum_oracle(oracle_mod, a, num)
    o.find_patterns()
    _, i0 = check_bynum(f"{panel} {num} M0:", o.patterns(), a, num)
    o.resolve_all()
    al, w, _ = o.samples()
    o.find_patterns()
    _, i1 = check_bynum(f"{panel} {num} M1:", o.patterns(), a, num, samples=(al, w))
    if (panel, num) == ("miss", 25):
        assert i0["rounds"] == i1["rounds"] == 11 and i0["cut_gap"] is None and i1["cut_gap"] is None
    if (panel, num) == ("miss", 60):
        assert (i0["rounds"], i1["rounds"]) == (23, 24) and i0["cut_gap"] is not None and i1["cut_gap"] is not None


@pytest.mark.parametrize("mode", ["reference", "device"])
def test_exact_mstep_after_find_patterns_by_num(oracle_mod, mode):
    """estimatePatterns after findPatternByNum filters by the search's last
    threshold (m_min_freq is a member: PatternManager.cpp:55-60, :400)."""
    panel, num = "miss", 60
    a = bynum_panel(panel, quirk=False)
    o = bynum_oracle(oracle_mod, a, num)
    o.set_exact_order(mode)
    o.find_patterns()
    prev = o.patterns()
    _, info = check_bynum(f"{panel} {num} (locus 0 complete) M0:", prev, a, num)
    assert info["rounds"] > 2 and info["last_threshold"] < 0.5
    o.resolve_all()
    o.estimate_patterns()
    new = o.patterns()
    check_exact_step(f"{panel} {num} {mode} after ByNum:", new, a, prev, 1,
                     (Fraction(info["last_threshold"]), BYNUM_MIN_LEN, BYNUM_MAX_LEN), mode == "device")
    check_estep_after(f"{panel} {num} {mode} after ByNum:", oracle_view(o, o.resolve_all()), a, new, 1, BYNUM_S)


@pytest.mark.parametrize("mode", ["reference", "device"])
def test_exact_mstep_after_exhausted_search(oracle_mod, mode):
    """A search that runs out of candidates before it has max_num patterns
    goes on lowering m_min_freq to 1e-38 (PatternManager.cpp:58-62: the loop
    tests only the size and the threshold), and the exact M-step after it
    filters by that: every candidate of positive frequency stays.  The hand
    panel of the self-tests: all eight single alleles in round 1, nothing
    reserved."""
    a, _ = hand_panel()
    o = oracle_mod.Oracle(a, "S" * a.shape[2], min_len=1, max_len=30, sample_size=2)
    o.set_num_patterns(10)
    o.set_exact_order(mode)
    o.find_patterns()
    prev = o.patterns()
    _, info = check_bynum("hand 10 M0:", prev, a, 10, max_len=30)
    assert info["patterns"] == 8 and info["last_threshold"] <= 1e-38
    o.resolve_all()
    o.estimate_patterns()
    new = o.patterns()
    minfo = check_exact_step(f"hand 10 {mode} after an exhausted search:", new, a, prev, 1,
                             (Fraction(info["last_threshold"]), 1, 30), mode == "device")
    # every string some haplotype has, and the single alleles: more than any threshold of a search
    # that stopped at the eight would keep
    assert minfo["kept"] == 8 + sum(len({h[s:s + n] for h in map(tuple, a[:, 0])}) for s in range(4)
                                    for n in range(2, 5 - s))


# ------------------------------------------------------- negative controls ----
def test_negative_controls(oracle_mod):
    """check_pattern_set is not vacuous: one kept pattern removed, one filtered
    candidate added back, or two neighbours swapped in the implementation's
    table, and it raises."""
    name = "a3"
    a = build_panel(name, quirk=False)
    hl = head_len(name)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][-1], a)
    o.find_patterns()
    prev = o.patterns()
    o.resolve_all()
    o.estimate_patterns()
    new = o.patterns()
    params = mining_params(name, a.shape[0])
    kept, info = sen.estimate_patterns_set(a, prev, hl, *params)
    sen.check_pattern_set(new, kept, info, a)
    ta, L = en.allele_table(a), a.shape[2]

    def rows(order, extra=None):
        out = {k: np.ascontiguousarray(v[order]) for k, v in new.items()}
        if extra is not None:
            s, al = extra
            out["start"] = np.append(out["start"], s).astype(np.int32)
            out["len"] = np.append(out["len"], len(al)).astype(np.int32)
            row = np.zeros((1, out["alleles"].shape[1]), np.int32)
            row[0, :len(al)] = al
            out["alleles"] = np.vstack([out["alleles"], row])
            for k in ("freq", "prefix", "tp"):
                out[k] = np.append(out[k], 0.01)
        succ = en.rebuild_successors(out, ta, L)  # so that only the set or the order is at fault
        out["succ"] = np.pad(succ, ((0, 0), (0, new["succ"].shape[1] - succ.shape[1])), constant_values=-1)
        return out

    n = len(kept)
    ids = list(range(n))
    sen.check_pattern_set(rows(ids), kept, info, a)
    longest = max(range(n), key=lambda i: len(kept[i][1]))  # no other pattern's successor: only the set changes
    with pytest.raises(AssertionError):
        sen.check_pattern_set(rows([i for i in ids if i != longest]), kept, info, a)
    # a candidate the final filter dropped: an extension, by a symbol of the locus, that is not kept
    dropped = next((s, al + (sym,)) for s, al in kept if s + len(al) < L for sym, _ in ta[s + len(al)]
                   if (s, al + (sym,)) not in set(kept))
    with pytest.raises(AssertionError):
        sen.check_pattern_set(rows(ids, extra=dropped), kept, info, a)
    swapped = ids[:]
    swapped[n // 2], swapped[n // 2 + 1] = swapped[n // 2 + 1], swapped[n // 2]
    with pytest.raises(AssertionError):
        sen.check_pattern_set(rows(swapped), kept, info, a)
    # the conditions are part of the check: a candidate on the threshold, or within 1e-9 of it
    with pytest.raises(AssertionError):
        sen.check_pattern_set(new, kept, dict(info, equal=1), a)
    with pytest.raises(AssertionError):
        sen.check_pattern_set(new, kept, dict(info, margin=5e-10), a)
    # the sorted ByNum tail: runs of equal frequency are sets, anything else is order
    b = bynum_panel("miss")
    ob = bynum_oracle(oracle_mod, b, 60)
    ob.find_patterns()
    pt = ob.patterns()
    pats, binfo = sen.find_patterns_by_num(b, 60, BYNUM_MIN_LEN, BYNUM_MAX_LEN)
    sen.check_pattern_set(pt, pats, binfo, b)
    tail = binfo["sorted_from"]
    i = next(i for i in range(tail, len(pats) - 1) if pats[i][1] != pats[i + 1][1])
    order = list(range(len(pats)))
    order[i], order[i + 1] = order[i + 1], order[i]
    bad = {k: np.ascontiguousarray(v[order]) for k, v in pt.items()}
    bad["succ"] = np.pad(en.rebuild_successors(bad, en.allele_table(b), b.shape[2]),
                         ((0, 0), (0, 0)), constant_values=-1)
    with pytest.raises(AssertionError):
        sen.check_pattern_set(bad, pats, binfo, b)
    with pytest.raises(AssertionError):
        sen.check_pattern_set(pt, pats, dict(binfo, cut_gap=5e-10), b)
