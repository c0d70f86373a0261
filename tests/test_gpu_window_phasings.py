"""hmc_window_phasings (exact_query.hip exact_window_phasings) on the GPU: the
ranked haplotype pairs of a locus window with the flanks summed — against
exhaustive enumeration (tests/window_enumeration.py), byte for byte against
hmc_haplotype_dosages fed the two-sided pattern each row spells, against the
pair and ranked calls within bounds, against itself across k, window order,
the other individuals, the cap, the LDS tier, store groups and a shard, and in
its statuses and errors.

Bound of a row against enumeration.  A row's prob is, operation for operation,
hmc_haplotype_dosages' value for the two-sided pattern the row spells (halved
exactly when the two strings are equal), so the bound is that test's:
gamma(dosage_k(L, M)) = gamma(6L + 4M + 15) relative, M the enumerator's count
of ordered phasings of the individual (test_gpu_haplotype_dosages' docstring
derives it; asserted <= 1e-12 on these panels).  Two rows are held to the
enumeration's order only where their exact posteriors differ by more than the
two bounds together.
"""
import os
import subprocess
from fractions import Fraction

import ctypes as C
import numpy as np
import pytest

import hmc_amd
from hmc_amd import synth
from hmc_amd._lib import HMCError, lib

import enumeration as en
import pair_enumeration as pe
import window_enumeration as wn
from test_enumeration_oracle import build_panel, head_len, perturbed_tables
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_gpu_haplotype_dosages import dosage_k
from test_gpu_posterior_draws import draw_k
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, MIXED_L, large_model, mixed_panel, mosaic_with_heads, rowsum_k
from test_gpu_switch_posteriors import switch_k

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
PANEL_CASES = [("snp", 2), ("a3", 3), ("a4", 6), ("short", 5), ("mc", 4), ("minlen2", 10)]
KS = (1, 4, 1024)
CAP = 1024
FIELDS = ("hap", "prob", "count", "n_config", "status")
SPILL_TIER = 1  # every record of two or more states goes through the device-memory scratch
_cache = {}


class ValueMismatch(AssertionError):
    """A row's prob is outside its bound of the enumerated value."""


def ask(m, wins, k, indiv=None):
    return m.window_phasings([s for s, _ in wins], [n for _, n in wins], k, indiv)


def same(x, y, fields=FIELDS):
    for f in fields:
        assert np.ascontiguousarray(x[f]).tobytes() == np.ascontiguousarray(y[f]).tobytes(), f


def row_key(out, i, w, r, n):
    return tuple(int(v) for v in out["hap"][i, w, r, 0, :n]), tuple(int(v) for v in out["hap"][i, w, r, 1, :n])


def tiny(name, S):
    if name not in _cache:
        a = build_panel(name)
        m = gpu_model(name, S, a)
        m.find_patterns()
        assert m.head_len() == head_len(name)
        pt = m.patterns()
        m.resolve_all()
        _cache[name] = (a, m, pt)
    return _cache[name]


def check_shapes_and_fallback(out, a, wins, k, i, w):
    """Rows past the count: the input genotype over the window at prob 0; -1 past the window's length."""
    s, n = wins[w]
    cnt = int(out["count"][i, w])
    assert (out["hap"][i, w, :, :, n:] == -1).all()
    for r in range(cnt, min(k, cnt + 3)):
        assert (out["hap"][i, w, r, :, :n] == a[i, :, s:s + n]).all() and out["prob"][i, w, r] == 0
    if cnt < k:
        assert not out["prob"][i, w, cnt:].any() and (out["hap"][i, w, cnt:, :, :n] == a[i, :, s:s + n]).all()


def check_windows(m, a, pt, hl, ks=KS):
    """Every window of windows_of(L), every individual, every k against enumeration; returns statistics."""
    N, _, L = a.shape
    ta = en.allele_table(a)
    wins = wn.windows_of(L)
    exact = wn.window_exact(a, pt, hl, wins)
    quirk = en.head_quirk(a, hl)
    worst, loosest, rows, over, equal, order_checked = 0.0, Fraction(0), 0, 0, 0, 0
    for k in ks:
        out = ask(m, wins, k)
        maxlen = max(n for _, n in wins)
        assert out["hap"].shape == (N, len(wins), k, 2, maxlen) and out["prob"].shape == (N, len(wins), k)
        for i in range(N):
            g = en.gamma(dosage_k(L, en.phasing_count(a[i], ta)))
            assert g <= 1e-12
            loosest = max(loosest, g)
            for w, (s, n) in enumerate(wins):
                C_ = wn.config_count(a[i], ta, s, n)
                st, cnt = int(out["status"][i, w]), int(out["count"][i, w])
                check_shapes_and_fallback(out, a, wins, k, i, w)
                if C_ > CAP:  # over the cap: status 4 and the fallback rows
                    assert st == 4 and cnt == 0 and out["n_config"][i, w] == 0, (i, s, n, C_)
                    over += k == ks[0]
                    continue
                assert st == 0 and cnt == min(k, int(out["n_config"][i, w])), (i, s, n)
                keys = [row_key(out, i, w, r, n) for r in range(cnt)]
                assert len(set(keys)) == cnt and all(x <= y for x, y in keys), (i, s, n, "a pair listed twice or unordered")
                allowed = wn.restrictions(a[i], ta, s, n)
                if quirk[i]:  # the head pairing is no phasing model: consistency (above head_len) and distinctness only
                    if s >= hl:
                        assert set(keys) <= allowed, (i, s, n)
                    continue
                assert set(keys) <= allowed, (i, s, n)
                e = exact[i][s, n]
                post = dict(e)
                assert int(out["n_config"][i, w]) == wn.positive(e), (i, s, n)
                for r, key in enumerate(keys):
                    p = float(out["prob"][i, w, r])
                    assert p > 0
                    if not en.within(p, post[key], g):
                        raise ValueMismatch((i, (s, n), key, en.relerr(p, post[key])))
                    worst = max(worst, en.relerr(p, post[key]))
                    equal += key[0] == key[1]
                    if r:
                        assert p <= float(out["prob"][i, w, r - 1]), (i, s, n, r)
                    # the enumeration's order wherever its gaps exceed the bound
                    if r < len(e) and e[r][0] != key:
                        assert abs(e[r][1] - post[key]) <= 2 * g * e[r][1] / (1 - g), (i, s, n, r, key, e[r])
                    elif r < len(e):
                        order_checked += 1
                rows += cnt
    return dict(windows=len(wins), rows=rows, over_cap=over, equal_haplotype_rows=equal, rows_in_exact_order=order_checked,
                prob_bound=float(loosest), worst_u=worst / float(en.U), stats=m.window_stats())


@pytest.mark.parametrize("name,S", PANEL_CASES)
def test_against_enumeration(name, S):
    a, m, pt = tiny(name, S)
    m.set_window_tuning(0, 0)
    res = check_windows(m, a, pt, head_len(name))
    print(name, S, res)
    assert res["rows"] > 0 and res["equal_haplotype_rows"] > 0 and res["stats"]["sweep_ms"] > 0


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the value comparison raises."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    bad_tp, _ = perturbed_tables(a, pt, gpu_view(m), 1)
    m2 = gpu_model(name, S, a)
    feed(m2, bad_tp)
    m2.resolve_all()
    with pytest.raises(ValueMismatch) as ei:
        check_windows(m2, a, pt, 1, ks=(4,))
    print("first value outside its bound:", ei.value.args[0])
    assert 0 < ei.value.args[0][3] < 1e-8  # the size of the perturbation, not a wrong table


# ------------------------------------------------ byte for byte against the dosages ----
def rows_against_dosages(m, a, wins, k, who):
    """Every returned row of the individuals `who` against hmc_haplotype_dosages fed the two-sided pattern that
    spells it: the same double, halved for equal haplotypes.  Returns (rows compared, rows of equal haplotypes)."""
    out = ask(m, wins, k, who)
    rows = equal = 0
    for q, i in enumerate(who):
        pats = []
        for w, (s, n) in enumerate(wins):
            if out["status"][q, w] != 0:
                continue
            for r in range(int(out["count"][q, w])):
                x, y = row_key(out, q, w, r, n)
                pats.append((w, r, s, x, y))
        if not pats:
            continue
        d = m.haplotype_dosages([p[2] for p in pats], [p[3] for p in pats], [p[4] for p in pats], [i])
        assert d["status"][0] == 0
        for c, (w, r, s, x, y) in enumerate(pats):
            want = d["dosage"][0, c] * (0.5 if x == y else 1.0)
            assert out["prob"][q, w, r].tobytes() == np.float64(want).tobytes(), (i, wins[w], r, out["prob"][q, w, r], want)
            rows += 1
            equal += x == y
    return rows, equal


def both_ranges(m, fn):
    for ext in (False, True):
        m.set_posterior_range(ext)
        try:
            fn(ext)
        finally:
            m.set_posterior_range(False)


@pytest.mark.parametrize("name,S", PANEL_CASES)
def test_rows_are_the_dosages_doubles(name, S):
    a, m, _ = tiny(name, S)
    N, _, L = a.shape
    wins = wn.windows_of(L)

    def check(ext):
        rows, equal = rows_against_dosages(m, a, wins, 8, list(range(N)))
        print(name, "extended" if ext else "regular", rows, "rows,", equal, "of equal haplotypes")
        assert rows > 100 and equal > 0

    both_ranges(m, check)


def mosaic():
    if "mosaic" not in _cache:
        N, L = BITS_SHAPE
        a = mosaic_with_heads(N, L, 3, 0.05, 7)
        _cache["mosaic"] = (a, large_model(a))
    return _cache["mosaic"]


def mosaic_windows(L):
    """Lengths 1, 3, 8 and 16 over the panel, overlapping, one repeated, out of order."""
    wins = [(s, n) for n in (16, 1, 8, 3) for s in range(0, L - n + 1, 29)]
    return wins + [wins[2], (L - 5, 5), (0, 12)]


def test_mosaic_rows_are_the_dosages_doubles():
    a, m = mosaic()
    N, L = BITS_SHAPE
    wins = mosaic_windows(L)
    who = list(range(0, N, 7))
    assert int(m.frontier_max().max()) > 256

    def check(ext):
        rows, equal = rows_against_dosages(m, a, wins, 4, who)
        print("mosaic", "extended" if ext else "regular", rows, "rows,", equal, "of equal haplotypes")
        assert rows > 300 and equal > 0

    both_ranges(m, check)


# ----------------------------------------------------------- cross-checks within bounds ----
@pytest.mark.parametrize("name,S", [("snp", 2), ("a3", 3)])
def test_against_pair_and_ranked_calls(name, S):
    a, m, pt = tiny(name, S)
    N, _, L = a.shape
    ta = en.allele_table(a)
    hl = head_len(name)
    quirk = en.head_quirk(a, hl)
    # windows whose only branching loci are two heterozygous ones: cis and trans of pair_posteriors
    n_pairs = 0
    for i in range(N):
        if quirk[i]:
            continue
        het = pe.het_loci(a[i])
        g = en.gamma(dosage_k(L, en.phasing_count(a[i], ta))) + en.gamma(switch_k(L, en.phasing_count(a[i], ta)))
        for x, y in zip(het, het[1:]):
            if (a[i, :, x:y + 1] < 0).any():
                continue
            out = ask(m, [(x, y - x + 1)], 4, [i])
            pr = m.pair_posteriors([i], [x], [y])
            assert out["count"][0, 0] == out["n_config"][0, 0] == 2 and out["status"][0, 0] == 0 and pr["status"][0] == 0
            for r in range(2):
                h0, h1 = row_key(out, 0, 0, r, y - x + 1)
                cis = (h0[0] < h1[0]) == (h0[-1] < h1[-1])
                want = Fraction(float(pr["post"][0, 0 if cis else 1]))
                assert abs(Fraction(float(out["prob"][0, 0, r])) - want) <= g * want / (1 - g), (i, x, y, r)
            n_pairs += 1
    assert n_pairs >= 10
    # the whole panel as one window: ranked_phasings' rows
    full = ask(m, [(0, L)], 1024)
    rk = m.ranked_phasings(16)
    n_rows = 0
    for i in range(N):
        if quirk[i] or full["status"][i, 0] != 0:
            continue
        M = en.phasing_count(a[i], ta)
        g = en.gamma(dosage_k(L, M)) + en.gamma(draw_k(L, M))
        got = {row_key(full, i, 0, r, L): float(full["prob"][i, 0, r]) for r in range(int(full["count"][i, 0]))}
        assert int(full["n_config"][i, 0]) == len(got)
        assert min(16, len(got)) == int(rk["count"][i])
        for r in range(int(rk["count"][i])):
            key = tuple(int(v) for v in rk["hap"][i, r, 0]), tuple(int(v) for v in rk["hap"][i, r, 1])
            key = key if key[0] <= key[1] else (key[1], key[0])
            want = Fraction(float(rk["prob"][i, r]))
            assert key in got and abs(Fraction(got[key]) - want) <= g * want / (1 - g), (i, r)
            n_rows += 1
        # all rows: their probs sum to 1 within the bound
        tot = sum((Fraction(p) for p in got.values()), Fraction(0))
        assert abs(tot - 1) <= en.gamma(dosage_k(L, M)) / (1 - en.gamma(dosage_k(L, M))), (i, float(tot))
    assert n_rows >= 50


# --------------------------------------------------------------- what the bits depend on ----
def test_bits_independent_of_path():
    """k, window order and duplicates, the other individuals, the cap, the tier,
    store groups and a shard do not change a bit."""
    a, m = mosaic()
    N, L = BITS_SHAPE
    wins = mosaic_windows(L)
    m.set_window_tuning(0, 0)
    ref = ask(m, wins, 8)
    s0 = m.window_stats()
    print(s0)
    assert s0["groups"] == 1 and s0["sweep_ms"] > 0 and s0["configs_built"] >= 64 and s0["n_spilled"] > 0
    assert (ref["status"] == 0).sum() > ref["status"].size // 2 and (ref["count"] > 1).sum() > 100
    # a repeated window repeats its rows
    for f in FIELDS:
        assert np.ascontiguousarray(ref[f][:, 2]).tobytes() == np.ascontiguousarray(ref[f][:, len(wins) - 3]).tobytes(), f
    # k: row prefixes
    for k in (1, 3, 64):
        got = ask(m, wins, k)
        c = min(k, 8)
        assert got["status"].tobytes() == ref["status"].tobytes() and got["n_config"].tobytes() == ref["n_config"].tobytes()
        assert np.ascontiguousarray(got["prob"][:, :, :c]).tobytes() == np.ascontiguousarray(ref["prob"][:, :, :c]).tobytes()
        assert np.ascontiguousarray(got["hap"][:, :, :c]).tobytes() == np.ascontiguousarray(ref["hap"][:, :, :c]).tobytes()
        assert (got["count"] == np.minimum(ref["n_config"], k)).all()
    # window order, duplicates, a window alone
    rng = np.random.default_rng(len(wins))
    pick = np.concatenate([rng.permutation(len(wins)), rng.integers(0, len(wins), 5)])
    got = ask(m, [wins[w] for w in pick], 8)
    maxlen = max(n for _, n in wins)
    for f in FIELDS:
        assert got[f].tobytes() == np.ascontiguousarray(ref[f][:, pick]).tobytes(), f
    for w in (0, len(wins) // 2, len(wins) - 1):
        one = ask(m, [wins[w]], 8)
        n = wins[w][1]
        assert one["prob"].tobytes() == np.ascontiguousarray(ref["prob"][:, [w]]).tobytes()
        assert one["hap"].tobytes() == np.ascontiguousarray(ref["hap"][:, [w], :, :, :n]).tobytes()
        assert one["count"].tobytes() == np.ascontiguousarray(ref["count"][:, [w]]).tobytes()
    # individuals as a subset, permuted, with a repeat
    who = [N - 1, 3, 17, 3, 0]
    sub = ask(m, wins, 8, who)
    for f in FIELDS:
        assert sub[f].tobytes() == np.ascontiguousarray(ref[f][who]).tobytes(), f
    # a cap that still holds every C that ran; the tier that forces the device-memory scratch
    ta = en.allele_table(a)
    cs = np.array([[wn.config_count(a[i], ta, s, n) for s, n in wins] for i in range(N)])
    assert ((cs > CAP) == (ref["status"] == 4)).all()
    held = int(cs[cs <= CAP].max())
    m.set_window_tuning(held, 0)
    same(ask(m, wins, 8), ref)
    m.set_window_tuning(0, SPILL_TIER)
    same(ask(m, wins, 8), ref)
    assert m.window_stats()["n_spilled"] == N
    m.set_window_tuning(0, 0)
    # a lowered cap: status 4 exactly where C exceeds it, the other rows unchanged
    m.set_window_tuning(16, 0)
    low = ask(m, wins, 8)
    m.set_window_tuning(0, 0)
    assert ((cs > 16) == (low["status"] == 4)).all() and (low["status"] == 4).any() and (low["status"] == 0).any()
    assert m.window_stats()["n_over_cap"] == int((cs > 16).sum()) and m.window_stats()["configs_built"] == 16
    keep = low["status"] == 0
    for f in FIELDS:
        assert np.ascontiguousarray(low[f][keep]).tobytes() == np.ascontiguousarray(ref[f][keep]).tobytes(), f
    assert not low["count"][~keep].any() and not low["prob"][~keep].any()
    for i, w in zip(*np.nonzero(low["status"] == 4)):
        s, n = wins[w]
        assert (low["hap"][i, w, :, :, :n] == a[i, :, s:s + n]).all()
    # store groups, a shard
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = ask(m2, wins, 8)
    print(m2.window_stats())
    assert m2.window_stats()["groups"] >= 2
    same(got, ref)
    m3 = large_model(a, shard=(20, 40))
    part = ask(m3, wins, 8)
    for f in FIELDS:
        assert part[f].tobytes() == np.ascontiguousarray(ref[f][20:40]).tobytes(), f
    for bad in (0, N - 1):  # outside the shard
        with pytest.raises(HMCError) as ei:
            ask(m3, wins, 8, [25, bad])
        assert ei.value.code == -1 and "shard" in str(ei.value) and "entry 1" in str(ei.value), str(ei.value)


def test_tiers_and_caps_on_the_tiny_panels():
    """The scratch path and a lowered cap on an enumerable panel: the default's bytes, status 4 aside."""
    a, m, _ = tiny("a3", 3)
    N, _, L = a.shape
    ta = en.allele_table(a)
    wins = wn.windows_of(L)
    m.set_window_tuning(0, 0)
    ref = ask(m, wins, 1024)
    m.set_window_tuning(0, SPILL_TIER)
    same(ask(m, wins, 1024), ref)
    assert m.window_stats()["n_spilled"] > 0
    cs = np.array([[wn.config_count(a[i], ta, s, n) for s, n in wins] for i in range(N)])
    for cap in (1, 2, 5, 100):
        m.set_window_tuning(cap, 0)
        low = ask(m, wins, 1024)
        assert ((cs > min(cap, CAP)) == (low["status"] == 4)).all(), cap
        keep = low["status"] == 0
        for f in FIELDS:
            assert np.ascontiguousarray(low[f][keep]).tobytes() == np.ascontiguousarray(ref[f][keep]).tobytes(), (cap, f)
    m.set_window_tuning(0, 0)


# ------------------------------------------------------------------ statuses and errors ----
def test_statuses_on_the_mixed_panel():
    """Regular range: statuses 1 and 2 exactly where map_phase has them, the
    input genotype at prob 0; extended range: real rows everywhere."""
    b = mixed_panel(MIXED_L)
    m = large_model(b)
    N, _, L = b.shape
    wins = [(0, 6), (L // 2, 9), (L - 4, 4), (7, 1)]
    ta = en.allele_table(b)
    assert all(wn.config_count(b[i], ta, s, n) <= CAP for i in range(N) for s, n in wins)
    mp = m.map_phase()
    assert {0, 1, 2} <= set(mp["status"].tolist())
    reg = ask(m, wins, 4)
    assert (reg["status"] == mp["status"][:, None]).all()
    gone = reg["status"] != 0
    assert not reg["count"][gone].any() and not reg["n_config"][gone].any() and not reg["prob"][gone].any()
    for i, w in zip(*np.nonzero(gone)):
        s, n = wins[w]
        assert (reg["hap"][i, w, :, :, :n] == b[i, :, s:s + n]).all()
    m.set_posterior_range(True)
    ext = ask(m, wins, 4)
    m.set_posterior_range(False)
    assert not ext["status"].any() and (ext["count"] >= 1).all() and (ext["prob"][:, :, 0] > 0).all()
    # all rows of a window: within the large-panel bound of 1 (test_gpu_haplotype_dosages: every row carries at most
    # g = gamma(rowsum_k(L, F) + 1) relative, and so does their exact sum)
    g = en.gamma(rowsum_k(L, int(m.frontier_max().max())) + 1)
    assert g < 1e-6
    for i in range(N):
        for w in range(len(wins)):
            tot = sum(Fraction(float(p)) for p in ask_all_rows(m, wins[w], i))
            assert abs(tot - 1) <= 2 * g, (i, w, float(tot))
    same(ask(m, wins, 4), reg)  # the range set back: the regular bytes again


def ask_all_rows(m, win, i):
    m.set_posterior_range(True)
    try:
        out = ask(m, [win], 1024, [i])
    finally:
        m.set_posterior_range(False)
    assert out["count"][0, 0] == out["n_config"][0, 0]
    return out["prob"][0, 0, :int(out["count"][0, 0])]


def raw_call(m, n, indiv, W, start, ln, maxlen, k):
    i32 = lambda x: None if x is None else np.ascontiguousarray(x, np.int32)  # noqa: E731
    indiv, start, ln = i32(indiv), i32(start), i32(ln)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    prob = np.full((max(n, 1), max(W, 1), max(k, 1)), -7.0)
    st = np.full((max(n, 1), max(W, 1)), -7, np.int32)
    rc = lib().hmc_window_phasings(m._h, n, ptr(indiv), W, ptr(start), ptr(ln), maxlen, k, None,
                                   prob.ctypes.data_as(C.POINTER(C.c_double)), None, None, ptr(st))
    return rc, prob, st


def test_errors_and_call_order():
    a = build_panel("a3")
    N, _, L = a.shape
    m = gpu_model("a3", 3, a)
    wins = [(0, 3), (2, 1), (L - 2, 2)]
    m.find_patterns()
    with pytest.raises(HMCError) as ei:
        ask(m, wins, 4)
    assert ei.value.code == -1 and "E-step" in str(ei.value)  # HMC_EARG: no E-step yet
    m.resolve_all()
    ref = ask(m, wins, 4)
    assert not ref["status"].any()
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        ask(m, wins, 4)
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    before = (m.estep_results(), m.resolutions())
    ref = ask(m, wins, 4)
    assert not ref["status"].any() and ref["prob"].shape == (N, 3, 4)
    st = m.window_stats()
    assert st["groups"] >= 1 and st["sweep_ms"] > 0 and st["n_over_cap"] == 0 and st["configs_built"] in (4, 16, 64, 256, 1024)
    after = (m.estep_results(), m.resolutions())
    for x, y in zip(before, after):  # what the last E-step left is unchanged by the call
        if isinstance(x, dict):
            assert all(np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes() for f in x)
        else:
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    # outputs may be NULL
    rc, prob, st_ = raw_call(m, N, None, 3, [w[0] for w in wins], [w[1] for w in wins], 3, 4)
    assert rc == 0 and prob.tobytes() == ref["prob"].tobytes() and not st_.any()
    # n = 0 and n_windows = 0 succeed with no device work: zero stats, nothing written
    out = ask(m, wins, 4, [])
    assert out["prob"].shape == (0, 3, 4) and not any(m.window_stats().values())
    ask(m, wins, 4)
    out = ask(m, [], 4)
    assert out["prob"].shape == (N, 0, 4) and not any(m.window_stats().values())
    rc, prob, st_ = raw_call(m, 0, [0], 1, [0], [1], 1, 1)
    assert rc == 0 and (prob == -7).all() and (st_ == -7).all()
    rc, prob, st_ = raw_call(m, 2, [0, 1], 0, None, None, 1, 1)
    assert rc == 0 and (prob == -7).all()
    # HMC_EARG, naming the first offender
    for what, who in (("below the shard", [0, -1]), ("past the shard", [0, N])):
        with pytest.raises(HMCError) as ei:
            ask(m, wins, 4, who)
        assert ei.value.code == -1 and "entry 1" in str(ei.value), (what, str(ei.value))
    bad = {"negative start": (-1, 1), "empty": (0, 0), "past the last locus": (L - 1, 2), "start past the panel": (L, 1)}
    for what, w in bad.items():
        with pytest.raises(HMCError) as ei:
            ask(m, [wins[0], w, wins[1]], 4)
        assert ei.value.code == -1 and "window 1" in str(ei.value), (what, str(ei.value))
    rc, _, _ = raw_call(m, 1, [0], 2, [0, 0], [1, 3], 2, 1)  # len > maxlen
    assert rc == -1 and b"window 1" in lib().hmc_ctx_error(m._h)
    for k in (0, -1, 1025):
        with pytest.raises(HMCError) as ei:
            ask(m, wins, k)
        assert ei.value.code == -1 and "k = " in str(ei.value), k
    same(ask(m, wins, 4), ref)  # a refused call leaves nothing behind
    for cap, tier in ((-1, 0), (1025, 0), (0, -1), (0, 513)):
        with pytest.raises(HMCError) as ei:
            m.set_window_tuning(cap, tier)
        assert ei.value.code == -1, (cap, tier)
    m.set_window_tuning(1024, 512)
    same(ask(m, wins, 4), ref)
    m.set_window_tuning(0, 0)


def test_leaves_the_em_untouched():
    """find_patterns, resolve_all, [window_phasings], em_iteration: the same LL,
    pairs and next table with and without the call."""
    a = build_panel("a4")
    L = a.shape[2]

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.find_patterns()
        m.resolve_all()
        if call:
            assert ask(m, wn.windows_of(L), 8)["prob"].shape[0] == a.shape[0]
        log, old, go = m.em_iteration(1, -np.finfo(np.float64).max)
        log = {k: v for k, v in log.items() if not k.startswith("t_")}
        return log, old, go, m.resolutions(), m.patterns(), m.estep_results()

    def eq(x, y):
        if isinstance(x, dict):
            return x.keys() == y.keys() and all(eq(x[k], y[k]) for k in x)
        if isinstance(x, (tuple, list)):
            return len(x) == len(y) and all(eq(p, q) for p, q in zip(x, y))
        if isinstance(x, np.ndarray):
            return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        return x == y

    assert eq(chain(True), chain(False))


# ------------------------------------------------------------------------ CLI ----
def test_cli_output_windows(tmp_path):
    """hmc_resolve --output-windows FILE --windows WINFILE --window-k K on a3 as
    a PHASE file: one line per individual of status 0, window and rank, the
    numbers read back to the API's doubles; a malformed line fails with its
    number."""
    a = build_panel("a3")
    N, _, L = a.shape
    src, winf, dst = tmp_path / "a3.inp", tmp_path / "a3.windows", tmp_path / "a3.wp"
    synth.write_phase(synth.Panel(a, "S" * L), str(src))
    wins = [("geneA", 0, 3), ("one", 4, 1), ("tail", L - 4, 4), ("geneA2", 0, 3)]
    winf.write_text("# windows of the test\n\n" + "".join(f"{n}\t{s} {ln}\n" for n, s, ln in wins))
    r = subprocess.run([CLI, "--output-windows", str(dst), "--windows", str(winf), "--window-k", "3", str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    out = ask(m, [(s, ln) for _, s, ln in wins], 3)
    assert not out["status"].any()
    lines = dst.read_text().splitlines()
    assert lines[0] == "Id\tWindow\tStart\tLength\tRank\tPosterior\tHaplotype0\tHaplotype1"
    want = [(i, w, r) for i in range(N) for w in range(len(wins)) for r in range(int(out["count"][i, w]))]
    assert len(lines) - 1 == len(want) and len(want) > N * len(wins)
    for ln, (i, w, r) in zip(lines[1:], want):
        f = ln.split("\t")
        n = wins[w][2]
        assert len(f) == 8 and f[0].lstrip("#") == str(i + 1) and [int(v) for v in f[1:5]] == [w, wins[w][1], n, r]
        assert float(f[5]) == float(out["prob"][i, w, r])
        for side in range(2):
            assert f[6 + side].split(" ") == [chr(int(v)) for v in out["hap"][i, w, r, side, :n]]
    dst2 = tmp_path / "a3.wp2"
    m.write_window_phasings(str(dst2), [s for _, s, _ in wins], [ln for _, _, ln in wins], 3)
    assert dst2.read_text() == dst.read_text()
    for bad, lineno in (("x 0\n", 4), ("x 99 1\n", 4), ("x 0 0\n", 4), ("x zero 1\n", 4), (f"x {L - 1} 2\n", 4)):
        winf.write_text("# c\n\nok 0 1\n" + bad)
        dst.unlink(missing_ok=True)
        r = subprocess.run([CLI, "--output-windows", str(dst), "--windows", str(winf), str(src)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 1 and f"line {lineno}" in r.stderr, (bad, r.stderr)
        assert not dst.exists()
    for args in (["--output-windows", str(dst)], ["--windows", str(winf)], ["--window-k", "3"]):
        r = subprocess.run([CLI, *args, str(src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--output-windows" in r.stderr and "Usage" in r.stderr, r.stderr
