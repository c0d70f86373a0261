"""hmc_haplotype_dosages (exact_query.hip exact_haplotype_dosages) on the GPU: the
exact expected copies of caller-given haplotypes — against exhaustive
enumeration (tests/dosage_enumeration.py), against itself across every
schedule (slots per state NS, rounds, the LDS tier, pattern order, duplicates,
a pattern asked alone, individuals as a subset or permuted, store groups, a
shard) byte for byte, against the three pinned posterior calls on a large
panel, and in extended range.

Bound of one value against enumeration, u = 2^-53, every addend non-negative so
nothing cancels; L loci, M the enumerator's count of ordered phasings of the
individual (enumeration.phasing_count).  The sweep is the switch kernel's with
some terms replaced by exact zeros, so the count is switch_k's
(test_gpu_switch_posteriors, test_gpu_pair_posteriors) plus one:
  labelled forward value of a state  anchored as the record's forward
        likelihood or 0, then the same chain — per locus the state's product of
        two transition probabilities (one rounding) multiplied into the running
        value (one), and sums that merge at most M prefixes of phasings, a
        subset of the forward likelihood's own terms; a filtered label is an
        exact 0: over the whole panel at most 2L+2 multiplications and M
        additions: 2L+2+M;
  backward likelihood                2L+2+M;
  their product                      1 (the scaling by powers of two is exact);
  S_0 and S_1                        a lane adds at most ceil(F/64) <= M of its
        states' products, then 6 butterfly steps: M+6 each, on disjoint terms;
  S_0 + S_1                          1;
  P(genotype), the divisor           2L+2+M (check_estep's total);
  the division                       1.
Together 6L + 4M + 15 roundings: gamma(6L + 4M + 15) relative, at most
gamma(6*10 + 4*1960 + 15) = 8.8e-13 on these panels (asserted <= 1e-12).

On the large panel no enumeration exists; there a dosage x is compared with a
number y formed from a pinned call's doubles.  Both carry at most
g = gamma(rowsum_k(L, F) + 1) relative (test_gpu_posteriors.rowsum_k bounds a
sum of forward x backward products over P(genotype) with frontiers of at most F
states; the dosage adds S_0 + S_1; a sum of such non-negative values, formed
here in exact rationals, keeps the relative bound) and the absolute underflow
term t = (6 L F^2 + 2F) ETA / P(genotype) of check_rows_sum_to_one, so
|x - y| <= g (x + y) / (1 - g) + 2 t.  The draws' prob is a product of at most
L transition products over P(genotype): fewer roundings than rowsum_k, so the
same g covers it.
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

import dosage_enumeration as dn
import enumeration as en
from test_dosage_enumeration import MIN_MIXED, MIN_MIXED_INDIVIDUALS
from test_enumeration_oracle import PANELS, build_panel, head_len, perturbed_tables
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, ETA, MIXED_L, mixed_panel, mosaic_with_heads, rowsum_k
from test_gpu_switch_posteriors import switch_k
from test_scaled_tables import SUBNORMAL_C, scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
SLOTS = (1, 2, 4, 8)  # every instantiated NS
SPILL_TIER = 1        # every record of two or more states goes through the device-memory scratch
PANEL_CASES = [("snp", 2), ("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5), ("minlen2", 10)]


class ValueMismatch(AssertionError):
    """A dosage is outside its bound of the enumerated value."""


def dosage_k(L, M):
    return switch_k(L, M) + 1


def ask(m, pats, indiv=None):
    """patterns (start, A, B or None) -> the call's dict"""
    two = any(B is not None for _, _, B in pats)
    rows_b = [B if B is not None else (dn.ANY,) * len(A) for _, A, B in pats] if two else None
    return m.haplotype_dosages([s for s, _, _ in pats], [A for _, A, _ in pats], rows_b, indiv)


def same_bytes(x, y):
    return x["status"].tobytes() == y["status"].tobytes() and x["dosage"].tobytes() == y["dosage"].tobytes()


def check_dosages(m, a, pt, hl, non_vacuous=True):
    """panel_patterns of the panel against enumeration; returns the largest
    observed error in units of u and the loosest bound."""
    N, _, L = a.shape
    pats = dn.panel_patterns(a, pt, hl)
    m.set_dosage_tuning(0, 0)
    out = ask(m, pats)
    stats = m.dosage_stats()
    assert out["dosage"].shape == (N, len(pats)) and not out["status"].any()
    assert stats["slots"] == 4 and stats["rounds"] > 1 and stats["n_spilled"] == 0  # far more than 4 windows overlap
    ta = en.allele_table(a)
    quirk = en.head_quirk(a, hl)
    assert quirk.sum() <= 1 and quirk.sum() <= N / 4
    exact = dn.dosages_exact(a, pt, hl, pats)
    if non_vacuous:
        mixed, who = dn.mixed_values(exact)
        assert mixed >= MIN_MIXED and who >= MIN_MIXED_INDIVIDUALS, (mixed, who)
    worst, loosest, zeros = 0.0, Fraction(0), 0
    for i in range(N):
        g = en.gamma(dosage_k(L, en.phasing_count(a[i], ta)))
        assert g <= 1e-12
        loosest = max(loosest, g)
        row = out["dosage"][i]
        if quirk[i]:  # the head pairing is no phasing model: the range only
            assert ((row >= 0) & (row <= 2 + float(2 * g))).all(), i
            continue
        for p, e in enumerate(exact[i]):
            if e == 0:
                assert row[p] == 0.0, (i, pats[p], row[p])
                zeros += 1
                continue
            if not en.within(row[p], e, g):
                raise ValueMismatch((i, pats[p], en.relerr(row[p], e)))
            worst = max(worst, en.relerr(row[p], e))
    return dict(patterns=len(pats), exact_zeros=zeros, worst_u=worst / float(en.U), loosest_bound=float(loosest), stats=stats)


@pytest.mark.parametrize("name,S", PANEL_CASES)
def test_against_enumeration(name, S):
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    res = check_dosages(m, a, pt, hl)
    print(name, S, res)
    assert res["exact_zeros"] > 0
    # the same patterns at one slot, spilled: the bytes of the automatic schedule
    pats = dn.panel_patterns(a, pt, hl)
    ref = ask(m, pats)
    m.set_dosage_tuning(1, SPILL_TIER)
    assert same_bytes(ask(m, pats), ref)
    assert m.dosage_stats()["n_spilled"] > 0 and m.dosage_stats()["slots"] == 1
    m.set_dosage_tuning(0, 0)


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the value comparison raises."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    view = gpu_view(m)
    check_dosages(m, a, pt, 1)
    bad_tp, _ = perturbed_tables(a, pt, view, 1)
    m2 = gpu_model(name, S, a)
    feed(m2, bad_tp)
    m2.resolve_all()
    with pytest.raises(ValueMismatch) as ei:
        check_dosages(m2, a, pt, 1)
    i, pat, err = ei.value.args[0]
    print("first value outside its bound: individual", i, "pattern", pat, "relative error", err)
    assert 0 < err < 1e-8  # the size of the perturbation, not a wrong table


# ------------------------------------------------------------ the large panel ----
_large = {}


def large_panel():
    if "a" not in _large:
        N, L = BITS_SHAPE
        _large["a"] = mosaic_with_heads(N, L, 3, 0.05, 7)
    return _large["a"]


def large_model(a, budgets=None, shard=None):
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * a.shape[2]))
    if budgets:
        m.set_store_budgets(*budgets)
    m.find_patterns()
    if shard:
        m.set_shard(*shard)
    m.resolve_all()
    return m


def reference_model():
    if "m" not in _large:
        _large["m"] = large_model(large_panel())
    return _large["m"]


def bits_patterns(a):
    """Lengths 1, 5, 40 and L, overlapping heavily: windows of the first
    individuals' genotype rows (row 0 where typed, else any), some two-sided."""
    N, _, L = a.shape
    pats = []
    for i, s in enumerate(range(0, L, 3)):
        g = a[i % N]
        for n in (1, 5, 40):
            if s + n > L:
                continue
            A = tuple(int(x) if x >= 0 else dn.ANY for x in g[0, s:s + n])
            B = tuple(int(x) if x >= 0 else dn.ANY for x in g[1, s:s + n])
            pats.append((s, A, B if (i + n) % 2 else None))
    for i in (0, 1, 2):
        pats.append((0, tuple(int(x) if x >= 0 else dn.ANY for x in a[i, 0]), None))
    pats.append((0, (dn.ANY,) * L, None))
    pats.append((3, (dn.ABSENT,) * 5, None))
    return pats


def test_bits_independent_of_path():
    """Slots, rounds, the tier, the other patterns and their order, the other
    individuals, store groups and a shard do not change a bit."""
    a = large_panel()
    N, L = BITS_SHAPE
    pats = bits_patterns(a)
    assert {len(A) for _, A, _ in pats} == {1, 5, 40, L}
    m = reference_model()
    assert int(m.frontier_max().max()) > 254  # past the default LDS tier
    m.set_dosage_tuning(0, 0)
    ref = ask(m, pats)
    s0 = m.dosage_stats()
    print(s0)
    assert s0["groups"] == 1 and s0["slots"] == 4 and s0["rounds"] > 1 and 0 < s0["n_spilled"] < N and not ref["status"].any()
    assert (ref["dosage"] >= 0).all() and (ref["dosage"] <= 2 + 1e-9).all()
    assert (ref["dosage"][:, -1] == 0.0).all() and np.abs(ref["dosage"][:, -2] - 2).max() < 1e-9
    assert ((ref["dosage"] > 0.05) & (ref["dosage"] < 0.95)).sum() > 100
    for ns in SLOTS:
        m.set_dosage_tuning(ns, 0)
        assert same_bytes(ask(m, pats), ref), ns
        st = m.dosage_stats()
        print(st)
        assert st["slots"] == ns and st["n_spilled"] == s0["n_spilled"]
        if ns == 1:
            assert st["rounds"] > 1  # overlapping windows took later rounds
    m.set_dosage_tuning(0, SPILL_TIER)
    assert same_bytes(ask(m, pats), ref)
    assert m.dosage_stats()["n_spilled"] == N
    m.set_dosage_tuning(0, 0)
    # shuffled, with duplicates: columns follow the caller's order
    rng = np.random.default_rng(len(pats))
    pick = np.concatenate([rng.permutation(len(pats)), rng.integers(0, len(pats), len(pats) // 4)])
    got = ask(m, [pats[k] for k in pick])
    assert got["dosage"].tobytes() == np.ascontiguousarray(ref["dosage"][:, pick]).tobytes()
    # a single pattern per call
    for k in sorted({0, len(pats) // 2, len(pats) - 4, len(pats) - 1, int(rng.integers(0, len(pats)))}):
        one = ask(m, [pats[k]])
        assert one["dosage"].tobytes() == np.ascontiguousarray(ref["dosage"][:, [k]]).tobytes(), pats[k]
        assert m.dosage_stats()["rounds"] == 1 and m.dosage_stats()["slots"] == 1
    # individuals as a subset, permuted, with a repeat
    who = [N - 1, 3, 17, 3, 0]
    sub = ask(m, pats, who)
    assert sub["dosage"].tobytes() == np.ascontiguousarray(ref["dosage"][who]).tobytes() and not sub["status"].any()
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = ask(m2, pats)
    print(m2.dosage_stats())
    assert m2.dosage_stats()["groups"] >= 2
    assert same_bytes(got, ref)
    m3 = large_model(a, shard=(20, 40))
    part = ask(m3, pats)
    assert part["dosage"].tobytes() == np.ascontiguousarray(ref["dosage"][20:40]).tobytes() and not part["status"].any()
    for bad in (0, N - 1):  # outside the shard
        with pytest.raises(HMCError) as ei:
            ask(m3, pats, [25, bad])
        assert ei.value.code == -1 and "shard" in str(ei.value) and "entry 1" in str(ei.value), str(ei.value)


def close_large(x, y, g, t):
    """|x - y| within the sum of the two calls' bounds (module docstring); y may be a Fraction."""
    x, y = Fraction(float(x)), Fraction(y) if isinstance(y, Fraction) else Fraction(float(y))
    return abs(x - y) <= g * (x + y) / (1 - g) + 2 * t


def test_consistent_with_the_pinned_calls():
    a = large_panel()
    N, L = BITS_SHAPE
    m = reference_model()
    m.set_dosage_tuning(0, 0)
    F = int(m.frontier_max().max())
    g = en.gamma(rowsum_k(L, F) + 1)
    assert g < 1e-9
    total = m.estep_results()["total"]
    t = [(6 * L * F * F + 2 * F) * ETA / Fraction(float(x)) for x in total]
    assert max(t) < 1e-200
    num, sym, _ = m.allele_table()
    # one-sided, one locus, at each missing site: the allele counts weighted by the genotype posteriors' bins
    gp = m.genotype_posteriors()
    assert len(gp["indiv"]) > 300 and not gp["status"].any()
    loci = sorted(set(gp["locus"].tolist()))
    pats = [(k, (int(sym[k, j]),), None) for k in loci for j in range(num[k])]
    col = {(k, j): c for c, (k, j) in enumerate((k, j) for k in loci for j in range(num[k]))}
    out = ask(m, pats)
    assert not out["status"].any()
    n = 0
    for q in range(len(gp["indiv"])):
        i, k = int(gp["indiv"][q]), int(gp["locus"][q])
        for j in range(num[k]):
            want = sum((Fraction(float(p)) * (int(lo == j) + int(hi == j)) for (lo, hi), p in zip(gp["pairs"].tolist(), gp["post"][q])),
                       Fraction(0))
            assert close_large(out["dosage"][i, col[k, j]], want, g, t[i]), (i, k, j, out["dosage"][i, col[k, j]], float(want))
            n += 1
    # at a locus typed in the input: the allele's count in the genotype (an absent allele: exactly 0)
    typed = 0
    for i in range(N):
        for k in loci:
            if (a[i, :, k] < 0).any():
                continue
            for j in range(num[k]):
                c = int((a[i, :, k] == sym[k, j]).sum())
                d = out["dosage"][i, col[k, j]]
                assert (d == 0.0) if c == 0 else close_large(d, Fraction(c), g, t[i]), (i, k, j, d, c)
                typed += 1
    # two heterozygous loci, -1 between: pair_posteriors' cis and trans
    sl = m.pair_span_list(3)
    pr = m.pair_posteriors(sl["indiv"], sl["locus_a"], sl["locus_b"])
    assert len(sl["indiv"]) > 300 and not pr["status"].any()
    specs = []
    for i, x, y in zip(sl["indiv"].tolist(), sl["locus_a"].tolist(), sl["locus_b"].tolist()):
        lx, hx, ly, hy = (int(v) for v in (a[i, :, x].min(), a[i, :, x].max(), a[i, :, y].min(), a[i, :, y].max()))
        gap = (dn.ANY,) * (y - x - 1)
        specs += [(x, (lx,) + gap + (ly,), (hx,) + gap + (hy,)), (x, (lx,) + gap + (hy,), (hx,) + gap + (ly,))]
    uniq = sorted(set(specs))
    at = {s: c for c, s in enumerate(uniq)}
    out = ask(m, uniq)
    for q, i in enumerate(sl["indiv"].tolist()):
        for c in range(2):
            d = out["dosage"][i, at[specs[2 * q + c]]]
            assert close_large(d, pr["post"][q, c], g, t[i]), (q, c, d, pr["post"][q, c])
    # every locus given: the posterior of a drawn pair
    D = 64
    dr = m.posterior_draws(D, 11)
    assert not dr["status"].any()
    for i in range(N):
        pairs = sorted({(tuple(h[0].tolist()), tuple(h[1].tolist())) for h in dr["hap"][i]})
        prob = {(tuple(h[0].tolist()), tuple(h[1].tolist())): float(p) for h, p in zip(dr["hap"][i], dr["prob"][i])}
        one = ask(m, [(0, h0, h1) for h0, h1 in pairs], [i])
        assert one["status"][0] == 0
        for (h0, h1), d in zip(pairs, one["dosage"][0]):
            want = prob[h0, h1] * (2 if h0 == h1 else 1)
            assert close_large(d, want, g, t[i]), (i, d, want)
    print(dict(missing_site_values=n, typed_values=typed, pair_rows=len(sl["indiv"]), g=float(g)))
    assert n > 600 and typed > 1000


# ------------------------------------------------------------ extended range ----
def test_extended_range_on_the_mixed_panel():
    """Regular range: rows of zeros with status 1 / 2 where the other calls
    have them; extended range: status 0 everywhere and the all -1 pattern is 2."""
    b = mixed_panel(MIXED_L)
    m = large_model(b)
    N, _, L = b.shape
    est = m.estep_results()
    assert (est["status"] == 1).any() and (est["status"] == 0).any()
    pats = [(0, (dn.ANY,) * L, None), (5, tuple(int(x) for x in b[4, 0, 5:13]), None), (L - 1, (int(b[5, 0, L - 1]),), None)]
    assert all(x >= 0 for _, A, _ in pats[1:] for x in A)
    reg = ask(m, pats)
    dr = m.posterior_draws(1, 0)
    assert reg["status"].tobytes() == dr["status"].tobytes()
    assert {1, 2} <= set(reg["status"].tolist()) and (reg["status"] == 0).any()
    assert not reg["dosage"][reg["status"] != 0].any()
    m.set_posterior_range(True)
    ext = ask(m, pats)
    m.set_posterior_range(False)
    F = int(m.frontier_max().max())
    g = en.gamma(rowsum_k(L, F) + 1)
    assert g < 1e-6
    assert not ext["status"].any() and m.dosage_stats()["n_pruned"] == 0
    assert all(abs(Fraction(float(d)) - 2) <= 2 * g for d in ext["dosage"][:, 0])
    assert ((ext["dosage"] >= 0) & (ext["dosage"] <= 2 + float(2 * g))).all()
    # where the regular range answers: within the sum of the two bounds
    tot = est["total"]
    for i in np.nonzero(reg["status"] == 0)[0]:
        t = (6 * L * F * F + 2 * F) * ETA / Fraction(float(tot[i]))
        for x, y in zip(reg["dosage"][i], ext["dosage"][i]):
            assert close_large(x, y, g, t), (i, x, y)
    assert same_bytes(ask(m, pats), reg)  # the range set back: the regular bytes again


@pytest.mark.parametrize("name", ["a3", "snp"])
def test_extended_range_on_scaled_tables(name):
    """A table scaled by a power of two until every total underflows: the
    regular range gives every row up, the extended range answers with the bytes
    of the unscaled table's extended run, which meet the enumeration's bound."""
    a = build_panel(name)
    S = PANELS[name]["S"][0]
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    m.resolve_all()
    pats = dn.panel_patterns(a, pt, 1)
    reg = ask(m, pats)
    m.set_posterior_range(True)
    res = check_dosages(m, a, pt, 1)
    ext = ask(m, pats)
    print(name, "extended", res)
    N, _, L = a.shape
    ta = en.allele_table(a)
    for i in range(N):  # regular against extended: the sum of the two bounds
        g = en.gamma(dosage_k(L, en.phasing_count(a[i], ta)))
        assert all(close_large(x, y, g, 0) for x, y in zip(reg["dosage"][i], ext["dosage"][i])), i
    m2 = gpu_model(name, S, a)
    feed(m2, scaled(pt, SUBNORMAL_C[name]))
    m2.resolve_all()
    gone = ask(m2, pats)
    assert (gone["status"] == 2).all() and not gone["dosage"].any()
    m2.set_posterior_range(True)
    assert same_bytes(ask(m2, pats), ext)


# ------------------------------------------------------- call order and errors ----
def raw_call(m, n, indiv, P, start, ln, maxlen, A):
    i32 = lambda x: None if x is None else np.ascontiguousarray(x, np.int32)  # noqa: E731
    indiv, start, ln, A = i32(indiv), i32(start), i32(ln), i32(A)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    out = np.full((max(n, 1), max(P, 1)), -7.0)
    st = np.full(max(n, 1), -7, np.int32)
    rc = lib().hmc_haplotype_dosages(m._h, n, ptr(indiv), P, ptr(start), ptr(ln), maxlen, ptr(A), None,
                                     out.ctypes.data_as(C.POINTER(C.c_double)), ptr(st))
    return rc, out, st


def test_errors_and_call_order():
    a = build_panel("a3")
    N, _, L = a.shape
    m = gpu_model("a3", 3, a)
    pats = [(0, (int(a[0, 0, 0]),), None), (2, (dn.ANY, dn.ANY, dn.ANY), None)]
    m.find_patterns()
    with pytest.raises(HMCError) as ei:
        ask(m, pats)
    assert ei.value.code == -1  # HMC_EARG: no E-step yet
    m.resolve_all()
    ref = ask(m, pats)
    assert not ref["status"].any()
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        ask(m, pats)
    assert ei.value.code == -1
    m.resolve_all()
    ref = ask(m, pats)
    assert not ref["status"].any() and ref["dosage"].shape == (N, 2)
    assert m.dosage_stats()["groups"] >= 1 and m.dosage_stats()["sweep_ms"] > 0
    # n = 0 and n_patterns = 0 succeed with no device work: zero stats, nothing written
    out = ask(m, pats, [])
    assert out["dosage"].shape == (0, 2) and not any(m.dosage_stats().values())
    ask(m, pats)
    out = ask(m, [])
    assert out["dosage"].shape == (N, 0) and not out["status"].any() and not any(m.dosage_stats().values())
    rc, o, s = raw_call(m, 0, [0], 1, [0], [1], 1, [[-1]])
    assert rc == 0 and (o == -7).all() and (s == -7).all()
    rc, o, s = raw_call(m, 2, [0, 1], 0, None, None, 0, None)
    assert rc == 0 and (o == -7).all()
    # HMC_EARG, naming the first offender
    for what, who in (("below the shard", [0, -1]), ("past the shard", [0, N])):
        with pytest.raises(HMCError) as ei:
            ask(m, pats, who)
        assert ei.value.code == -1 and "entry 1" in str(ei.value), (what, str(ei.value))
    bad = {"negative start": (-1, (dn.ANY,), None), "empty": (0, (), None), "past the last locus": (L - 1, (dn.ANY, dn.ANY), None),
           "start past the panel": (L, (dn.ANY,), None)}
    for what, p in bad.items():
        with pytest.raises(HMCError) as ei:
            ask(m, [pats[0], p, pats[1]])
        assert ei.value.code == -1 and "pattern 1" in str(ei.value), (what, str(ei.value))
    rc, _, _ = raw_call(m, 1, [0], 2, [0, 0], [1, 3], 2, [[-1, -1], [-1, -1]])  # len > maxlen
    assert rc == -1 and b"pattern 1" in lib().hmc_ctx_error(m._h)
    assert same_bytes(ask(m, pats), ref)  # a refused call leaves nothing behind
    for slots, tier in ((3, 0), (16, 0), (-2, 0), (0, -1), (0, 255), (2, 1016), (0, 1 << 20)):
        with pytest.raises(HMCError) as ei:
            m.set_dosage_tuning(slots, tier)
        assert ei.value.code == -1, (slots, tier)
    m.set_dosage_tuning(8, 254)
    assert same_bytes(ask(m, pats), ref)
    m.set_dosage_tuning(0, 0)


def test_leaves_the_em_untouched():
    """find_patterns, resolve_all, [haplotype_dosages], em_iteration: the same
    LL, pairs and next table with and without the call; what the last E-step
    left is unchanged by it, and so are the other posterior calls."""
    a = build_panel("a4")
    pats = [(0, (dn.ANY,) * a.shape[2], None), (1, (int(a[0, 0, 1]), int(a[0, 0, 2])), None)]

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.find_patterns()
        _, H, _ = m.resolve_all()
        state = []
        if call:
            others = lambda: (m.genotype_posteriors(), m.switch_posteriors(), m.posterior_draws(4, 1))  # noqa: E731
            o0 = others()
            before = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier(), m.resolutions())
            assert ask(m, pats)["dosage"].shape == (a.shape[0], 2)
            after = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier(), m.resolutions())
            state = [before, after, o0, others()]
        log, old, go = m.em_iteration(1, -np.finfo(np.float64).max)
        log = {k: v for k, v in log.items() if not k.startswith("t_")}
        return state, (log, old, go, m.resolutions(), m.patterns(), m.estep_results())

    def same(x, y):
        if isinstance(x, dict):
            return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (tuple, list)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, np.ndarray):
            return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        return x == y

    state, with_call = chain(True)
    _, without = chain(False)
    assert same(state[0], state[1]), "hmc_get_estep rows, samples, resolutions or E-step statistics moved"
    assert same(state[2], state[3]), "another posterior call moved"
    assert same(with_call, without)
    assert np.isfinite(with_call[0]["log_likelihood"])


# ------------------------------------------------------------------------ CLI ----
def test_cli_output_dosages(tmp_path):
    """hmc_resolve --output-dosages FILE --haplotypes HAPFILE on a3 as a PHASE
    file: one line per individual of status 0 and pattern, the numbers read
    back to the API's doubles; '?' and the '|' form are parsed; a malformed
    line fails with its number."""
    a = build_panel("a3")
    N, _, L = a.shape
    src, hapf, dst = tmp_path / "a3.inp", tmp_path / "a3.haps", tmp_path / "a3.dosages"
    synth.write_phase(synth.Panel(a, "S" * L), str(src))
    g = a[0]
    typed = [k for k in range(L - 2) if (g[:, k:k + 3] >= 0).all()][0]
    pats = [("one", 0, (int(a[1, 0, 0]),), None), ("any", 2, (dn.ANY, int(a[2, 0, 3]), dn.ANY), None),
            ("pair", typed, tuple(int(x) for x in g[0, typed:typed + 3]), tuple(int(x) for x in g[1, typed:typed + 3])),
            ("all", 0, (dn.ANY,) * L, (dn.ANY,) * L)]
    spell = lambda row: " ".join("?" if x == dn.ANY else chr(x) for x in row)  # noqa: E731
    text = "# haplotypes of the test\n\n"
    for name, s, A, B in pats:
        text += f"{name}\t{s} {spell(A)}" + (f" | {spell(B)}" if B is not None else "") + "\n"
    hapf.write_text(text)
    r = subprocess.run([CLI, "--output-dosages", str(dst), "--haplotypes", str(hapf), str(src)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    out = ask(m, [(s, A, B) for _, s, A, B in pats])
    assert not out["status"].any()
    lines = dst.read_text().splitlines()
    assert lines[0] == "Id\tHaplotype\tDosage" and len(lines) - 1 == N * len(pats)
    for q, ln in enumerate(lines[1:]):
        i, p = divmod(q, len(pats))
        f = ln.split("\t")
        assert len(f) == 3 and f[0].lstrip("#") == str(i + 1) and f[1] == pats[p][0]
        assert float(f[2]) == float(out["dosage"][i, p])
    assert ((out["dosage"] > 0.01) & (out["dosage"] < 1.99)).any()
    # the Python writer gives the same file
    dst2 = tmp_path / "a3.dosages2"
    m.write_haplotype_dosages(str(dst2), [p[0] for p in pats], [p[1] for p in pats], [p[2] for p in pats],
                              [p[3] if p[3] is not None else (dn.ANY,) * len(p[2]) for p in pats])
    assert dst2.read_text() == dst.read_text()
    # malformed lines: the line number is named, nothing is written
    for bad, lineno in (("x 0 A | C G\n", 4), ("x\t99 A\n", 4), ("x 0 AC\n", 4), ("x 0\n", 4), ("x zero A\n", 4), ("x 0 A | C | G\n", 4)):
        hapf.write_text("# c\n\nok 0 ?\n" + bad)
        dst.unlink(missing_ok=True)
        r = subprocess.run([CLI, "--output-dosages", str(dst), "--haplotypes", str(hapf), str(src)], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1 and f"line {lineno}" in r.stderr, (bad, r.stderr)
        assert not dst.exists()
    for args in (["--output-dosages", str(dst)], ["--haplotypes", str(hapf)]):
        r = subprocess.run([CLI, *args, str(src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--haplotypes" in r.stderr and "Usage" in r.stderr, r.stderr
