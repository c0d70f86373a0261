"""hmc_ranked_phasings (exact_query.hip exact_ranked_phasings) on the GPU: the k most
probable haplotype pairs, each once, with their exact posteriors — against
exhaustive enumeration (tests/ranked_enumeration.py), against hmc_map_phase
(row 0, byte for byte), against itself across k and everything else the result
must not depend on, and on the mosaic, where enumeration is impossible, against
the haplotype dosages and the posterior draws.

Bounds, u = 2^-53, L loci, gamma(n) = n u / (1 - n u):
  rows       ranked_enumeration.reject_reason: distinct pairs, count = min(k,
             pairs of positive posterior), e(c_r) >= e*_r (1 - g) / (1 + g),
             g = gamma(2L + 2);
  prob       within gamma(4L + 5 + M) of the pair's enumerated posterior
             (test_gpu_posterior_draws.draw_k: the same computation as a
             draw's prob);
  order      prob[r + 1] <= prob[r] (1 + gamma(4L + 6)): the sweep ranks
             computed values of at most 2L + 2 roundings, prob is another
             product of as many in a different association, each quotient
             rounded once (test_gpu_map_phase.BEAM_K);
  dosage     a heterozygous row's prob against haplotype_dosages of the
             two-sided pattern that spells it: the same pair's posterior as a
             quotient over a lattice sum — per record a state's product (1),
             the sum of its contributions in any order (fewer than F, the
             largest frontier), the final sum over at most F states, one
             division, (L + 2)(F + 2) + 1 — against prob's 2L + 3
             (test_gpu_map_phase.test_statuses_and_extended_range).
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hmc_amd
from hmc_amd import synth
from hmc_amd._lib import HMCError

import draw_enumeration as de
import enumeration as en
import ranked_enumeration as re_
import test_gpu_map_phase as tm
from test_enumeration_oracle import build_panel, head_len
from test_gpu_enumeration import feed, gpu_model
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, ETA, MIXED_L, mixed_panel
from test_gpu_posterior_draws import SEED, ValueMismatch, check_genotype, draw_k, large_model
from test_scaled_tables import scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
KS = (1, 4, 8, 16)  # list widths 2, 4, 8, 16
WIDTH = {1: 2, 3: 4, 4: 4, 8: 8, 16: 16}
D_MOSAIC = 4096
K_MOSAIC = 8
FIELDS = ("hap", "prob", "count", "status")


def same(x, y, rows_x=slice(None), rows_y=slice(None), fields=FIELDS):
    for f in fields:
        assert np.ascontiguousarray(x[f][rows_x]).tobytes() == np.ascontiguousarray(y[f][rows_y]).tobytes(), f


def row0(out):
    return dict(hap=np.ascontiguousarray(out["hap"][:, 0]), prob=np.ascontiguousarray(out["prob"][:, 0]), status=out["status"])


def first_rows(out, r):
    return dict(hap=out["hap"][:, :r], prob=out["prob"][:, :r], count=np.minimum(out["count"], r), status=out["status"])


def keys_of(out, i):
    return [de.pair_key(out["hap"][i, r, 0], out["hap"][i, r, 1]) for r in range(int(out["count"][i]))]


def check_ranked(m, a, pt, hl, ks=KS):
    """ranked_phasings of every individual at every k of `ks` against enumeration; returns statistics."""
    N, _, L = a.shape
    ta, syms = tm.syms_of(a)
    ranked = re_.ranked_exact(a, pt, hl)
    quirk = en.head_quirk(a, hl)
    g_order = en.gamma(tm.BEAM_K(L))
    worst, loosest, rows, short, mirrors = 0.0, Fraction(0), 0, 0, 0
    for k in ks:
        out = m.ranked_phasings(k)
        assert out["hap"].shape == (N, k, 2, L) and out["prob"].shape == (N, k) and out["count"].shape == (N,)
        assert not out["status"].any() and m.ranked_stats()["k_built"] == WIDTH[k]
        for i in range(N):
            cnt = int(out["count"][i])
            assert 1 <= cnt <= k
            check_genotype(out["hap"][i, :cnt], a[i], syms, hl if quirk[i] else 0)
            keys = keys_of(out, i)
            assert len(set(keys)) == cnt, (k, i, "a pair listed twice")
            for r in range(cnt, k):  # rows past the count: the input genotype at prob 0
                assert (out["hap"][i, r] == a[i]).all() and out["prob"][i, r] == 0
            if quirk[i]:  # the head pairing is no phasing model: genotype consistency and distinctness only
                continue
            e = ranked[i]
            assert re_.reject_reason(keys, cnt, k, e, L) is None, (k, i, re_.reject_reason(keys, cnt, k, e, L))
            post = dict(e)
            g = en.gamma(draw_k(L, en.phasing_count(a[i], ta)))
            assert g <= 1e-12
            loosest = max(loosest, g)
            for r, key in enumerate(keys):
                p = float(out["prob"][i, r])
                if not en.within(p, post[key], g):
                    raise ValueMismatch((i, key, en.relerr(p, post[key])))
                worst = max(worst, en.relerr(p, post[key]))
                if r:
                    assert Fraction(p) <= Fraction(float(out["prob"][i, r - 1])) * (1 + g_order), (k, i, r)
            rows += cnt
            short += cnt < k
            mirrors += sum(re_.het_behind_hom_first(key) for key in keys)
    return dict(rows=rows, individuals_with_fewer_pairs_than_rows=short, mirror_pairs_listed=mirrors,
                prob_bound=float(loosest), worst_u=worst / float(en.U), stats=m.ranked_stats())


@pytest.mark.parametrize("name,S", tm.MAP_PANEL_S)
def test_against_enumeration(name, S):
    """Every row passes the enumeration's predicate at k = 1, 4, 8 and 16, prob
    is within the draws' bound of the pair's enumerated posterior and
    descending within the order bound, every row is a phasing of the genotype,
    rows past the count are the input genotype at prob 0.  Prints the rows
    checked, how many individuals had fewer pairs than rows, how many listed
    pairs are heterozygous behind a homozygous first locus (two mirror lattice
    paths each; tests/test_ranked_enumeration.py asserts the panels have them
    in their top rows) and the worst relative error of prob in units of u."""
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    st = check_ranked(m, a, pt, hl)
    print(name, S, st)
    assert st["mirror_pairs_listed"] >= 1


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the comparison of prob raises."""
    from test_enumeration_oracle import perturbed_tables
    from test_gpu_enumeration import gpu_view
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
        check_ranked(m2, a, pt, 1, ks=(4,))
    assert 0 < ei.value.args[0][2] < 1e-8  # the size of the perturbation


def tiny(name="a3", S=3, windowed=False):
    a = build_panel(name)
    m = gpu_model(name, S, a)
    if windowed:
        m.set_estep_windows("always", 3)
    m.find_patterns()
    m.resolve_all()
    return a, m


def both_ranges(m, fn):
    for ext in (False, True):
        m.set_posterior_range(ext)
        try:
            fn(ext)
        finally:
            m.set_posterior_range(False)


def test_row_0_is_map_phase():
    """Rows [:, 0] of ranked_phasings(k) are map_phase()'s bytes (hap, prob,
    status) for each k, in both ranges, on a tiny panel and on the 60 x 120
    mosaic, whose frontiers exceed 256 states."""
    _, m = tiny()
    a2, m2, _, _ = tm.mosaic()
    assert int(m2.frontier_max().max()) > 256
    for model in (m, m2):
        def check(ext, model=model):
            ref = model.map_phase()
            assert not ref["status"].any()
            for k in KS:
                out = model.ranked_phasings(k)
                assert (out["count"] >= 1).all()
                tm.same(row0(out), ref)
        both_ranges(model, check)


def test_k_does_not_enter():
    """The k = 4 rows are the first 4 of k = 16 and the k = 3 rows the first 3
    of k = 8, byte for byte — list widths 4 against 16 and 4 against 8 — on a
    tiny panel and on the mosaic."""
    _, m = tiny()
    _, m2, _, _ = tm.mosaic()
    for model in (m, m2):
        for small, large in ((4, 16), (3, 8)):
            same(model.ranked_phasings(small), first_rows(model.ranked_phasings(large), small))


def mosaic_ranked():
    a, m, _, _ = tm.mosaic()
    if "ranked" not in tm._cache:
        tm._cache["ranked"] = (m.ranked_phasings(K_MOSAIC), m.ranked_stats())
    return (a, m) + tm._cache["ranked"]


def test_mosaic_cross_checks():
    """The 60 x 120 mosaic, k = 8: rows distinct, sum of prob at most 1; every
    heterozygous row's prob against haplotype_dosages of the two-sided pattern
    that spells the whole pair; no draw of 4 096 more probable than row 0, a
    draw equal to a listed pair carries that row's prob, and the draws land in
    the listed set as often as the sum of prob says."""
    a, m, out, stats = mosaic_ranked()
    N, L = BITS_SHAPE
    K = K_MOSAIC
    assert stats["groups"] == 1 and stats["k_built"] == 8 and not out["status"].any()
    _, syms = tm.syms_of(a)
    for i in range(N):
        cnt = int(out["count"][i])
        assert cnt >= 1
        check_genotype(out["hap"][i, :cnt], a[i], syms)
        assert len(set(keys_of(out, i))) == cnt
        assert (out["prob"][i, :cnt] > 0).all() and not out["prob"][i, cnt:].any()
        assert Fraction(0) < sum(Fraction(float(x)) for x in out["prob"][i]) <= 1 + Fraction(1, 10 ** 12)
    # the dosages: (L + 2)(F + 2) + 1 operations against 2L + 3
    F = int(m.frontier_max().max())
    g = en.gamma(2 * L + 3 + (L + 2) * (F + 2) + 1)
    compared = 0
    for i in range(N):
        cnt = int(out["count"][i])
        het = [r for r in range(cnt) if (out["hap"][i, r, 0] != out["hap"][i, r, 1]).any()]
        if not het:
            continue
        ds = m.haplotype_dosages([0] * len(het), [out["hap"][i, r, 0].tolist() for r in het],
                                 [out["hap"][i, r, 1].tolist() for r in het], indiv=[i])
        assert not ds["status"].any()
        for q, r in enumerate(het):
            assert tm.close(out["prob"][i, r], ds["dosage"][0, q], g), (i, r, out["prob"][i, r], ds["dosage"][0, q])
            compared += 1
    # the draws
    dr = m.posterior_draws(D_MOSAIC, SEED)
    assert not dr["status"].any()
    g_top, g_same = en.gamma(tm.BEAM_K(L)), en.gamma(2 * tm.BEAM_K(L))
    hits, comparisons = [], 0
    for i in range(N):
        cnt = int(out["count"][i])
        assert Fraction(float(dr["prob"][i].max())) <= Fraction(float(out["prob"][i, 0])) * (1 + g_top), i
        h = dr["hap"][i]
        listed = np.zeros(D_MOSAIC, bool)
        for r in range(cnt):
            row = out["hap"][i, r]
            eq = (h == row[None]).all(axis=(1, 2)) | (h == row[None, ::-1]).all(axis=(1, 2))
            p = Fraction(float(out["prob"][i, r]))
            assert all(en.within(float(x), p, g_same) for x in np.unique(dr["prob"][i][eq])), (i, r)
            assert not (listed & eq).any()
            listed |= eq
        tot = min(float(sum(Fraction(float(x)) for x in out["prob"][i, :cnt])), 1.0)
        n_in = int(listed.sum())
        comparisons += de.check_frequencies({"listed": n_in, "other": D_MOSAIC - n_in}, D_MOSAIC,
                                            {"listed": tot, "other": max(1.0 - tot, 0.0)})
        hits.append(n_in)
    print("mosaic: dosage comparisons", compared, "bound", float(g), "; draws inside the listed", K, "pairs (min, max of",
          D_MOSAIC, ")", min(hits), max(hits), "; sum of prob min / median",
          float(out["prob"].sum(axis=1).min()), float(np.median(out["prob"].sum(axis=1))), stats)
    assert compared >= N


def test_determinism_small():
    a, m = tiny()
    k = 4
    full = m.ranked_phasings(k)
    same(full, m.ranked_phasings(k))  # two calls
    pick = [7, 2, 2, 9, 0, 7]  # a subset, permuted, with repeats
    same(m.ranked_phasings(k, pick), full, rows_y=pick)
    m.posterior_draws(64, SEED)  # other calls of the family in between
    m.map_phase()
    same(m.ranked_phasings(k), full)
    m.set_ranked_tuning(list_budget(m))  # several launches per group
    same(m.ranked_phasings(k), full)
    assert m.ranked_stats()["batches"] >= 2
    m.set_ranked_tuning(0)
    m.set_shard(3, 8)
    m.resolve_all()
    same(m.ranked_phasings(k), full, rows_y=slice(3, 8))
    same(m.ranked_phasings(k, [7, 3]), full, rows_y=[7, 3])
    _, mw = tiny(windowed=True)  # a windowed E-step before the call
    assert mw.estep_windows()["windows"] == -(-a.shape[2] // 3)
    same(mw.ranked_phasings(k), full)


def list_budget(m):
    """A list-store budget that forces several launches and refuses nobody: the
    bytes the values of the largest individual can take (16 per state of its at
    most L + 1 records of at most F states, 8 per record).  An individual alone
    may take 1.5 width times the budget, which is then what its lists (24 width
    bytes per state) can take; the shard together takes more than the budget."""
    F = int(m.frontier_max().max())
    return 16 * (m.L + 1) * F + 8 * (m.L + 1)


def test_determinism_large():
    """The mosaic: a permuted subset with repeats, forced groups, several
    batches of the list store and a shard give the bytes of the one-group run."""
    a, m, ref, _ = mosaic_ranked()
    k = K_MOSAIC
    same(m.ranked_phasings(k), ref)
    pick = [59, 0, 31, 31, 7, 59]
    same(m.ranked_phasings(k, pick), ref, rows_y=pick)
    m.set_ranked_tuning(list_budget(m))
    got = m.ranked_phasings(k)
    print(m.ranked_stats())
    assert m.ranked_stats()["batches"] >= 2 and m.ranked_stats()["groups"] == 1
    m.set_ranked_tuning(0)
    same(got, ref)
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = m2.ranked_phasings(k)
    print(m2.ranked_stats())
    assert m2.ranked_stats()["groups"] >= 2
    same(got, ref)
    m3 = large_model(a, shard=(20, 40))
    same(m3.ranked_phasings(k), ref, rows_y=slice(20, 40))


def test_statuses_and_extended_range():
    """The mixed panel (1 200 loci), k = 4: statuses equal map_phase's in both
    ranges; rows of status 1 and 2 are the input genotype at prob 0 with count
    0; where both ranges give status 0 the haplotypes are the same bytes and
    prob agrees within test_gpu_map_phase.test_statuses_and_extended_range's
    bound (stated there); row 0 is map_phase's in both."""
    a = mixed_panel(MIXED_L)
    L = a.shape[2]
    k = 4
    m = large_model(a)
    ref = m.map_phase()
    reg = m.ranked_phasings(k)
    assert np.array_equal(reg["status"], ref["status"])
    assert (reg["status"] == 1).sum() >= 1 and (reg["status"] == 2).sum() >= 1 and (reg["status"] == 0).sum() >= 4
    tm.same(row0(reg), ref)
    _, syms = tm.syms_of(a)

    def check_rows(out):
        for i in range(a.shape[0]):
            cnt = int(out["count"][i])
            if out["status"][i] != 0:
                assert cnt == 0
            else:
                assert cnt >= 1
                check_genotype(out["hap"][i, :cnt], a[i], syms)
                assert len(set(keys_of(out, i))) == cnt
                assert (out["prob"][i, :cnt] > 0).all() and out["prob"][i].sum() <= 1 + 1e-9
            for r in range(cnt, k):
                assert (out["hap"][i, r] == a[i]).all() and out["prob"][i, r] == 0

    check_rows(reg)
    reg_stats = m.ranked_stats()
    m.set_posterior_range(True)
    ext = m.ranked_phasings(k)
    ext_ref = m.map_phase()
    assert np.array_equal(ext["status"], ext_ref["status"]) and not (ext["status"] == 2).any()
    assert m.ranked_stats()["n_pruned"] == 0
    tm.same(row0(ext), ext_ref)
    check_rows(ext)
    both = np.nonzero((reg["status"] == 0) & (ext["status"] == 0))[0]
    assert len(both) >= 4
    F = int(m.frontier_max().max())
    g = en.gamma(2 * L + 3 + (L + 2) * (F + 2))
    total = m.estep_results()["total"]
    for i in both:
        assert reg["hap"][i].tobytes() == ext["hap"][i].tobytes() and reg["count"][i] == ext["count"][i], i
        for r in range(int(reg["count"][i])):
            slack = (Fraction(L + 2) + Fraction(float(reg["prob"][i, r])) * (6 * L * F * F + F)) * ETA / Fraction(float(total[i]))
            assert tm.close(reg["prob"][i, r], ext["prob"][i, r], g, slack), (i, r, reg["prob"][i, r], ext["prob"][i, r])
    m.set_posterior_range(False)
    same(m.ranked_phasings(k), reg)
    print("regular", reg["status"].tolist(), reg["count"].tolist(), reg_stats, "extended", ext["status"].tolist(),
          ext["count"].tolist(), m.ranked_stats(), "bound", float(g))


@pytest.mark.parametrize("name", ["a3", "hom"])
def test_extended_range_ignores_a_power_of_two(name):
    """Every freq and tp of the table times 2^-40: no byte of the extended result changes."""
    a = build_panel(name)
    S = 3
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()

    def fed(table, extended):
        x = gpu_model(name, S, a)
        feed(x, table)
        x.resolve_all()
        x.set_posterior_range(extended)
        return x.ranked_phasings(8)

    ref, got = fed(pt, True), fed(scaled(pt, 40), True)
    assert not ref["status"].any()
    same(got, ref)
    reg = fed(pt, False)  # and the regular range on the unscaled table: the same pairs
    assert not reg["status"].any() and reg["hap"].tobytes() == ref["hap"].tobytes()


def test_errors_and_empty_calls():
    a = build_panel("a3")
    L = a.shape[2]
    m = gpu_model("a3", 3, a)
    m.find_patterns()
    pt = m.patterns()
    with pytest.raises(HMCError) as ei:
        m.ranked_phasings(4)
    assert ei.value.code == -1 and "E-step" in str(ei.value) and "ranked phasings" in str(ei.value)  # HMC_EARG: no E-step yet
    m.resolve_all()
    assert m.ranked_phasings(4)["hap"].shape == (10, 4, 2, L)
    for k in (0, 17, -3):
        with pytest.raises(HMCError) as ei:
            m.ranked_phasings(k)
        assert ei.value.code == -1 and "k = %d" % k in str(ei.value)
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        m.ranked_phasings(4)
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    feed(m, pt)  # set_patterns after the E-step
    with pytest.raises(HMCError) as ei:
        m.ranked_phasings(4)
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.ranked_phasings(4, [1, 10, 11])
    assert ei.value.code == -1 and "individual 10" in str(ei.value)
    m.set_ranked_tuning(8)  # a list store that holds nobody: the individual is named
    with pytest.raises(HMCError) as ei:
        m.ranked_phasings(4, [6, 2])
    assert ei.value.code == -7 and "individual" in str(ei.value)  # HMC_ENOMEM
    m.set_ranked_tuning(0)
    m.set_shard(2, 6)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.ranked_phasings(4, [3, 1])
    assert ei.value.code == -1 and "individual 1 " in str(ei.value)
    out = m.ranked_phasings(4, [])  # n = 0
    assert out["hap"].shape == (0, 4, 2, L) and out["prob"].shape == (0, 4)
    assert m.ranked_stats()["groups"] == 0 and m.ranked_stats()["k_built"] == 0
    # every output NULL through the raw call
    assert hmc_amd.lib().hmc_ranked_phasings(m._h, 0, None, 4, None, None, None, None) == 0
    assert m.ranked_stats()["groups"] == 1 and m.ranked_stats()["k_built"] == 4
    with pytest.raises(HMCError) as ei:
        m.write_ranked_phasings(os.devnull, 17)
    assert ei.value.code == -1


def test_leaves_the_em_untouched():
    """find_patterns, resolve_all, [ranked_phasings], find_patterns,
    resolve_all: the same bits with and without the call."""
    a = build_panel("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.find_patterns()
        _, H, _ = m.resolve_all()
        if call:
            before = (m.estep_results(), m.samples(H), m.switch_posteriors(), m.map_phase())
            assert m.ranked_phasings(16)["prob"][:, 0].all()
            after = (m.estep_results(), m.samples(H), m.switch_posteriors(), m.map_phase())
            assert repr(before) == repr(after)
        m.find_patterns()
        pt = m.patterns()
        ll, H2, re = m.resolve_all()
        return repr((pt, ll, H2, re, m.samples(H2), m.estep_results(), m.resolutions()))

    with np.printoptions(threshold=1 << 30, floatmode="unique"):
        assert chain(True) == chain(False)


def parse_ranked_file(path, L):
    """[(id, [prob], [hap[2][L]])] per individual, in file order."""
    lines = open(path).read().splitlines()
    assert lines[0] == "Id\tRank\tPosterior\tHaplotype0\tHaplotype1"
    out = []
    for line in lines[1:]:
        f = line.split("\t")
        assert len(f) == 5
        if not out or out[-1][0] != f[0]:
            out.append((f[0], [], []))
        assert int(f[1]) == len(out[-1][1])  # ranks from 0, ascending
        out[-1][1].append(float(f[2]))
        hap = [[ord(c) for c in f[3 + side].split(" ")] for side in range(2)]
        assert len(hap[0]) == L and len(hap[1]) == L
        out[-1][2].append(hap)
    return out


def test_cli_output_ranked(tmp_path):
    """hmc_resolve --output-ranked on a3 as a PHASE file writes what
    write_ranked_phasings writes, the file parses back to ranked_phasings()'s
    arrays, and the phased output is byte-identical to a run without the option."""
    a = build_panel("a3")
    N, _, L = a.shape
    src = tmp_path / "a3.inp"
    synth.write_phase(synth.Panel(a, "S" * L), str(src))
    r = subprocess.run([CLI, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "a3.inp.reconstructed").read_bytes()
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    for k, args in ((4, []), (16, ["--ranked", "16"])):  # the default K is 4
        dst = tmp_path / ("ranked%d.tsv" % k)
        r = subprocess.run([CLI, "--output-ranked", str(dst)] + args + [str(src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "a3.inp.reconstructed").read_bytes() == plain
        out = m.ranked_phasings(k)
        assert not out["status"].any()
        own = tmp_path / ("own%d.tsv" % k)
        m.write_ranked_phasings(str(own), k)
        assert own.read_bytes() == dst.read_bytes()
        rows = parse_ranked_file(dst, L)
        assert len(rows) == N and len({x[0] for x in rows}) == N
        for i, (_, prob, hap) in enumerate(rows):
            cnt = int(out["count"][i])
            assert len(prob) == cnt
            assert np.array(prob).tobytes() == out["prob"][i, :cnt].tobytes()
            assert np.array(hap, np.int32).tobytes() == np.ascontiguousarray(out["hap"][i, :cnt]).tobytes()
    ext = tmp_path / "ext.tsv"
    r = subprocess.run([CLI, "--output-ranked", str(ext), "--extended-range", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert [x[2] for x in parse_ranked_file(ext, L)] == [x[2] for x in parse_ranked_file(tmp_path / "ranked4.tsv", L)]
    r = subprocess.run([CLI, "--output-ranked"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--output-ranked" in r.stderr
    r = subprocess.run([CLI, "--ranked", "3", str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--ranked needs --output-ranked" in r.stderr
    r = subprocess.run([CLI, "--output-ranked", str(ext), "--ranked", "17", str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--ranked" in r.stderr
