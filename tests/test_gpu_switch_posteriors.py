"""hmc_switch_posteriors (exact_query.hip exact_switch_posteriors) on the GPU: for
every pair of consecutive heterozygous loci of an individual the posterior
that their lower alleles share a haplotype (cis) and that they do not (trans),
against exhaustive enumeration (tests/switch_enumeration.py) and against
itself across groupings, shards and the sweep's two stores.

Bound of one value against enumeration (switch_k), u = 2^-53, every addend
non-negative so nothing cancels; L loci, M the enumerator's count of ordered
phasings of the individual (enumeration.phasing_count):
  labelled forward value of a state  it starts as the anchor record's forward
        likelihood and goes on through the same chain — per locus the state's
        product of two transition probabilities (one rounding) multiplied into
        the running value (one), and sums that merge at most M prefixes of
        phasings, a subset of the forward likelihood's own terms — so over the
        whole panel at most 2L+2 multiplications and M additions: 2L+2+M, as
        for a forward likelihood (test_gpu_posteriors.py);
  backward likelihood                2L+2+M;
  their product                      1 (the scaling by powers of two is exact);
  the site's sum                     a lane adds at most ceil(F/64) <= M of its
        states' products, then 6 butterfly steps: M+6;
  P(genotype), the divisor           2L+2+M (check_estep's total);
  the division                       1.
Together 6L + 4M + 14 roundings: gamma(6L + 4M + 14) relative, at most
gamma(6*10 + 4*1960 + 14) = 8.8e-13 on these panels (asserted <= 1e-12).  The
exact cis and trans sum to 1, so the exact sum of a row's two doubles is within
the same bound of 1.  Measured on the MI355X: worst error 4.4 u (a3).

On the large panels no enumeration exists; there only "a row sums to 1" is
held, within test_gpu_posteriors.rowsum_k: F the largest number of states at a
locus, a state has at most 2F contributions; per locus 2 multiplications and 2F
additions for the labelled forward value (re-anchoring replaces it by a
forward likelihood of the same count), the backward value and the divisor's
chain each, then the product, the site's sum (F/64 + 6) and the division:
3L(2F+2) + F + 8 for each of the two values, and the exact sum of the two adds
no rounding.  The underflow term of check_rows_sum_to_one counts F products for
its one bin; here the two sums take 2F: (6 L F^2 + 2F) ETA / P(genotype).
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hmc_amd
from hmc_amd import synth
from hmc_amd._lib import HMCError

import enumeration as en
import switch_enumeration as se
from test_enumeration_oracle import build_panel, head_len, perturbed_tables, prune
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_gpu_posteriors import (BITS_BUDGETS, BITS_SHAPE, DBL_MIN, ETA, MIXED_L, exact_sum, mixed_panel, mosaic_with_heads,
                                 rowsum_k)
from test_switch_enumeration import COUNTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
SPILL_TIER = 1  # every record of two or more states goes through the device-memory scratch


class ValueMismatch(AssertionError):
    """cis or trans of a site is outside its bound of the enumerated posterior."""


def switch_k(L, M):
    return 6 * L + 4 * M + 14


def check_switches(m, a, pt, hl, counts=None):
    """Every site of the library's answer against enumeration, with the default
    tier and with one that spills (identical bits); returns the largest
    observed error in units of u and the loosest bound used."""
    m.set_switch_tier(0)
    out = m.switch_posteriors()
    stats = m.switch_stats()
    assert stats["n_spilled"] == 0
    m.set_switch_tier(SPILL_TIER)
    spilled = m.switch_posteriors()
    assert m.switch_stats()["n_spilled"] > 0
    m.set_switch_tier(0)
    for k in out:
        assert out[k].tobytes() == spilled[k].tobytes(), k
    num, sym, _ = m.allele_table()
    N, _, L = a.shape
    ta = en.allele_table(a)
    for k in range(L):  # "lower index" is "lower symbol": the two definitions agree
        assert sym[k, :num[k]].tolist() == sorted(s for s, _ in ta[k])
    quirk = en.head_quirk(a, hl)
    assert quirk.sum() <= 1 and quirk.sum() <= N / 4
    exact = se.switch_posteriors(a, pt, hl)
    want = se.sites(a)
    assert list(zip(out["indiv"].tolist(), out["locus_a"].tolist(), out["locus_b"].tolist())) == want
    assert out["post"].shape == (len(want), 2) and m.switch_posterior_shape() == (len(want), 2)
    assert not out["status"].any()
    if counts is not None:
        enum = [s for s in want if not quirk[s[0]]]
        assert (len(want), len(enum), sum(1 for _, x, _ in enum if x < hl), sum(1 for _, x, y in enum if y - x > 1)) == counts
    worst, loosest = 0.0, Fraction(0)
    for q, (i, x, y) in enumerate(want):
        row = out["post"][q]
        g = en.gamma(switch_k(L, en.phasing_count(a[i], ta)))
        assert g <= 1e-12
        loosest = max(loosest, g)
        if quirk[i]:  # the head pairing is no phasing model: the normalisation only
            assert abs(exact_sum(row) - 1) <= g, (i, x, y, float(exact_sum(row) - 1))
            continue
        for c in range(2):
            e = exact[i, x, y][c]
            if counts is not None:
                assert 0 < e < 1, (i, x, y, c)  # every enumerated site of the seven panels is mixed
            if e == 0:
                assert row[c] == 0.0, (i, x, y, c, row[c])
                continue
            if not en.within(row[c], e, g):
                raise ValueMismatch((i, x, y, c, en.relerr(row[c], e)))
            worst = max(worst, en.relerr(row[c], e))
        assert abs(exact_sum(row) - 1) <= g, (i, x, y, float(exact_sum(row) - 1))
    return dict(sites=len(want), worst_u=worst / float(en.U), loosest_bound=float(loosest), stats=stats)


@pytest.mark.parametrize("name,S", [("snp", 2), ("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5), ("minlen2", 10)])
def test_against_enumeration(name, S):
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    print(name, S, check_switches(m, a, pt, hl, COUNTS[name]))


def test_after_a_windowed_estep():
    """The call runs its own exact-mode structure pass, so it answers the same
    after a windowed E-step."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.set_estep_windows("always", 3)
    m.find_patterns()
    pt = m.patterns()
    m.resolve_all()
    assert m.estep_windows()["windows"] == -(-a.shape[2] // 3)
    print(check_switches(m, a, pt, 1))


def test_hand_pruned_table():
    """The pruned table of test_hand_pruned_table_follows_the_chain through
    set_patterns: the successor chain differs from the global longest match."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pruned, ndrop = prune(m.patterns(), en.allele_table(a), a.shape[2])
    assert ndrop >= 3 and en.check_chain_equals_global(a, pruned, 1) > 0
    m2 = gpu_model(name, S, a)
    feed(m2, pruned)
    m2.resolve_all()
    print(check_switches(m2, a, pruned, 1))


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the value comparison raises."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    view = gpu_view(m)
    check_switches(m, a, pt, 1)
    bad_tp, _ = perturbed_tables(a, pt, view, 1)
    m2 = gpu_model(name, S, a)
    feed(m2, bad_tp)
    m2.resolve_all()
    with pytest.raises(ValueMismatch) as ei:  # a value comparison fires, not the site-list, status or row-sum checks
        check_switches(m2, a, pt, 1)
    i, x, y, c, err = ei.value.args[0]
    print("first value outside its bound: individual", i, "site", (x, y), "cis" if c == 0 else "trans", "relative error", err)
    assert 0 < err < 1e-8  # the size of the perturbation, not a wrong table


def large_model(a, budgets=None, shard=None, tier=0):
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * a.shape[2]))
    if budgets:
        m.set_store_budgets(*budgets)
    m.set_switch_tier(tier)
    m.find_patterns()
    if shard:
        m.set_shard(*shard)
    m.resolve_all()
    return m


def check_rows_sum_to_one(m, out):
    """Every row of status 0 sums to 1; rows of status 1 are exactly those of
    the unresolved individuals, rows of status 2 those of the resolved ones
    whose P(genotype) is below DBL_MIN; both kinds are zeros.  Bound of a
    status-0 row: |exact sum - 1| <= gamma(rowsum_k) + (6 L F^2 + 2F) ETA /
    P(genotype) (module docstring; the derivation of the underflow term is
    test_gpu_posteriors.check_rows_sum_to_one's), below 1e-6 (asserted), so no
    row passes on a vacuous bound."""
    F = int(m.frontier_max().max())
    g = en.gamma(rowsum_k(m.L, F))
    er = m.estep_results()
    i0 = getattr(m, "i0", 0)
    total, est = er["total"][out["indiv"] - i0], er["status"][out["indiv"] - i0]
    resolved = (est == 0) & (total > 0)
    assert np.array_equal(out["status"] == 1, ~resolved)
    assert np.array_equal(out["status"] == 2, resolved & (total < DBL_MIN))
    assert not out["post"][out["status"] != 0].any()
    dev, gmax = 0.0, 0.0
    for q in np.nonzero(out["status"] == 0)[0]:
        gq = g + (6 * m.L * F * F + 2 * F) * ETA / Fraction(float(total[q]))
        assert gq < 1e-6, (q, float(gq))
        d = abs(exact_sum(out["post"][q]) - 1)
        assert d <= gq, (q, float(d), float(gq), float(total[q]))
        dev, gmax = max(dev, float(d)), max(gmax, float(gq))
    return dict(rows=int((out["status"] == 0).sum()), worst_dev=dev, largest_bound=gmax,
                rows_status_1=int((out["status"] == 1).sum()), rows_status_2=int((out["status"] == 2).sum()))


def test_bits_independent_of_path():
    """One group, forced groups, a shard and a spilling tier give the same bits."""
    N, L = BITS_SHAPE
    a = mosaic_with_heads(N, L, 3, 0.05, 7)
    m = large_model(a)
    assert int(m.frontier_max().max()) > 256, m.frontier_max().max()
    ref = m.switch_posteriors()
    s1 = m.switch_stats()
    assert s1["groups"] == 1 and s1["n_spilled"] == 0
    assert list(zip(ref["indiv"].tolist(), ref["locus_a"].tolist(), ref["locus_b"].tolist())) == se.sites(a)
    assert len(ref["indiv"]) > 100
    print("row sums", check_rows_sum_to_one(m, ref), s1)
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = m2.switch_posteriors()
    print(m2.switch_stats())
    assert m2.switch_stats()["groups"] >= 2
    for k in ("indiv", "locus_a", "locus_b", "status"):
        assert np.array_equal(ref[k], got[k])
    assert ref["post"].tobytes() == got["post"].tobytes()
    m3 = large_model(a, shard=(20, 40))
    part = m3.switch_posteriors()
    sel = (ref["indiv"] >= 20) & (ref["indiv"] < 40)
    assert sel.sum() > 0 and np.array_equal(part["indiv"], ref["indiv"][sel])
    assert np.array_equal(part["locus_a"], ref["locus_a"][sel]) and np.array_equal(part["locus_b"], ref["locus_b"][sel])
    assert part["post"].tobytes() == np.ascontiguousarray(ref["post"][sel]).tobytes()
    m4 = large_model(a, tier=64)  # frontiers of up to 890 states: most individuals go through the scratch
    sp = m4.switch_posteriors()
    print(m4.switch_stats())
    assert m4.switch_stats()["n_spilled"] > 0
    assert np.array_equal(ref["status"], sp["status"]) and ref["post"].tobytes() == sp["post"].tobytes()


@pytest.mark.parametrize("exact", [False, True])
def test_leaves_the_em_untouched(exact):
    """find_patterns, resolve_all, [switch_posteriors], find_patterns,
    resolve_all: the same bits with and without the call; and
    genotype_posteriors answers the same bytes before and after it."""
    a = build_panel("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.exact_estimate = exact
        m.find_patterns()
        _, H, _ = m.resolve_all()
        state = []
        if call:
            gp0 = m.genotype_posteriors()
            before = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            assert len(m.switch_posteriors()["indiv"]) > 0
            after = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            gp1 = m.genotype_posteriors()
            state = [before, after, gp0, gp1]
        m.find_patterns()
        pt = m.patterns()
        ll, H2, re = m.resolve_all()
        al, w, tw = m.samples(H2)
        er = m.estep_results()
        return state, (pt, ll, H2, re, al, w, tw, er, m.resolutions())

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
    assert same(state[0], state[1]), "hmc_get_estep rows, samples or E-step statistics moved"
    assert same(state[2], state[3]), "genotype posteriors moved"
    assert same(with_call, without)


def test_unresolved_and_subnormal_individuals():
    """The mixed panel of test_resolved_next_to_unresolved: status 1 exactly on
    the unresolved individuals' sites, status 2 exactly where P(genotype) is
    below DBL_MIN, both rows of zeros, every other row sums to 1."""
    a = mixed_panel(MIXED_L)
    m = large_model(a)
    st = m.estep_results()["status"]
    assert (st == 1).any() and (st == 0).any()
    out = m.switch_posteriors()
    assert list(zip(out["indiv"].tolist(), out["locus_a"].tolist(), out["locus_b"].tolist())) == se.sites(a)
    assert np.array_equal(out["status"] == 1, st[out["indiv"]] == 1)
    res = check_rows_sum_to_one(m, out)
    print("unresolved individuals", np.nonzero(st == 1)[0].tolist(), res, m.switch_stats())
    assert res["rows"] >= 12 and res["rows_status_1"] >= 12 and res["rows_status_2"] >= 1


def test_call_order_and_counting():
    b = build_panel("a3")
    m = gpu_model("a3", 3, b)
    ns = len(se.sites(b))
    assert ns == COUNTS["a3"][0] and m.switch_posterior_shape() == (ns, 2)  # counted before any model exists
    m.find_patterns()
    with pytest.raises(HMCError) as ei:
        m.switch_posteriors()
    assert ei.value.code == -1  # HMC_EARG: no E-step yet
    m.resolve_all()
    assert len(m.switch_posteriors()["indiv"]) == ns
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        m.switch_posteriors()
    assert ei.value.code == -1
    m.resolve_all()
    assert len(m.switch_posteriors()["indiv"]) == ns
    with pytest.raises(HMCError) as ei:  # a tier the kernel's LDS cannot hold
        m.set_switch_tier(1 << 20)
    assert ei.value.code == -1
    # no individual with two heterozygous loci: no sites, and the call succeeds
    one, two = ord("1"), ord("2")
    c = np.array([[[one, one, one], [one, two, one]], [[two, one, two], [two, one, one]], [[one, two, two], [one, two, two]],
                  [[one, -1, one], [two, one, -1]]], np.int32)
    assert se.sites(c) == []
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(c, "SSS"))
    assert m.switch_posterior_shape() == (0, 2)
    m.find_patterns()
    m.resolve_all()
    out = m.switch_posteriors()
    assert len(out["indiv"]) == 0 and out["post"].shape == (0, 2)


def test_cli_output_switch_posteriors(tmp_path):
    """hmc_resolve --output-switch-posteriors on a3 as a PHASE file: one line
    per status-0 site, the numbers read back to the API's doubles, the symbols
    are the allele table's."""
    a = build_panel("a3")
    src = tmp_path / "a3.inp"
    synth.write_phase(synth.Panel(a, "S" * a.shape[2]), str(src))
    r = subprocess.run([CLI, "--output-switch-posteriors", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    out = m.switch_posteriors()
    _, sym, _ = m.allele_table()
    lines = (tmp_path / "a3.inp.switches").read_text().splitlines()
    assert lines[0] == "Id\tMarkerA\tMarkerB\tAlleleA\tAlleleB\tCis\tTrans"
    keep = np.nonzero(out["status"] == 0)[0]
    assert len(lines) - 1 == len(keep) == COUNTS["a3"][0]
    markers = {}
    for ln, q in zip(lines[1:], keep):
        i, x, y = int(out["indiv"][q]), int(out["locus_a"][q]), int(out["locus_b"][q])
        f = ln.split("\t")
        assert len(f) == 7
        assert f[0].lstrip("#") == str(i + 1)
        assert markers.setdefault(f[1], x) == x and markers.setdefault(f[2], y) == y
        assert (ord(f[3]), ord(f[4])) == (int(a[i, :, x].min()), int(a[i, :, y].min()))
        assert ord(f[3]) in sym[x].tolist() and ord(f[4]) in sym[y].tolist()
        assert (float(f[5]), float(f[6])) == (float(out["post"][q, 0]), float(out["post"][q, 1]))
    assert len(set(markers.values())) == len(markers)
