"""hmc_pair_posteriors (exact_query.hip exact_pair_posteriors) on the GPU: for
caller-given pairs (a, b) of heterozygous loci of an individual, any distance
apart, the posterior that their lower alleles share a haplotype (cis) and that
they do not (trans) — against exhaustive enumeration
(tests/pair_enumeration.py), against itself across every schedule (slots per
state NS, rounds, the LDS tier, query order, duplicates, a query asked alone,
store groups, a shard) byte for byte, and against hmc_switch_posteriors on
span-1 queries byte for byte.

Bound of one value against enumeration (switch_k of
test_gpu_switch_posteriors), u = 2^-53, every addend non-negative so nothing
cancels; L loci, M the enumerator's count of ordered phasings of the
individual (enumeration.phasing_count):
  labelled forward value of a state  it starts as the anchor record's forward
        likelihood and goes on through the same chain — per locus the state's
        product of two transition probabilities (one rounding) multiplied into
        the running value (one), and sums that merge at most M prefixes of
        phasings, a subset of the forward likelihood's own terms.  Carrying
        the label through more loci (a distant b) only goes further along that
        chain: whatever the distance, a value at record b + 1 has passed at
        most all L loci, so over the whole panel at most 2L+2 multiplications
        and M additions: 2L+2+M, as for a forward likelihood — no operation
        beyond those already counted for the consecutive case;
  backward likelihood                2L+2+M;
  their product                      1 (the scaling by powers of two is exact);
  the query's sum                    a lane adds at most ceil(F/64) <= M of its
        states' products, then 6 butterfly steps: M+6;
  P(genotype), the divisor           2L+2+M (check_estep's total);
  the division                       1.
Together 6L + 4M + 14 roundings: gamma(6L + 4M + 14) relative, at most
gamma(6*10 + 4*1960 + 14) = 8.8e-13 on these panels (asserted <= 1e-12).  The
exact cis and trans sum to 1, so the exact sum of a row's two doubles is within
the same bound of 1.  Measured on the MI355X: worst error 4.4 u (a3) over the
468 enumerated all-pairs queries of the seven panels.

On the large panels no enumeration exists; there rows are held to sum to 1
within test_gpu_switch_posteriors.check_rows_sum_to_one's bound (rowsum_k with
the two-sum underflow term), on span-1 queries, where the sweep is the
consecutive one.
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
import pair_enumeration as pe
import switch_enumeration as se
from test_enumeration_oracle import build_panel, head_len, perturbed_tables, prune
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, MIXED_L, exact_sum, mixed_panel, mosaic_with_heads
from test_gpu_switch_posteriors import check_rows_sum_to_one, switch_k
from test_pair_enumeration import COUNTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
SLOTS = (1, 2, 4, 8)  # every instantiated NS
SPILL_TIER = 1     # every record of two or more states goes through the device-memory scratch
PANEL_CASES = [("snp", 2), ("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5), ("minlen2", 10)]


class ValueMismatch(AssertionError):
    """cis or trans of a query is outside its bound of the enumerated posterior."""


def ask(m, queries):
    q = np.array(queries, np.int32).reshape(-1, 3)
    return m.pair_posteriors(q[:, 0], q[:, 1], q[:, 2])


def same_bytes(x, y):
    return x["status"].tobytes() == y["status"].tobytes() and x["post"].tobytes() == y["post"].tobytes()


def check_schedules(m, queries, ref, overlap, lds_holds_all=True):
    """The same queries under every schedule: identical bytes."""
    for ns in SLOTS:
        m.set_pair_tuning(ns, 0)
        assert same_bytes(ask(m, queries), ref), ns
        st = m.pair_stats()
        assert st["slots"] == ns
        assert (st["max_rounds"] > 1) == (overlap > ns), (ns, overlap, st)
        if lds_holds_all:
            assert st["n_spilled"] == 0  # the default tier
        if ns == 2:
            assert overlap >= 3 and st["max_rounds"] > 1  # anchors that found no free slot took a later round
        m.set_pair_tuning(ns, SPILL_TIER)
        assert same_bytes(ask(m, queries), ref), (ns, "spilled")
        assert m.pair_stats()["n_spilled"] > 0
    m.set_pair_tuning(0, 0)
    # shuffled, with duplicates: rows follow the caller's order
    rng = np.random.default_rng(len(queries))
    pick = np.concatenate([rng.permutation(len(queries)), rng.integers(0, len(queries), max(3, len(queries) // 4))])
    got = ask(m, [queries[k] for k in pick])
    assert got["status"].tobytes() == ref["status"][pick].tobytes()
    assert got["post"].tobytes() == np.ascontiguousarray(ref["post"][pick]).tobytes()
    # a single query asked alone
    for k in sorted({0, len(queries) // 2, len(queries) - 1, int(rng.integers(0, len(queries)))}):
        one = ask(m, [queries[k]])
        assert one["post"].tobytes() == ref["post"][k].tobytes() and one["status"][0] == ref["status"][k], queries[k]
        assert m.pair_stats()["max_rounds"] == 1 and m.pair_stats()["slots"] == 1


def check_pairs(m, a, pt, hl, counts=None, schedules=True):
    """All pairs of heterozygous loci of every individual against enumeration;
    returns the largest observed error in units of u and the loosest bound."""
    N, _, L = a.shape
    queries = pe.all_pairs(a)
    overlap = pe.max_overlap(queries)
    m.set_pair_tuning(0, 0)
    out = ask(m, queries)
    stats = m.pair_stats()
    assert stats["n_spilled"] == 0 and stats["max_rounds"] >= 1
    assert stats["slots"] == (1 if overlap <= 1 else 2 if overlap <= 2 else 4 if overlap <= 4 else 8)
    assert out["post"].shape == (len(queries), 2) and not out["status"].any()
    if schedules:
        check_schedules(m, queries, out, overlap)
    num, sym, _ = m.allele_table()
    ta = en.allele_table(a)
    for k in range(L):  # "lower index" is "lower symbol": the two definitions agree
        assert sym[k, :num[k]].tolist() == sorted(s for s, _ in ta[k])
    quirk = en.head_quirk(a, hl)
    assert quirk.sum() <= 1 and quirk.sum() <= N / 4
    exact = pe.pair_posteriors(a, pt, hl, queries)
    if counts is not None:  # what ran: the shapes of the module docstring of test_pair_enumeration
        enum = [q for q in queries if not quirk[q[0]]]
        het = {i: pe.het_loci(a[i]) for i in range(N)}
        ran = (len(queries), len(enum), sum(1 for _, x, y in enum if x < hl <= y), sum(1 for _, x, y in enum if y < hl),
               sum(1 for i, x, y in enum if any(k not in het[i] for k in range(x + 1, y))),
               sum(1 for i, x, y in enum if het[i].index(y) - het[i].index(x) >= 3), overlap)
        assert ran == counts
        assert ran[2] > 0 and ran[4] > 0 and ran[5] > 0 and (hl < 2 or ran[3] > 0)
    worst, loosest = 0.0, Fraction(0)
    for q, (i, x, y) in enumerate(queries):
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
                assert 0 < e < 1, (i, x, y, c)  # every enumerated query of the seven panels is mixed
            if e == 0:
                assert row[c] == 0.0, (i, x, y, c, row[c])
                continue
            if not en.within(row[c], e, g):
                raise ValueMismatch((i, x, y, c, en.relerr(row[c], e)))
            worst = max(worst, en.relerr(row[c], e))
        assert abs(exact_sum(row) - 1) <= g, (i, x, y, float(exact_sum(row) - 1))
    return dict(queries=len(queries), overlap=overlap, worst_u=worst / float(en.U), loosest_bound=float(loosest), stats=stats)


@pytest.mark.parametrize("name,S", PANEL_CASES)
def test_against_enumeration(name, S):
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    print(name, S, check_pairs(m, a, pt, hl, COUNTS[name]))


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
    print(check_pairs(m, a, pt, 1, schedules=False))


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
    print(check_pairs(m2, a, pruned, 1, schedules=False))


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the value comparison raises."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    view = gpu_view(m)
    check_pairs(m, a, pt, 1, schedules=False)
    bad_tp, _ = perturbed_tables(a, pt, view, 1)
    m2 = gpu_model(name, S, a)
    feed(m2, bad_tp)
    m2.resolve_all()
    with pytest.raises(ValueMismatch) as ei:  # a value comparison fires, not the status, schedule or row-sum checks
        check_pairs(m2, a, pt, 1)
    i, x, y, c, err = ei.value.args[0]
    print("first value outside its bound: individual", i, "query", (x, y), "cis" if c == 0 else "trans", "relative error", err)
    assert 0 < err < 1e-8  # the size of the perturbation, not a wrong table


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


def test_bits_independent_of_path():
    """One group, forced groups, a shard, every NS and a spilling tier give the
    same bits on a panel whose frontiers pass every LDS tier."""
    N, L = BITS_SHAPE
    a = mosaic_with_heads(N, L, 3, 0.05, 7)
    queries = pe.span_list(a, 3)
    assert len(queries) > 300 and pe.max_overlap(queries) == 3
    m = large_model(a)
    fbig = int(m.frontier_max().max())
    assert fbig > 254, fbig  # past the default LDS tier
    ref = ask(m, queries)
    s1 = m.pair_stats()
    print(s1)
    assert s1["groups"] == 1 and s1["slots"] == 4 and s1["n_spilled"] > 0 and s1["max_rounds"] == 1
    assert (ref["status"] == 0).all()
    for ns in SLOTS:  # 1 and 2 slots take rounds; the widest individuals spill at every NS
        m.set_pair_tuning(ns, 0)
        assert same_bytes(ask(m, queries), ref), ns
        st = m.pair_stats()
        print(st)
        assert st["slots"] == ns and (st["max_rounds"] > 1) == (ns <= 2) and 0 < st["n_spilled"] == s1["n_spilled"] < N
    m.set_pair_tuning(0, 64)
    assert same_bytes(ask(m, queries), ref) and m.pair_stats()["n_spilled"] > 0
    m.set_pair_tuning(0, 0)
    # span-1 rows are hmc_switch_posteriors' rows
    sw = m.switch_posteriors()
    consecutive = set(pe.span_list(a, 1))
    span1 = [k for k, q in enumerate(queries) if q in consecutive]
    assert [queries[k] for k in span1] == list(zip(sw["indiv"].tolist(), sw["locus_a"].tolist(), sw["locus_b"].tolist()))
    assert np.ascontiguousarray(ref["post"][span1]).tobytes() == sw["post"].tobytes()
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = ask(m2, queries)
    print(m2.pair_stats())
    assert m2.pair_stats()["groups"] >= 2
    assert same_bytes(got, ref)
    m3 = large_model(a, shard=(20, 40))
    part = [q for q in queries if 20 <= q[0] < 40]
    sel = np.array([20 <= q[0] < 40 for q in queries])
    sl = m3.pair_span_list(3)
    assert list(zip(sl["indiv"].tolist(), sl["locus_a"].tolist(), sl["locus_b"].tolist())) == part
    got = ask(m3, part)
    assert got["post"].tobytes() == np.ascontiguousarray(ref["post"][sel]).tobytes() and not got["status"].any()
    for bad in (queries[0], queries[-1]):  # individuals 0 and 59: outside the shard
        with pytest.raises(HMCError) as ei:
            ask(m3, [part[0], bad])
        assert ei.value.code == -1 and "shard" in str(ei.value) and "query 1" in str(ei.value), str(ei.value)


def triples(d):
    return list(zip(d["indiv"].tolist(), d["locus_a"].tolist(), d["locus_b"].tolist()))


def test_span_one_is_switch_posteriors():
    """pair_span_list(1) is the site list of switch_posteriors and its rows
    have switch_posteriors' bytes, on an enumeration panel and on the mixed
    panel, where status 1 and 2 agree site by site too."""
    a = build_panel("mc")  # head_len 2
    m = gpu_model("mc", 4, a)
    m.find_patterns()
    m.resolve_all()
    sw = m.switch_posteriors()
    sl = m.pair_span_list(1)
    assert triples(sl) == triples(sw) == se.sites(a)
    got = m.pair_posteriors(sl["indiv"], sl["locus_a"], sl["locus_b"])
    assert got["post"].tobytes() == sw["post"].tobytes() and got["status"].tobytes() == sw["status"].tobytes()
    for ns in SLOTS:
        m.set_pair_tuning(ns, SPILL_TIER)
        got = m.pair_posteriors(sl["indiv"], sl["locus_a"], sl["locus_b"])
        assert got["post"].tobytes() == sw["post"].tobytes(), ns
    b = mixed_panel(MIXED_L)
    m = large_model(b)
    st = m.estep_results()["status"]
    assert (st == 1).any() and (st == 0).any()
    sw = m.switch_posteriors()
    sl = m.pair_span_list(1)
    assert triples(sl) == triples(sw) == se.sites(b)
    got = m.pair_posteriors(sl["indiv"], sl["locus_a"], sl["locus_b"])
    assert got["status"].tobytes() == sw["status"].tobytes() and got["post"].tobytes() == sw["post"].tobytes()
    assert np.array_equal(got["status"] == 1, st[sl["indiv"]] == 1)
    res = check_rows_sum_to_one(m, dict(indiv=sl["indiv"], status=got["status"], post=got["post"]))
    print(res, m.pair_stats())
    assert res["rows"] >= 12 and res["rows_status_1"] >= 12 and res["rows_status_2"] >= 1


def test_span_lists():
    a = build_panel("snp")
    m = gpu_model("snp", 2, a)  # counted from the panel: no model yet
    most = max(len(pe.het_loci(a[i])) for i in range(a.shape[0]))
    for K in (1, 2, 5, most + 3):
        assert triples(m.pair_span_list(K)) == pe.span_list(a, K), K
    assert triples(m.pair_span_list(most + 3)) == pe.all_pairs(a)
    assert len(m.pair_span_list(1)["indiv"]) == m.switch_posterior_shape()[0]
    for K in (0, -1):
        with pytest.raises(HMCError) as ei:
            m.pair_span_list(K)
        assert ei.value.code == -1


def test_errors_and_call_order():
    a = build_panel("a3")
    m = gpu_model("a3", 3, a)
    queries = pe.all_pairs(a)
    m.find_patterns()
    with pytest.raises(HMCError) as ei:
        ask(m, queries)
    assert ei.value.code == -1  # HMC_EARG: no E-step yet
    m.resolve_all()
    ref = ask(m, queries)
    assert not ref["status"].any()
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        ask(m, queries)
    assert ei.value.code == -1
    m.resolve_all()
    ref = ask(m, queries)  # (of the new table: other numbers)
    assert not ref["status"].any() and ref["post"].shape == (len(queries), 2)
    # n = 0 succeeds
    out = m.pair_posteriors([], [], [])
    assert out["post"].shape == (0, 2) and len(out["status"]) == 0
    N, _, L = a.shape
    i, x, y = queries[0]
    g = a[i]
    hom = [k for k in range(L) if g[0, k] >= 0 and g[0, k] == g[1, k]]
    missing = [(j, k) for j in range(N) for k in range(L) if (a[j, :, k] < 0).any()]
    assert hom and missing
    jm, km = missing[0]
    hm = [k for k in pe.het_loci(a[jm]) if k != km]
    bad = {"homozygous locus": (i, min(x, hom[0]), max(x, hom[0])) if hom[0] != x else None,
           "missing locus": (jm, min(km, hm[0]), max(km, hm[0])),
           "a = b": (i, x, x), "a > b": (i, y, x), "individual below the shard": (-1, x, y),
           "individual past the shard": (N, x, y), "locus out of range": (i, x, L), "negative locus": (i, -1, y)}
    for what, q in bad.items():
        assert q is not None, what
        with pytest.raises(HMCError) as ei:  # the first offending query is named: it comes second here
            ask(m, [queries[0], q, queries[1]])
        assert ei.value.code == -1 and "query 1" in str(ei.value), (what, str(ei.value))
    assert same_bytes(ask(m, queries), ref)  # a refused call leaves nothing behind
    for slots, tier in ((3, 0), (16, 0), (-2, 0), (0, -1), (0, 255), (2, 1016), (0, 1 << 20)):
        with pytest.raises(HMCError) as ei:  # a slot count not instantiated; a tier past the LDS at NS = 8
            m.set_pair_tuning(slots, tier)
        assert ei.value.code == -1, (slots, tier)
    m.set_pair_tuning(8, 254)
    assert same_bytes(ask(m, queries), ref)
    m.set_pair_tuning(0, 0)


@pytest.mark.parametrize("exact", [False, True])
def test_leaves_the_em_untouched(exact):
    """find_patterns, resolve_all, [pair_posteriors], em_iteration: the same
    LL, pairs and next table with and without the call; what the last E-step
    left is unchanged by it, and the other two posterior calls answer the same
    bytes before and after."""
    a = build_panel("a4")
    queries = pe.all_pairs(a)

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.exact_estimate = exact
        m.find_patterns()
        _, H, _ = m.resolve_all()
        state = []
        if call:
            gp0, sw0 = m.genotype_posteriors(), m.switch_posteriors()
            before = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            assert len(ask(m, queries)["status"]) == len(queries)
            after = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            state = [before, after, (gp0, sw0), (m.genotype_posteriors(), m.switch_posteriors())]
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
    assert same(state[0], state[1]), "hmc_get_estep rows, samples or E-step statistics moved"
    assert same(state[2], state[3]), "genotype or switch posteriors moved"
    assert same(with_call, without)
    assert np.isfinite(with_call[0]["log_likelihood"])


def test_cli_output_pair_posteriors(tmp_path):
    """hmc_resolve --output-pair-posteriors FILE --pair-span 3 on a3 as a PHASE
    file: one line per status-0 query of pair_span_list(3), the numbers read
    back to the API's doubles; without --pair-span the flag is a usage error."""
    a = build_panel("a3")
    src = tmp_path / "a3.inp"
    dst = tmp_path / "a3.pairs"
    synth.write_phase(synth.Panel(a, "S" * a.shape[2]), str(src))
    r = subprocess.run([CLI, "--output-pair-posteriors", str(dst), "--pair-span", "3", str(src)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    sl = m.pair_span_list(3)
    assert triples(sl) == pe.span_list(a, 3)
    out = m.pair_posteriors(sl["indiv"], sl["locus_a"], sl["locus_b"])
    _, sym, _ = m.allele_table()
    lines = dst.read_text().splitlines()
    assert lines[0] == "Id\tMarkerA\tMarkerB\tAlleleA\tAlleleB\tCis\tTrans"
    keep = np.nonzero(out["status"] == 0)[0]
    assert len(lines) - 1 == len(keep) == len(pe.span_list(a, 3)) > COUNTS["a3"][0] // 2
    markers = {}
    for ln, q in zip(lines[1:], keep):
        i, x, y = int(sl["indiv"][q]), int(sl["locus_a"][q]), int(sl["locus_b"][q])
        f = ln.split("\t")
        assert len(f) == 7
        assert f[0].lstrip("#") == str(i + 1)
        assert markers.setdefault(f[1], x) == x and markers.setdefault(f[2], y) == y
        assert (ord(f[3]), ord(f[4])) == (int(a[i, :, x].min()), int(a[i, :, y].min()))
        assert ord(f[3]) in sym[x].tolist() and ord(f[4]) in sym[y].tolist()
        assert (float(f[5]), float(f[6])) == (float(out["post"][q, 0]), float(out["post"][q, 1]))
    assert len(set(markers.values())) == len(markers)
    for args in (["--output-pair-posteriors", str(dst)], ["--output-pair-posteriors", str(dst), "--pair-span", "0"]):
        dst.unlink()
        r = subprocess.run([CLI, *args, str(src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--pair-span" in r.stderr and "Usage" in r.stderr, r.stderr
        assert not dst.exists()  # refused before any work
        dst.write_text("")
