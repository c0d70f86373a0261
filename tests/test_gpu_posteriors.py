"""hmc_genotype_posteriors (exact_query.hip exact_site_posteriors) on the GPU: the
posterior of the unordered genotype at every locus with a missing input
allele, against exhaustive enumeration (tests/posterior_enumeration.py) and
against itself across groupings and shards.

Bound of one bin against enumeration (posterior_k), u = 2^-53, every addend
non-negative so nothing cancels; L loci, M the enumerator's count of ordered
phasings of the individual (enumeration.phasing_count):
  forward likelihood of a state   at most 2L+2 multiplications (per locus the
        two transition probabilities multiplied, then into the running value;
        the head's doubling is exact) and, the sums merging at most M
        prefixes of phasings, M additions: 2L+2+M   (as check_estep's total);
  backward likelihood             the same chain from the other end: 2L+2+M;
  their product                   1;
  the bin's sum                   a lane adds at most ceil(F/64) <= M of its
        states' products, then 6 butterfly steps: M+6;
  P(genotype), the divisor        check_estep's total: 2L+2+M, fewer than the
        dividend's roundings, so the quotient of the two (1 + theta) factors
        is 1 + theta of the sum of the counts (Higham, Lemma 3.3);
  the division                    1.
Together 6L + 4M + 14 roundings: gamma(6L + 4M + 14) relative, at most
gamma(6*10 + 4*1960 + 14) = 8.8e-13 on these panels (asserted <= 1e-12).  A
row's exact bins sum to 1, so the exact sum of a row's doubles is within the
same bound of 1.

On the large panels no enumeration exists and M is astronomical; there only
"a row sums to 1" is held, within rowsum_k: an addend of a sequential sum of c
terms passes c-1 additions, a state has at most 2F contributions (each state
of the locus before, either orientation) and at most 2F forward links, F the
largest number of lattice states at a locus (frontier_max(), a count of the
structure, not a value under test); per locus 2 multiplications and 2F
additions for the forward, the backward and the divisor's chain each, then the
product, the bin's sum (F/64 + 6) and the division: 3L(2F+2) + F + 8.
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
import posterior_enumeration as pe
from test_enumeration_oracle import build_panel, head_len, perturbed_tables, prune
from test_gpu_enumeration import feed, gpu_model, gpu_view

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")


class BinMismatch(AssertionError):
    """A bin of a row is outside its bound of the enumerated posterior."""


def posterior_k(L, M):
    return 6 * L + 4 * M + 14


def rowsum_k(L, F):
    return 3 * L * (2 * F + 2) + F + 8


def exact_sum(row):
    return sum((Fraction(float(x)) for x in row), Fraction(0))


def check_posteriors(m, a, pt, hl):
    """Every site of the library's answer against enumeration; returns the
    largest observed error in units of u and the loosest bound used."""
    out = m.genotype_posteriors()
    num, sym, _ = m.allele_table()
    N, _, L = a.shape
    ta = en.allele_table(a)
    quirk = en.head_quirk(a, hl)
    assert quirk.sum() <= 1 and quirk.sum() <= N / 4
    exact = pe.site_posteriors(a, pt, hl)
    want = pe.sites(a)
    assert list(zip(out["indiv"].tolist(), out["locus"].tolist())) == want
    assert out["post"].shape == (len(want), m.amax * (m.amax + 1) // 2)
    assert out["pairs"].tolist() == [[lo, hi] for hi in range(m.amax) for lo in range(hi + 1)]
    assert not out["status"].any()
    worst, loosest, nz = 0.0, Fraction(0), 0
    for q, (i, k) in enumerate(want):
        row = out["post"][q]
        g = en.gamma(posterior_k(L, en.phasing_count(a[i], ta)))
        assert g <= 1e-12
        loosest = max(loosest, g)
        if quirk[i]:  # the head pairing is no phasing model: the normalisation only
            assert abs(exact_sum(row) - 1) <= g, (i, k, float(exact_sum(row) - 1))
            continue
        ex = exact[i, k]
        for b, (lo, hi) in enumerate(out["pairs"].tolist()):
            e = ex.get((int(sym[k, lo]), int(sym[k, hi])), Fraction(0)) if hi < num[k] else Fraction(0)
            if e == 0:
                assert row[b] == 0.0, (i, k, lo, hi, row[b])
                continue
            if not en.within(row[b], e, g):
                raise BinMismatch((i, k, lo, hi, en.relerr(row[b], e)))
            worst = max(worst, en.relerr(row[b], e))
            nz += 1
        assert abs(exact_sum(row) - 1) <= g, (i, k, float(exact_sum(row) - 1))
    return dict(sites=len(want), nonzero_bins=nz, worst_u=worst / float(en.U), loosest_bound=float(loosest))


@pytest.mark.parametrize("name,S", [("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5)])
def test_against_enumeration(name, S):
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    print(name, S, check_posteriors(m, a, pt, hl), m.posterior_stats())


def test_after_a_windowed_estep():
    """The call runs its own exact-mode structure pass, so it answers the same
    after a windowed E-step (the fused E-step is in the variants library only)."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.set_estep_windows("always", 3)
    m.find_patterns()
    pt = m.patterns()
    m.resolve_all()
    assert m.estep_windows()["windows"] == -(-a.shape[2] // 3)
    print(check_posteriors(m, a, pt, 1))


def test_hand_pruned_table():
    """The pruned table of test_hand_pruned_table_follows_the_chain through
    set_patterns: the chain differs from the global longest match."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pruned, ndrop = prune(m.patterns(), en.allele_table(a), a.shape[2])
    assert ndrop >= 3 and en.check_chain_equals_global(a, pruned, 1) > 0
    m2 = gpu_model(name, S, a)
    feed(m2, pruned)
    m2.resolve_all()
    print(check_posteriors(m2, a, pruned, 1))


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the check raises."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    view = gpu_view(m)
    check_posteriors(m, a, pt, 1)
    bad_tp, _ = perturbed_tables(a, pt, view, 1)
    m2 = gpu_model(name, S, a)
    feed(m2, bad_tp)
    m2.resolve_all()
    with pytest.raises(BinMismatch) as ei:  # a bin comparison fires, not the order, status or row-sum checks
        check_posteriors(m2, a, pt, 1)
    i, k, lo, hi, err = ei.value.args[0]
    print("first bin outside its bound: individual", i, "locus", k, "pair", (lo, hi), "relative error", err)
    assert 0 < err < 1e-8  # the size of the perturbation, not a wrong table


# (N, L) of the path-independence panel: its largest frontier is 890 states (asserted > 256), so a
# lane of the site kernel takes several states and a 256-thread loop over a record strides
BITS_SHAPE = (60, 120)
# (trace bytes, record bytes): stores too small for the 60 individuals of a large panel at once
# (measured: three groups on the 60 x 120 panel at 4 MiB, five on the 60 x 1 600 one at 16 MiB)
BITS_BUDGETS = (1 << 22, 1 << 22)
PRUNED_BUDGETS = (1 << 24, 1 << 24)


def mosaic_with_heads(N, L, A, missing, seed):
    a = synth.founder_mosaic(N, L, A=A, missing=missing, seed=seed).alleles.copy()
    a[:, :, :1] = synth.founder_mosaic(N, L, A=A, missing=0.0, seed=seed).alleles[:, :, :1]
    return a


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


ETA = Fraction(1, 2 ** 1074)  # smallest subnormal double: a result below 2^-1022 is off by up to ETA / 2, not u
DBL_MIN = 2.0 ** -1022


def check_rows_sum_to_one(m, out):
    """Every row of status 0 sums to 1; rows of status 2 are exactly those of
    the resolved individuals whose P(genotype) is below DBL_MIN, and are zeros.

    Bound of a status-0 row: |exact sum - 1| <= gamma(rowsum_k) + (6 L F^2 + F) ETA / P(genotype).
    The second term is the underflow of the likelihoods themselves (exact_fb and the value pass
    keep raw doubles): an absolute error e in a forward value travels on through the same
    non-negative linear maps as the value, so it reaches the row's sum as e x backward <= e; per
    locus and state at most 2F operations can each add ETA / 2, over L loci and F states, alike
    for the backward values and for P(genotype) from the value pass, and F products: (3 L 2F F +
    F) ETA absolute, relative to P(genotype) = estep_results()["total"], an input of the
    posterior.  With P(genotype) >= DBL_MIN, which status 0 guarantees, it is at most (6 L F^2 +
    F) 2^-52: 1.4e-7 at L = 1 600, F = 256; the whole bound must stay below 1e-6 (asserted), so
    no row passes on a vacuous bound.  Returns the largest deviation and the largest bound."""
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
        gq = g + (6 * m.L * F * F + F) * ETA / Fraction(float(total[q]))
        assert gq < 1e-6, (q, float(gq))
        d = abs(exact_sum(out["post"][q]) - 1)
        assert d <= gq, (q, float(d), float(gq), float(total[q]))
        dev, gmax = max(dev, float(d)), max(gmax, float(gq))
    return dict(rows=int((out["status"] == 0).sum()), worst_dev=dev, largest_bound=gmax,
                rows_status_1=int((out["status"] == 1).sum()), rows_status_2=int((out["status"] == 2).sum()))


def test_bits_independent_of_path():
    """One group, forced groups and a shard give the same bits."""
    N, L = BITS_SHAPE
    a = mosaic_with_heads(N, L, 3, 0.05, 7)
    m = large_model(a)
    assert int(m.frontier_max().max()) > 256, m.frontier_max().max()
    ref = m.genotype_posteriors()
    assert m.posterior_stats()["groups"] == 1
    assert len(ref["indiv"]) == int(((a[:, 0] < 0) | (a[:, 1] < 0)).sum()) > 100
    print("row sums", check_rows_sum_to_one(m, ref), m.posterior_stats())
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = m2.genotype_posteriors()
    print(m2.posterior_stats())
    assert m2.posterior_stats()["groups"] >= 2
    for k in ("indiv", "locus", "status"):
        assert np.array_equal(ref[k], got[k])
    assert ref["post"].tobytes() == got["post"].tobytes()
    m3 = large_model(a, shard=(20, 40))
    part = m3.genotype_posteriors()
    sel = (ref["indiv"] >= 20) & (ref["indiv"] < 40)
    assert sel.sum() > 0 and np.array_equal(part["indiv"], ref["indiv"][sel])
    assert np.array_equal(part["locus"], ref["locus"][sel])
    assert part["post"].tobytes() == np.ascontiguousarray(ref["post"][sel]).tobytes()


@pytest.mark.parametrize("exact", [False, True])
def test_leaves_the_em_untouched(exact):
    """find_patterns, resolve_all, [genotype_posteriors], find_patterns,
    resolve_all: the same bits with and without the call."""
    a = build_panel("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.exact_estimate = exact
        m.find_patterns()
        _, H, _ = m.resolve_all()
        state = []
        if call:
            before = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            assert len(m.genotype_posteriors()["indiv"]) > 0
            after = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            state = [before, after]
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
    assert same(with_call, without)


def test_unresolved_individuals():
    """The i.i.d. panel of test_underflow_unresolved with 20 alleles missing:
    sites of unresolved individuals are marked and zero, the others sum to 1.
    (On this panel all six individuals come out unresolved, so every site is
    of the first kind; test_resolved_next_to_unresolved holds the other.)"""
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 2, (6, 2, 2500)) + ord("1")).astype(np.int32)
    r2 = np.random.default_rng(11)
    for _ in range(20):
        a[r2.integers(0, 6), r2.integers(0, 2), r2.integers(1, 2500)] = -1
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(a, "S" * 2500))
    m.find_patterns()
    m.resolve_all()
    st = m.estep_results()["status"]
    assert (st == 1).any()
    out = m.genotype_posteriors()
    assert len(out["indiv"]) == int(((a[:, 0] < 0) | (a[:, 1] < 0)).sum())
    dead = st[out["indiv"]] == 1
    assert np.array_equal(out["status"], dead.astype(np.int32))
    assert not out["post"][dead].any()
    print("unresolved individuals", int((st == 1).sum()), "their sites", int(dead.sum()), "of", len(dead),
          "row sums", check_rows_sum_to_one(m, out), m.posterior_stats())


MIXED_L = 1200  # measured: six individuals unresolved, six resolved, one of those with a subnormal P(genotype)


def mixed_panel(L):
    """Nine founder-mosaic individuals, which the mined patterns explain, and
    three of i.i.d. alleles, which they do not; 36 alleles missing at loci >= 1."""
    a = synth.founder_mosaic(12, L, A=2, seed=1).alleles.copy()
    a[:3] = (np.random.default_rng(5).integers(0, 2, (3, 2, L)) + ord("1")).astype(np.int32)
    r = np.random.default_rng(11)
    for i in range(12):
        for _ in range(3):
            a[i, r.integers(0, 2), r.integers(1, L)] = -1
    return a


def test_resolved_next_to_unresolved():
    """A panel on which some individuals are unresolved and others are not:
    the first have marked rows of zeros, the others' rows sum to 1."""
    a = mixed_panel(MIXED_L)
    m = large_model(a)
    st = m.estep_results()["status"]
    assert (st == 1).any() and (st == 0).any()
    out = m.genotype_posteriors()
    assert np.array_equal(out["status"] == 1, st[out["indiv"]] == 1)
    res = check_rows_sum_to_one(m, out)
    print("unresolved individuals", np.nonzero(st == 1)[0].tolist(), res, m.posterior_stats())
    assert res["rows"] >= 12 and res["rows_status_1"] >= 12


def test_pruned_records():
    """A long panel on which one individual's forward likelihoods underflow
    (its records are rebuilt with extend()'s forward test, n_pruned = 1).
    Every row of status 0 sums to 1 within the non-vacuous bound of
    check_rows_sum_to_one; that individual's P(genotype) is subnormal, so its
    54 rows carry status 2 and are zeros (without the mark they missed 1 by
    up to 0.95: the divisor has a few bits).  One group and forced groups
    give the same bits and the same marks."""
    a = synth.founder_mosaic(60, 1600, A=2, seed=1).alleles.copy()
    r = np.random.default_rng(3)
    miss = r.random((60, 2, 1600)) < 0.01
    miss[:, :, 0] = False
    a[miss] = -1
    m = large_model(a)
    ref = m.genotype_posteriors()
    s1 = m.posterior_stats()
    res = check_rows_sum_to_one(m, ref)
    print("n_pruned", s1["n_pruned"], s1, "row sums", res)
    assert s1["groups"] == 1 and s1["n_pruned"] >= 1
    assert res["rows_status_2"] == 54 and res["rows_status_1"] == 0 and res["rows"] == len(ref["indiv"]) - 54
    m2 = large_model(a, budgets=PRUNED_BUDGETS)
    got = m2.genotype_posteriors()
    s2 = m2.posterior_stats()
    print(s2)
    assert s2["groups"] >= 2 and s2["n_pruned"] == s1["n_pruned"]
    assert np.array_equal(ref["status"], got["status"]) and ref["post"].tobytes() == got["post"].tobytes()


def test_call_order_and_counting():
    a = build_panel("snp")
    m = gpu_model("snp", 2, a)
    assert m.genotype_posterior_shape() == (0, 3)
    b = build_panel("a3")
    m = gpu_model("a3", 3, b)
    ns = int(((b[:, 0] < 0) | (b[:, 1] < 0)).sum())
    assert ns > 12 and m.genotype_posterior_shape() == (ns, 6)  # counted before any model exists
    m.find_patterns()
    with pytest.raises(HMCError) as ei:
        m.genotype_posteriors()
    assert ei.value.code == -1  # HMC_EARG: no E-step yet
    m.resolve_all()
    assert len(m.genotype_posteriors()["indiv"]) == ns
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        m.genotype_posteriors()
    assert ei.value.code == -1
    m.resolve_all()
    assert len(m.genotype_posteriors()["indiv"]) == ns


def test_cli_output_posteriors(tmp_path):
    """hmc_resolve --output-posteriors on a3 as a PHASE file: the numbers read
    back to the API's doubles, the symbols are the allele table's."""
    a = build_panel("a3")
    src = tmp_path / "a3.inp"
    synth.write_phase(synth.Panel(a, "S" * a.shape[2]), str(src))
    r = subprocess.run([CLI, "--output-posteriors", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    out = m.genotype_posteriors()
    _, sym, _ = m.allele_table()
    lines = (tmp_path / "a3.inp.posteriors").read_text().splitlines()
    assert lines[0] == "Id\tMarker\tAlleleLo\tAlleleHi\tPosterior"
    exp, markers = [], {}
    for q in range(len(out["indiv"])):
        for b, (lo, hi) in enumerate(out["pairs"].tolist()):
            if out["post"][q, b] != 0.0:
                exp.append((int(out["indiv"][q]), int(out["locus"][q]), int(sym[out["locus"][q], lo]),
                            int(sym[out["locus"][q], hi]), float(out["post"][q, b])))
    assert len(lines) - 1 == len(exp) > 12
    for ln, (i, k, slo, shi, p) in zip(lines[1:], exp):
        f = ln.split("\t")
        assert len(f) == 5
        assert f[0].lstrip("#") == str(i + 1) and markers.setdefault(f[1], k) == k
        assert (ord(f[2]), ord(f[3])) == (slo, shi)
        assert float(f[4]) == p
    assert len(markers) == len(set(out["locus"].tolist()))
