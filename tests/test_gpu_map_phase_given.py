"""hmc_map_phase_given on the GPU: MAP phasing over the haplotype pairs that are
consistent with caller-given phase sets, and P(evidence | genotype).

Against enumeration (tests/evidence_enumeration.py: exact rationals over every
phasing) on the seven enumerable panels the draws use, with three evidence
tables per covered individual; against the siblings hmc_pair_posteriors and
hmc_haplotype_dosages for a two-locus set; a negative control; the four
invariants byte for byte on the 60 x 120 mosaic; status 3 on a table with one
transition probability set to 0; statuses and ranges on the 12 x 1 200 mixed
panel; errors, the EM left untouched, the command line.

Bounds.  The returned pair: evidence_enumeration.accepts (consistent, and within
gamma(2L + 2) twice of the constrained maximum).  prob: gamma(draw_k), the
draws' bound of a pair's posterior.  evidence: gamma(evidence_k) with
evidence_k(L, M) = 5L + 5 + 2M, derived in tests/evidence_enumeration.py.  All
derived, none tuned; each test prints the bounds it used and the worst error
in units of u.
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
import evidence_enumeration as ee
import map_enumeration as me
from test_enumeration_oracle import build_panel, head_len, perturbed_tables
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_gpu_haplotype_dosages import dosage_k
from test_gpu_map_phase import BEAM_K, mosaic, parse_map_file, syms_of
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, MIXED_L, mixed_panel
from test_gpu_posterior_draws import PANEL_S, SEED, ValueMismatch, check_genotype, draw_k, large_model
from test_gpu_switch_posteriors import switch_k
from test_scaled_tables import scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
FIELDS = ("hap", "prob", "evidence", "status")


def same(x, y, rows_x=slice(None), rows_y=slice(None), fields=FIELDS):
    for f in fields:
        assert np.ascontiguousarray(x[f][rows_x]).tobytes() == np.ascontiguousarray(y[f][rows_y]).tobytes(), f


def covered_individuals(a, hl):
    """Individuals with two or more heterozygous loci outside the head quirk; the
    coverage the issue states is asserted, so a panel change cannot empty the checks."""
    quirk = en.head_quirk(a, hl)
    cov = [i for i in range(a.shape[0]) if not quirk[i] and len(ee.het_loci(a[i])) >= 2]
    assert len(cov) * 10 >= 6 * a.shape[0], cov
    assert max(len(ee.het_loci(a[i])) for i in cov) >= 4
    return cov


def evidence_tables(a, post, cov):
    """(a) one set over all heterozygous loci spelled from an exact maximiser,
    (b) the same from the exact second-best pair, (c) two disjoint sets, where
    four heterozygous loci allow, from a pair drawn with a fixed seed among
    those of positive posterior."""
    ta, tb, tc = [], [], []
    for i in cov:
        d, het = post[i], ee.het_loci(a[i])
        best = max(d.values())
        argmax = {k for k, p in d.items() if p == best}
        ta += ee.spell(max(argmax), i, [het])
        sb = me.second_best(dict(post=d, argmax=argmax))
        if sb is not None:
            tb += ee.spell(sb[0], i, [het], first_set=3)
        if len(het) >= 4:
            keys = sorted(k for k, p in d.items() if p > 0)
            pick = keys[int(np.random.default_rng(SEED + i).integers(len(keys)))]
            tc += ee.spell(pick, i, [het[:len(het) // 2], het[len(het) // 2:]], first_set=-1)
    return dict(a=ta, b=tb, c=tc)


def check_given(m, a, pt, hl):
    """map_phase_given of every individual under the three tables against enumeration; returns statistics."""
    N, _, L = a.shape
    ta, syms = syms_of(a)
    post = de.pair_posteriors_exact(a, pt, hl)
    cov = covered_individuals(a, hl)
    tables = evidence_tables(a, post, cov)
    assert all(tables.values())
    plain = m.map_phase()
    worst_p = worst_e = 0.0
    loosest_p = loosest_e = Fraction(0)
    n_checked = not_unconstrained = 0
    for which, entries in tables.items():
        out = m.map_phase_given(entries)
        assert out["hap"].shape == (N, 2, L) and out["evidence"].shape == (N,)
        with_entries = {e[0] for e in entries}
        assert m.given_stats()["n_constrained"] == len(with_entries)
        for i in range(N):
            if i not in with_entries:  # invariant 1: hmc_map_phase's bytes, evidence exactly 1.0
                same(out, plain, [i], [i], ("hap", "prob", "status"))
                assert out["evidence"][i] == 1.0
                continue
            assert out["status"][i] == 0, (which, i)
            check_genotype(out["hap"][i][None], a[i], syms)
            key = de.pair_key(out["hap"][i, 0], out["hap"][i, 1])
            c = ee.constrained_exact(post[i], entries, i)
            e_c = post[i].get(key, 0)
            assert ee.consistent(key, entries, i), (which, i, key)
            assert ee.accepts(key, e_c, entries, i, c["best"], L), (which, i, key, float(e_c), float(c["best"]))
            M = en.phasing_count(a[i], ta)
            gp, ge = en.gamma(draw_k(L, M)), en.gamma(ee.evidence_k(L, M))
            assert gp <= 1e-12 and ge <= 1e-12
            loosest_p, loosest_e = max(loosest_p, gp), max(loosest_e, ge)
            p, ev = float(out["prob"][i]), float(out["evidence"][i])
            if not en.within(p, e_c, gp):
                raise ValueMismatch((which, i, "prob", en.relerr(p, e_c)))
            if not en.within(ev, c["evidence"], ge):
                raise ValueMismatch((which, i, "evidence", en.relerr(ev, c["evidence"])))
            worst_p, worst_e = max(worst_p, en.relerr(p, e_c)), max(worst_e, en.relerr(ev, c["evidence"]))
            assert abs(out["given"][i] - p / ev) <= 1e-15
            n_checked += 1
            not_unconstrained += key != de.pair_key(plain["hap"][i, 0], plain["hap"][i, 1])
    g_pair = en.gamma(me.map_roundings(L))
    return dict(covered=len(cov), rows_checked=n_checked, pair_bound=float((1 - g_pair) / (1 + g_pair)), prob_bound=float(loosest_p),
                evidence_bound=float(loosest_e), worst_prob_u=worst_p / float(en.U), worst_evidence_u=worst_e / float(en.U),
                answers_that_differ_from_map_phase=not_unconstrained, stats=m.given_stats())


@pytest.mark.parametrize("name,S", PANEL_S)
def test_against_enumeration(name, S):
    """Genotype consistency, consistency with the evidence, the acceptance
    predicate, prob and evidence within their bounds, for tables (a), (b), (c);
    (b) and (c) must move the answer away from hmc_map_phase's somewhere."""
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    st = check_given(m, a, pt, hl)
    print(name, S, st)
    assert st["rows_checked"] >= 2 * st["covered"] and st["answers_that_differ_from_map_phase"] >= 1


def close2(x, y, g1, g2):
    """Two computed values of one exact positive number, within g1 and g2 of it."""
    x, y = Fraction(float(x)), Fraction(float(y))
    g = max(g1, g2)
    return abs(x - y) <= (g1 + g2) * max(x, y) / (1 - g)


@pytest.mark.parametrize("name,S", [("snp", 2), ("a4", 6), ("mc", 4)])
def test_against_the_siblings(name, S):
    """A single two-locus set (an individual's first and last heterozygous
    locus): evidence against hmc_pair_posteriors' cis or trans and against the
    matching two-sided pattern of hmc_haplotype_dosages, each within the sum
    of the two derived bounds; the two orientations sum to 1 within theirs."""
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    m.resolve_all()
    N, _, L = a.shape
    ta, _ = syms_of(a)
    cov = covered_individuals(a, hl)
    xy = {i: (ee.het_loci(a[i])[0], ee.het_loci(a[i])[-1]) for i in cov}
    lo = lambda i, k: int(a[i, :, k].min())  # noqa: E731
    hi = lambda i, k: int(a[i, :, k].max())  # noqa: E731
    cis = [(i, k, 0, lo(i, k)) for i in cov for k in xy[i]]
    trans = [(i, xy[i][0], 0, lo(i, xy[i][0])) for i in cov] + [(i, xy[i][1], 0, hi(i, xy[i][1])) for i in cov]
    oc, ot = m.map_phase_given(cis), m.map_phase_given(trans)
    pp = m.pair_posteriors(cov, [xy[i][0] for i in cov], [xy[i][1] for i in cov])
    assert not pp["status"].any()
    width = max(y - x + 1 for x, y in xy.values())
    A = [[lo(i, xy[i][0])] + [-1] * (xy[i][1] - xy[i][0] - 1) + [lo(i, xy[i][1])] for i in cov]
    B = [[hi(i, xy[i][0])] + [-1] * (xy[i][1] - xy[i][0] - 1) + [hi(i, xy[i][1])] for i in cov]
    ds = m.haplotype_dosages([xy[i][0] for i in cov], A, B, indiv=cov)
    assert not ds["status"].any() and width >= 2
    worst = 0.0
    for q, i in enumerate(cov):
        M = en.phasing_count(a[i], ta)
        ge, gs, gd = en.gamma(ee.evidence_k(L, M)), en.gamma(switch_k(L, M)), en.gamma(dosage_k(L, M))
        assert oc["status"][i] == 0 and ot["status"][i] == 0
        ec, et = oc["evidence"][i], ot["evidence"][i]
        assert close2(ec, pp["post"][q, 0], ge, gs), (i, ec, pp["post"][q, 0])
        assert close2(et, pp["post"][q, 1], ge, gs), (i, et, pp["post"][q, 1])
        assert close2(ec, ds["dosage"][q, q], ge, gd), (i, ec, ds["dosage"][q, q])
        assert abs(Fraction(float(ec)) + Fraction(float(et)) - 1) <= ge, (i, ec, et)
        worst = max(worst, abs(ec - pp["post"][q, 0]) / ec, abs(et - pp["post"][q, 1]) / et, abs(ec - ds["dosage"][q, q]) / ec)
    print(name, S, "two-locus sets:", len(cov), "worst difference to a sibling in u:", worst / float(en.U), "bounds (evidence, pair, dosage) at the last individual:",
          float(ge), float(gs), float(gd))


def test_negative_control():
    """One tp off by 1e-9 relative in the table the kernels run on (the
    enumerator keeps the true one): the comparison of prob or evidence raises,
    and the size of the miss is the size of the perturbation."""
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
        check_given(m2, a, pt, 1)
    print("negative control:", ei.value.args[0])
    assert 0 < ei.value.args[0][3] < 1e-8


def mosaic_evidence(a, res, keep=lambda i: True):
    """Consecutive heterozygous loci in sets of three, spelled from res[N, 2, L]."""
    out = []
    for i in range(a.shape[0]):
        het = ee.het_loci(a[i])
        if not keep(i):
            continue
        for s in range(0, len(het), 3):
            out += [(i, k, s // 3, int(res[i, 0, k])) for k in het[s:s + 3]]
    return out


def effective(entries):
    """Individuals with a set of two or more loci."""
    n = {}
    for i, k, s, f in entries:
        n[(i, s)] = n.get((i, s), 0) + 1
    return {i for (i, s), c in n.items() if c > 1}


def test_invariants_on_the_mosaic():
    """Invariants 1-4 byte for byte on the 60 x 120 mosaic: entry permutations,
    renamed sets, flipped sets, subsets with repeats, two block sizes and
    grids, a store budget that forces several groups; invariant 1 also in
    extended range; prob against hmc_ranked_phasings(16)."""
    a, m, plain, _ = mosaic()
    N, L = BITS_SHAPE
    res = m.resolutions()
    E = mosaic_evidence(a, res, keep=lambda i: i % 3 != 0)
    E += [(i, ee.het_loci(a[i])[0], 5, int(a[i, 1, ee.het_loci(a[i])[0]])) for i in range(0, N, 6) if ee.het_loci(a[i])]  # single-locus sets
    eff = effective(E)
    assert 30 <= len(eff) <= 40
    ref = m.map_phase_given(E)
    stats = m.given_stats()
    assert stats["n_constrained"] == len(eff) and stats["groups"] == 1
    _, syms = syms_of(a)
    # 1: no effective evidence gives hmc_map_phase's answer and evidence exactly 1.0
    none = [i for i in range(N) if i not in eff]
    same(ref, plain, none, none, ("hap", "prob", "status"))
    assert (ref["evidence"][none] == 1.0).all()
    same(m.map_phase_given([]), dict(plain, evidence=np.ones(N)))
    assert m.given_stats()["n_constrained"] == 0
    differs = 0
    for i in sorted(eff):
        assert ref["status"][i] == 0
        check_genotype(ref["hap"][i][None], a[i], syms)
        key = de.pair_key(ref["hap"][i, 0], ref["hap"][i, 1])
        assert ee.consistent(key, E, i)
        assert 0 < ref["evidence"][i] <= 1 + 1e-9 and 0 < ref["prob"][i] <= plain["prob"][i] * (1 + 1e-9)
        differs += key != de.pair_key(plain["hap"][i, 0], plain["hap"][i, 1])
    # 2: entry order, set names, other individuals, subsets with repeats, launch shapes, groups
    rng = np.random.default_rng(SEED)
    same(m.map_phase_given([E[q] for q in rng.permutation(len(E))]), ref)
    same(m.map_phase_given([(i, k, 1000 - 7 * s, f) for i, k, s, f in E]), ref)
    pick = [59, 1, 31, 31, 0, 7, 59, 6]
    same(m.map_phase_given(E, pick), ref, rows_y=pick)
    same(m.map_phase_given([e for e in E if e[0] in pick], pick), ref, rows_y=pick)
    for block, grid in ((64, 7), (128, 1)):
        assert hmc_amd.lib().hmc_set_given_tuning(m._h, block, grid) == 0
        same(m.map_phase_given(E), ref)
    assert hmc_amd.lib().hmc_set_given_tuning(m._h, 256, 0) == 0
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = m2.map_phase_given(E)
    assert m2.given_stats()["groups"] >= 2 and m2.given_stats()["n_constrained"] == len(eff)
    same(got, ref)
    m3 = large_model(a, shard=(20, 40))
    same(m3.map_phase_given(E), ref, rows_y=slice(20, 40))
    # 3: flipping sets wholesale
    which = {(i, s) for i, k, s, f in E if (i + s) % 2 == 0}
    same(m.map_phase_given(ee.flipped(E, a, which)), ref)
    same(m.map_phase_given(ee.flipped(E, a, {(i, s) for i, k, s, f in E})), ref)
    # 4: prob has the bits hmc_ranked_phasings(16) reports for the same pair; the returned pair is the list's first
    # consistent row wherever the list separates it from the next consistent one by more than the predicate's bound
    rk = m.ranked_phasings(16)
    g = en.gamma(me.map_roundings(L))
    in_list = first_rows = 0
    for i in sorted(eff):
        key = de.pair_key(ref["hap"][i, 0], ref["hap"][i, 1])
        rows = [r for r in range(rk["count"][i]) if ee.consistent(de.pair_key(rk["hap"][i, r, 0], rk["hap"][i, r, 1]), E, i)]
        for r in range(rk["count"][i]):
            if de.pair_key(rk["hap"][i, r, 0], rk["hap"][i, r, 1]) == key:
                assert rk["prob"][i, r].tobytes() == ref["prob"][i].tobytes(), (i, r)
                in_list += 1
        if rows:
            nxt = Fraction(float(rk["prob"][i, rows[1]])) if len(rows) > 1 else Fraction(0)
            if len(rows) > 1 or rk["count"][i] < 16:
                if Fraction(float(rk["prob"][i, rows[0]])) * (1 - g) / (1 + g) > nxt * (1 + g) / (1 - g):
                    assert de.pair_key(rk["hap"][i, rows[0], 0], rk["hap"][i, rows[0], 1]) == key, (i, rows[0])
                    first_rows += 1
    assert in_list >= len(eff) // 4 and first_rows >= 1
    # 1 in extended range
    m.set_posterior_range(True)
    try:
        ext_plain, ext = m.map_phase(), m.map_phase_given(E)
        same(ext, ext_plain, none, none, ("hap", "prob", "status"))
        assert (ext["evidence"][none] == 1.0).all() and not ext["status"].any()
        assert ext["hap"].tobytes() == ref["hap"].tobytes()
    finally:
        m.set_posterior_range(False)
    print("mosaic: constrained", len(eff), "of", N, "; answers that differ from map_phase:", differs, "; returned pairs found in ranked(16):", in_list,
          "; first consistent rows checked:", first_rows, "; evidence min / median", float(ref["evidence"][sorted(eff)].min()),
          float(np.median(ref["evidence"][sorted(eff)])), stats)


def zero_tp_table(a, pt, hl, cov):
    """The first pattern (index order, length >= 2) whose tp set to 0 keeps every
    enumerated individual's P(genotype) > 0 while a covered individual has a
    pair of exact posterior 0: (the table, {individual: such a pair})."""
    for q in range(len(pt["tp"])):
        if pt["len"][q] < 2 or pt["tp"][q] == 0:
            continue
        bad = {k: v.copy() for k, v in pt.items()}
        bad["tp"][q] = 0.0
        es = en.estep(a, bad, hl)
        if any(e is not None and e["total"] == 0 for e in es):
            continue
        hit = {i: min(k for k, p in es[i]["priors"].items() if p == 0) for i in cov if any(p == 0 for p in es[i]["priors"].values())}
        if hit:
            return bad, hit
    raise AssertionError("no such pattern")


def test_status_3():
    """No committed panel has impossible evidence (tests/test_evidence_enumeration.py), so one is made: a table with
    one transition probability set to 0, chosen by enumeration so that a covered individual keeps P(genotype) > 0
    while some pair of its has exact posterior 0; evidence spelled from that pair gives status 3, the input
    genotype and zeros, and the other individuals keep their answers."""
    name, S = "a3", 3
    a = build_panel(name)
    hl = head_len(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    bad, hit = zero_tp_table(a, m.patterns(), hl, covered_individuals(a, hl))
    m2 = gpu_model(name, S, a)
    feed(m2, bad)
    m2.resolve_all()
    plain = m2.map_phase()
    post = de.pair_posteriors_exact(a, bad, hl)
    E, expect3 = [], []
    for i, pair in hit.items():
        if plain["status"][i] != 0:
            continue
        ev = ee.spell(pair, i, [ee.het_loci(a[i])])
        E += ev
        if ee.constrained_exact(post[i], ev, i)["evidence"] == 0:  # (the pair's phase of the heterozygous loci is impossible)
            expect3.append(i)
    assert expect3, hit
    out = m2.map_phase_given(E)
    for i in range(a.shape[0]):
        if i in expect3:
            assert out["status"][i] == 3 and (out["hap"][i] == a[i]).all(), i
            assert out["prob"][i] == 0 and out["evidence"][i] == 0 and out["given"][i] == 0
        elif i not in {e[0] for e in E}:
            same(out, plain, [i], [i], ("hap", "prob", "status"))
        else:
            assert out["status"][i] == 0 and out["evidence"][i] > 0
    print("status 3 on individuals", expect3, "of", sorted(hit), m2.given_stats())


def test_statuses_and_ranges():
    """The mixed panel (12 x 1 200), evidence spelled from resolutions() in
    sets of three consecutive heterozygous loci.  Regular range: statuses 1 and
    2 exactly where map_phase puts them.  Extended range: the statuses of
    map_phase in extended range; the individuals the regular range gave up and
    the extended one resolves get rows consistent with genotype and evidence,
    0 < evidence <= 1 up to its bound and prob <= map_phase's up to
    gamma(BEAM_K).  Bound of evidence here, without enumeration: numerator and
    denominator are sums of positive terms over the lattice — per record a
    state's product (1), the sum of its contributions (fewer than 2F + 1
    additions with the labels' merge), the final sum over at most F states, the
    division: gamma(2 (L + 2)(2F + 3) + 1)."""
    a = mixed_panel(MIXED_L)
    N, _, L = a.shape
    m = large_model(a)
    E = mosaic_evidence(a, m.resolutions())
    reg_plain, reg = m.map_phase(), m.map_phase_given(E)
    assert (reg_plain["status"] == 1).sum() >= 1 and (reg_plain["status"] == 2).sum() >= 1
    assert np.array_equal(reg["status"] == 1, reg_plain["status"] == 1) and np.array_equal(reg["status"] == 2, reg_plain["status"] == 2)
    _, syms = syms_of(a)
    F = int(m.frontier_max().max())
    ge = en.gamma(2 * (L + 2) * (2 * F + 3) + 1)
    gb = en.gamma(BEAM_K(L))
    assert ge < 1e-9

    def check_rows(out, plain, rows):
        for i in rows:
            check_genotype(out["hap"][i][None], a[i], syms)
            assert ee.consistent(de.pair_key(out["hap"][i, 0], out["hap"][i, 1]), E, i), i
            assert 0 < Fraction(float(out["evidence"][i])) <= 1 + ge, (i, out["evidence"][i])
            assert 0 < Fraction(float(out["prob"][i])) <= Fraction(float(plain["prob"][i])) * (1 + gb), (i, out["prob"][i], plain["prob"][i])

    for i in range(N):
        if reg["status"][i] != 0:
            assert (reg["hap"][i] == a[i]).all() and reg["prob"][i] == 0 and reg["evidence"][i] == 0
    check_rows(reg, reg_plain, np.nonzero(reg["status"] == 0)[0])
    assert (reg["status"] == 0).sum() >= 4
    m.set_posterior_range(True)
    ext_plain, ext = m.map_phase(), m.map_phase_given(E)
    assert np.array_equal(ext["status"], ext_plain["status"]) and not (ext["status"] == 2).any()
    gained = np.nonzero((reg["status"] != 0) & (ext["status"] == 0))[0]
    assert len(gained) >= 1
    check_rows(ext, ext_plain, np.nonzero(ext["status"] == 0)[0])
    both = np.nonzero((reg["status"] == 0) & (ext["status"] == 0))[0]
    for i in both:
        assert reg["hap"][i].tobytes() == ext["hap"][i].tobytes(), i
    m.set_posterior_range(False)
    same(m.map_phase_given(E), reg)
    print("regular", reg["status"].tolist(), "extended", ext["status"].tolist(), "gained", gained.tolist(), m.given_stats(), "evidence bound", float(ge))


@pytest.mark.parametrize("name", ["a3", "hom"])
def test_extended_range_ignores_a_power_of_two(name):
    """Every freq and tp of the table times 2^-40: no byte of the extended result changes."""
    a = build_panel(name)
    S = 3
    hl = head_len(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    cov = covered_individuals(a, hl)
    E = evidence_tables(a, de.pair_posteriors_exact(a, pt, hl), cov)["c"]

    def fed(table, extended):
        x = gpu_model(name, S, a)
        feed(x, table)
        x.resolve_all()
        x.set_posterior_range(extended)
        return x.map_phase_given(E)

    ref, got = fed(pt, True), fed(scaled(pt, 40), True)
    assert not ref["status"].any() and len({e[0] for e in E}) >= 2
    same(got, ref)
    reg = fed(pt, False)  # and the regular range on the unscaled table: the same pairs
    assert not reg["status"].any() and reg["hap"].tobytes() == ref["hap"].tobytes()


def test_errors_and_empty_calls():
    a = build_panel("a3")
    N, _, L = a.shape
    m = gpu_model("a3", 3, a)
    m.find_patterns()
    with pytest.raises(HMCError) as ei:
        m.map_phase_given([])
    assert ei.value.code == -1 and "E-step" in str(ei.value)  # HMC_EARG: no E-step yet
    m.resolve_all()
    het = {i: ee.het_loci(a[i]) for i in range(N)}
    i4 = next(i for i in range(N) if len(het[i]) >= 4)
    h = het[i4]
    f = lambda i, k: int(a[i, 0, k])  # noqa: E731
    ihom, khom = next((i, k) for i in range(N) for k in range(L) if a[i, 0, k] >= 0 and a[i, 0, k] == a[i, 1, k])
    imis, kmis = next((i, k) for i in range(N) for k in range(L) if (a[i, :, k] < 0).any())
    good = [(i4, h[0], 7, f(i4, h[0])), (i4, h[1], 7, f(i4, h[1]))]
    assert m.map_phase_given(good)["status"][i4] == 0
    bad = {
        "outside the panel": ((N, 0, 0, 0), f"individual {N} "),
        "locus": ((i4, L, 7, 0), f"locus {L} "),
        "homozygous": ((ihom, khom, 0, int(a[ihom, 0, khom])), f"locus {khom} of individual {ihom} is not heterozygous"),
        "missing": ((imis, kmis, 0, int(a[imis, :, kmis].max())), f"locus {kmis} of individual {imis} is not heterozygous"),
        "neither allele": ((i4, h[2], 7, 9999), "allele 9999 is neither"),
        "duplicate": ((i4, h[0], 8, f(i4, h[0])), "has an earlier entry"),
    }
    for what, (entry, text) in bad.items():
        with pytest.raises(HMCError) as ei:
            m.map_phase_given(good + [entry] + [(-1, 0, 0, 0)])
        assert ei.value.code == -1 and "evidence entry 2:" in str(ei.value) and text in str(ei.value), (what, str(ei.value))
    inter = [(i4, h[0], 1, f(i4, h[0])), (i4, h[2], 1, f(i4, h[2])), (i4, h[1], 2, f(i4, h[1])), (i4, h[3], 2, f(i4, h[3]))]
    with pytest.raises(HMCError) as ei:
        m.map_phase_given(inter)
    assert ei.value.code == -4 and f"individual {i4}:" in str(ei.value) and "interleave" in str(ei.value)
    others = [i for i in range(N) if i != i4]
    assert not m.map_phase_given(inter, others)["evidence"].tolist().count(0.0)  # entries of individuals not asked for are ignored
    with pytest.raises(HMCError) as ei:
        m.map_phase_given(good, [1, N, N + 1])
    assert ei.value.code == -1 and f"individual {N}" in str(ei.value)
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        m.map_phase_given(good)
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.set_shard(2, 6)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.map_phase_given(good, [3, 1])
    assert ei.value.code == -1 and "individual 1 " in str(ei.value)
    out = m.map_phase_given(good, [])  # n = 0
    st = m.given_stats()
    assert out["hap"].shape == (0, 2, L) and out["evidence"].shape == (0,) and st["groups"] == 0 and st["n_constrained"] == 0
    assert st["structure_ms"] == 0 and st["sweep_ms"] == 0
    # every output NULL through the raw call
    assert hmc_amd.lib().hmc_map_phase_given(m._h, 0, None, 0, None, None, None, None, None, None, None, None) == 0
    assert m.given_stats()["groups"] == 1


def test_leaves_the_em_untouched():
    """find_patterns, resolve_all, [map_phase_given], find_patterns,
    resolve_all: the same bits with and without the call."""
    a = build_panel("a4")
    hl = head_len("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.find_patterns()
        _, H, _ = m.resolve_all()
        if call:
            E = evidence_tables(a, de.pair_posteriors_exact(a, m.patterns(), hl), covered_individuals(a, hl))["c"]
            before = (m.estep_results(), m.samples(H), m.switch_posteriors(), m.map_phase())
            assert m.map_phase_given(E)["prob"].all()
            after = (m.estep_results(), m.samples(H), m.switch_posteriors(), m.map_phase())
            assert repr(before) == repr(after)
        m.find_patterns()
        pt = m.patterns()
        ll, H2, re = m.resolve_all()
        return repr((pt, ll, H2, re, m.samples(H2), m.estep_results(), m.resolutions()))

    with np.printoptions(threshold=1 << 30, floatmode="unique"):
        assert chain(True) == chain(False)


def parse_given_file(path, L):
    lines = open(path).read().splitlines()
    assert lines[0] == "Id\tStatus\tPosterior\tEvidence" and (len(lines) - 1) % 3 == 0
    ids, status, prob, evid, hap = [], [], [], [], []
    for q in range(1, len(lines), 3):
        f = lines[q].split("\t")
        assert len(f) == 4
        ids.append(f[0]), status.append(int(f[1])), prob.append(float(f[2])), evid.append(float(f[3]))
        hap.append([[ord(c) for c in lines[q + 1 + side].split(" ")] for side in range(2)])
    return ids, np.array(status, np.int32), np.array(prob), np.array(evid), np.array(hap, np.int32).reshape(-1, 2, L)


def test_cli_output_map_given(tmp_path):
    """hmc_resolve --output-map-given FILE --evidence EVFILE on a3 as a PHASE
    file writes what write_map_phase_given writes, and the file parses back to
    map_phase_given()'s arrays; the phased output is byte-identical to a run
    without the option; a malformed evidence file names its line."""
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
    E = mosaic_evidence(a, m.resolutions(), keep=lambda i: i % 2 == 0)
    assert len(effective(E)) >= 2
    idf = tmp_path / "ids.tsv"  # the ids the writers use; a PHASE file names its markers M1 .. ML
    m.write_map_phase(str(idf))
    ids = parse_map_file(idf, L)[0]
    evf = tmp_path / "ev.tsv"
    with open(evf, "w") as fp:
        fp.write("# Id\tMarker\tSet\tAllele\n\n")
        for i, k, s, f in E:
            fp.write(f"{ids[i]}\tM{k + 1}\t{s}\t{chr(f)}\n")
    dst = tmp_path / "given.tsv"
    r = subprocess.run([CLI, "--output-map-given", str(dst), "--evidence", str(evf), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a3.inp.reconstructed").read_bytes() == plain
    out = m.map_phase_given(E)
    own = tmp_path / "own.tsv"
    m.write_map_phase_given(str(own), E)
    assert own.read_text().splitlines() == dst.read_text().splitlines()
    assert own.read_bytes() == dst.read_bytes()
    fids, status, prob, evid, hap = parse_given_file(dst, L)
    assert fids == ids and np.array_equal(status, out["status"])
    assert prob.tobytes() == out["prob"].tobytes() and evid.tobytes() == out["evidence"].tobytes() and hap.tobytes() == out["hap"].tobytes()
    assert (evid[sorted(effective(E))] < 1).any() and (evid[[i for i in range(N) if i not in effective(E)]] == 1).all()
    with open(evf, "a") as fp:
        fp.write(f"{ids[0]}\tno-such-marker\t0\tA\n")
    r = subprocess.run([CLI, "--output-map-given", str(dst), "--evidence", str(evf), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and f"evidence file line {len(E) + 3}:" in r.stderr, r.stderr
    r = subprocess.run([CLI, "--output-map-given", str(dst), str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--evidence" in r.stderr and "Usage" in r.stderr, r.stderr
