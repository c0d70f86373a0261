"""hmc_map_phase (exact_query.hip exact_map_phase) on the GPU: the most probable
haplotype pair and its exact posterior, against exhaustive enumeration
(tests/map_enumeration.py), against the E-step's k-best beam and the posterior
draws, and against itself across everything the result must not depend on.

Bounds, u = 2^-53, L loci, gamma(k) = k u / (1 - k u):
  the pair   its exact posterior e_c >= e* (1 - g) / (1 + g), g = gamma(2L + 2)
        (map_enumeration: the sweep's choice is a maximum of computed path
        values of at most 2L + 2 roundings each);
  prob       within gamma(4L + 5 + M) of e_c (test_gpu_posterior_draws.draw_k:
        the same computation as a draw's prob);
  prob against another computed value of a pair on the same divisor (the
        beam's best prior, a draw's prob): both numerators are products of at
        most 2L + 2 roundings, in different association, the sweep maximises
        a third such product, and each quotient is rounded once:
        prob >= other (1 - gamma(4L + 6)), written as other <= prob (1 + gamma(4L + 6))
        for the draws (BEAM_K).
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
import map_enumeration as me
from test_enumeration_oracle import build_panel, head_len
from test_gpu_enumeration import feed, gpu_model
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, ETA, MIXED_L, mixed_panel, mosaic_with_heads
from test_gpu_posterior_draws import PANEL_S, SEED, ValueMismatch, check_genotype, draw_k, large_model
from test_scaled_tables import scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
D_MOSAIC = 4096
# the draws' seven cases, on none of which the beam misses the maximiser, and the one found on the CPU where it
# does (tests/test_map_enumeration.py): "hom" with one state kept per locus, individuals 1 and 2
MAP_PANEL_S = PANEL_S + [("hom", 1)]
BEAM_MISSES = {("hom", 1): 2}
_cache = {}


def BEAM_K(L):
    return 4 * L + 6


def syms_of(a):
    ta = en.allele_table(a)
    return ta, [[s for s, f in ta[k] if f > 0] for k in range(a.shape[2])]


def check_map(m, a, pt, hl):
    """map_phase of every individual against enumeration; returns statistics."""
    N, _, L = a.shape
    out = m.map_phase()
    assert out["hap"].shape == (N, 2, L) and out["prob"].shape == (N,) and not out["status"].any()
    ta, syms = syms_of(a)
    exact = me.map_pairs_exact(a, pt, hl)
    quirk = en.head_quirk(a, hl)
    res = m.resolutions()
    g_pair = en.gamma(me.map_roundings(L))
    worst, loosest, differs, ratio, not_argmax = 0.0, Fraction(0), 0, Fraction(1), 0
    for i in range(N):
        check_genotype(out["hap"][i][None], a[i], syms, hl if quirk[i] else 0)
        if quirk[i]:  # the head pairing is no phasing model: genotype consistency only
            continue
        e = exact[i]
        key = de.pair_key(out["hap"][i, 0], out["hap"][i, 1])
        e_c = e["post"].get(key, 0)
        assert me.accepts(e_c, e["best"], L), (i, key, float(e_c), float(e["best"]))
        not_argmax += key not in e["argmax"]
        g = en.gamma(draw_k(L, en.phasing_count(a[i], ta)))
        assert g <= 1e-12
        loosest = max(loosest, g)
        p = float(out["prob"][i])
        if not en.within(p, e_c, g):
            raise ValueMismatch((i, key, en.relerr(p, e_c)))
        worst = max(worst, en.relerr(p, e_c))
        rkey = de.pair_key(res[i, 0], res[i, 1])
        e_r = e["post"].get(rkey, 0)
        assert e_r > 0
        if rkey != key:
            differs += 1
        ratio = max(ratio, e["best"] / e_r)
    return dict(pair_bound=float((1 - g_pair) / (1 + g_pair)), prob_bound=float(loosest), worst_u=worst / float(en.U),
                map_differs_from_resolutions=differs, largest_ratio=float(ratio), returned_not_an_exact_maximiser=not_argmax,
                stats=m.map_stats())


def check_never_worse_than_the_beam(m, out):
    """prob >= (the largest prior of the E-step's list / total) (1 - gamma(BEAM_K)), in exact arithmetic."""
    er = m.estep_results()
    L = m.L
    g = en.gamma(BEAM_K(L))
    n = 0
    for i in np.nonzero(out["status"] == 0)[0]:
        nc = int(er["ncand"][i])
        if nc == 0:
            continue
        beam = Fraction(float(er["prior"][i, :nc].max())) / Fraction(float(er["total"][i]))
        assert Fraction(float(out["prob"][i])) >= beam * (1 - g), (int(i), float(out["prob"][i]), float(beam))
        n += 1
    return n


@pytest.mark.parametrize("name,S", MAP_PANEL_S)
def test_against_enumeration(name, S):
    """The returned pair passes map_enumeration.accepts, prob is within the
    draws' bound of the pair's enumerated posterior, and prob is never below
    the beam's best.  Prints the bounds used, the worst relative error of prob
    in units of u and how often the MAP pair differs from resolutions().  On
    none of the draws' seven cases does the beam miss the maximiser (found on
    the CPU with the enumerator and the restatement, tests/
    test_map_enumeration.py), so there only >= 0 holds; ("hom", 1) is added
    because there it misses two individuals, and the count is asserted."""
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    st = check_map(m, a, pt, hl)
    st["beam_comparisons"] = check_never_worse_than_the_beam(m, m.map_phase())
    print(name, S, st)
    assert st["map_differs_from_resolutions"] >= BEAM_MISSES.get((name, S), 0)
    if (name, S) in BEAM_MISSES:
        assert st["largest_ratio"] > 1.5
    assert st["beam_comparisons"] >= a.shape[0] - 1


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
        check_map(m2, a, pt, 1)
    assert 0 < ei.value.args[0][2] < 1e-8  # the size of the perturbation


def mosaic():
    if "mosaic" not in _cache:
        N, L = BITS_SHAPE
        a = mosaic_with_heads(N, L, 3, 0.05, 7)
        m = large_model(a)
        _cache["mosaic"] = (a, m, m.map_phase(), m.map_stats())
    return _cache["mosaic"]


def same(x, y, rows_x=slice(None), rows_y=slice(None)):
    for k in ("hap", "prob", "status"):
        assert np.ascontiguousarray(x[k][rows_x]).tobytes() == np.ascontiguousarray(y[k][rows_y]).tobytes(), k


def test_mosaic_against_the_beam_and_the_draws():
    """The 60 x 120 mosaic (frontiers of several hundred states: more states
    than threads, several wavefronts in the final reduction): never below the
    beam's best, no draw of 4 096 more probable than the MAP pair, and the
    draws hit the MAP pair as often as its prob says."""
    a, m, out, stats = mosaic()
    N, L = BITS_SHAPE
    assert int(m.frontier_max().max()) > 256 and stats["groups"] == 1 and not out["status"].any()
    _, syms = syms_of(a)
    for i in range(N):
        check_genotype(out["hap"][i][None], a[i], syms)
    assert (out["prob"] > 0).all() and (out["prob"] <= 1 + 1e-12).all()
    assert check_never_worse_than_the_beam(m, out) == N
    dr = m.posterior_draws(D_MOSAIC, SEED)
    assert not dr["status"].any()
    g = en.gamma(BEAM_K(L))
    hits, comparisons = [], 0
    for i in range(N):
        top = Fraction(float(out["prob"][i])) * (1 + g)
        assert Fraction(float(dr["prob"][i].max())) <= top, (i, float(dr["prob"][i].max()), float(out["prob"][i]))
        h = dr["hap"][i]
        mp = out["hap"][i]
        eq = ((h == mp[None]).all(axis=(1, 2)) | (h == mp[None, ::-1]).all(axis=(1, 2)))
        p = float(out["prob"][i])
        # (a draw equal to the MAP pair carries the MAP pair's posterior)
        assert all(en.within(float(x), Fraction(p), en.gamma(2 * BEAM_K(L))) for x in np.unique(dr["prob"][i][eq]))
        comparisons += de.check_frequencies({"map": int(eq.sum()), "other": D_MOSAIC - int(eq.sum())}, D_MOSAIC,
                                            {"map": min(p, 1.0), "other": max(1.0 - p, 0.0)})
        hits.append(int(eq.sum()))
    res = m.resolutions()
    differs = sum(de.pair_key(res[i, 0], res[i, 1]) != de.pair_key(out["hap"][i, 0], out["hap"][i, 1]) for i in range(N))
    print("mosaic: MAP differs from resolutions() for", differs, "of", N, "; prob min / median", float(out["prob"].min()),
          float(np.median(out["prob"])), "; draws equal to the MAP pair (min, max of", D_MOSAIC, ")", min(hits), max(hits),
          "; frequency comparisons", comparisons, stats)


def test_determinism_small():
    name, S = "a3", 3
    a = build_panel(name)

    def model(windowed=False):
        m = gpu_model(name, S, a)
        if windowed:
            m.set_estep_windows("always", 3)
        m.find_patterns()
        m.resolve_all()
        return m

    m = model()
    full = m.map_phase()
    same(full, m.map_phase())  # two calls
    pick = [7, 2, 2, 9, 0, 7]  # a subset, permuted, with repeats
    same(m.map_phase(pick), full, rows_y=pick)
    m.posterior_draws(64, SEED)  # another call of the family in between
    same(m.map_phase(), full)
    m.set_shard(3, 8)
    m.resolve_all()
    same(m.map_phase(), full, rows_y=slice(3, 8))
    same(m.map_phase([7, 3]), full, rows_y=[7, 3])
    mw = model(windowed=True)  # a windowed E-step before the call
    assert mw.estep_windows()["windows"] == -(-a.shape[2] // 3)
    same(mw.map_phase(), full)


def test_determinism_large():
    """The mosaic: forced groups, a shard and a permuted subset with repeats give the bytes of the one-group run."""
    a, m, ref, _ = mosaic()
    same(m.map_phase(), ref)
    pick = [59, 0, 31, 31, 7, 59]
    same(m.map_phase(pick), ref, rows_y=pick)
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = m2.map_phase()
    print(m2.map_stats())
    assert m2.map_stats()["groups"] >= 2
    same(got, ref)
    m3 = large_model(a, shard=(20, 40))
    same(m3.map_phase(), ref, rows_y=slice(20, 40))


def close(x, y, g, absolute=Fraction(0)):
    x, y = Fraction(float(x)), Fraction(float(y))
    return abs(x - y) <= 2 * g * max(x, y) / (1 - g) + absolute


def test_statuses_and_extended_range():
    """The mixed panel (1 200 loci): statuses 1 and 2 exactly where the draws
    report them, those rows the input genotype at prob 0.  Extended range: no
    status 2; where both ranges give status 0 the haplotypes are the same
    bytes and prob agrees within the sum of the two bounds.
    Bound of one range's prob: the numerator 2L + 2 roundings, the division 1,
    the divisor a sum of positive terms over the lattice — per record a
    state's product (1), the sum of its contributions in any order (fewer than
    F, the largest frontier), and the final sum over at most F states:
    (L + 2)(F + 2) — together gamma(2L + 3 + (L + 2)(F + 2)).  Underflow, in
    the regular range only: each of the numerator's 2L + 2 operations may add
    ETA / 2 absolute, the quotient ETA / 2 more, and the E-step's total is off
    by at most (6 L F^2 + F) ETA relative to itself (test_gpu_posteriors.
    check_rows_sum_to_one): ((L + 2) + prob (6 L F^2 + F)) ETA / total."""
    a = mixed_panel(MIXED_L)
    L = a.shape[2]
    m = large_model(a)
    dr = m.posterior_draws(1, SEED)
    reg = m.map_phase()
    assert np.array_equal(reg["status"], dr["status"])
    assert (reg["status"] == 1).sum() >= 1 and (reg["status"] == 2).sum() >= 1 and (reg["status"] == 0).sum() >= 4
    _, syms = syms_of(a)
    for i in range(a.shape[0]):
        if reg["status"][i] != 0:
            assert (reg["hap"][i] == a[i]).all() and reg["prob"][i] == 0
        else:
            check_genotype(reg["hap"][i][None], a[i], syms)
            assert 0 < reg["prob"][i] <= 1 + 1e-9
    reg_stats = m.map_stats()
    m.set_posterior_range(True)
    ext = m.map_phase()
    ext_dr = m.posterior_draws(1, SEED)
    assert np.array_equal(ext["status"], ext_dr["status"]) and not (ext["status"] == 2).any()
    assert m.map_stats()["n_pruned"] == 0
    both = np.nonzero((reg["status"] == 0) & (ext["status"] == 0))[0]
    assert len(both) >= 4
    F = int(m.frontier_max().max())
    g = en.gamma(2 * L + 3 + (L + 2) * (F + 2))
    total = m.estep_results()["total"]
    for i in both:
        assert reg["hap"][i].tobytes() == ext["hap"][i].tobytes(), i
        slack = (Fraction(L + 2) + Fraction(float(reg["prob"][i])) * (6 * L * F * F + F)) * ETA / Fraction(float(total[i]))
        assert close(reg["prob"][i], ext["prob"][i], g, slack), (i, reg["prob"][i], ext["prob"][i])
    for i in np.nonzero(ext["status"] == 0)[0]:
        check_genotype(ext["hap"][i][None], a[i], syms)
    m.set_posterior_range(False)
    same(m.map_phase(), reg)
    print("regular", reg["status"].tolist(), reg_stats, "extended", ext["status"].tolist(), m.map_stats(), "bound", float(g))


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
        return x.map_phase()

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
        m.map_phase()
    assert ei.value.code == -1 and "E-step" in str(ei.value)  # HMC_EARG: no E-step yet
    m.resolve_all()
    assert m.map_phase()["hap"].shape == (10, 2, L)
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        m.map_phase()
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    feed(m, pt)  # set_patterns after the E-step
    with pytest.raises(HMCError) as ei:
        m.map_phase()
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.map_phase([1, 10, 11])
    assert ei.value.code == -1 and "individual 10" in str(ei.value)
    m.set_shard(2, 6)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.map_phase([3, 1])
    assert ei.value.code == -1 and "individual 1 " in str(ei.value)
    out = m.map_phase([])  # n = 0
    assert out["hap"].shape == (0, 2, L) and out["prob"].shape == (0,) and m.map_stats()["groups"] == 0
    # every output NULL through the raw call
    assert hmc_amd.lib().hmc_map_phase(m._h, 0, None, None, None, None) == 0
    assert m.map_stats()["groups"] == 1


def test_leaves_the_em_untouched():
    """find_patterns, resolve_all, [map_phase], find_patterns, resolve_all:
    the same bits with and without the call."""
    a = build_panel("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.find_patterns()
        _, H, _ = m.resolve_all()
        if call:
            before = (m.estep_results(), m.samples(H), m.switch_posteriors())
            assert m.map_phase()["prob"].all()
            after = (m.estep_results(), m.samples(H), m.switch_posteriors())
            assert repr(before) == repr(after)
        m.find_patterns()
        pt = m.patterns()
        ll, H2, re = m.resolve_all()
        return repr((pt, ll, H2, re, m.samples(H2), m.estep_results(), m.resolutions()))

    with np.printoptions(threshold=1 << 30, floatmode="unique"):
        assert chain(True) == chain(False)


def parse_map_file(path, L):
    lines = open(path).read().splitlines()
    assert lines[0] == "Id\tStatus\tPosterior" and (len(lines) - 1) % 3 == 0
    ids, status, prob, hap = [], [], [], []
    for q in range(1, len(lines), 3):
        f = lines[q].split("\t")
        assert len(f) == 3
        ids.append(f[0]), status.append(int(f[1])), prob.append(float(f[2]))
        hap.append([[ord(c) for c in lines[q + 1 + side].split(" ")] for side in range(2)])
    return ids, np.array(status, np.int32), np.array(prob), np.array(hap, np.int32).reshape(-1, 2, L)


def test_cli_output_map(tmp_path):
    """hmc_resolve --output-map on a3 as a PHASE file writes what
    write_map_phase writes, and the file parses back to map_phase()'s arrays;
    the phased output is byte-identical to a run without the option."""
    a = build_panel("a3")
    L = a.shape[2]
    src = tmp_path / "a3.inp"
    synth.write_phase(synth.Panel(a, "S" * L), str(src))
    r = subprocess.run([CLI, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "a3.inp.reconstructed").read_bytes()
    dst = tmp_path / "map.tsv"
    r = subprocess.run([CLI, "--output-map", str(dst), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a3.inp.reconstructed").read_bytes() == plain
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    out = m.map_phase()
    own = tmp_path / "own.tsv"
    m.write_map_phase(str(own))
    assert own.read_bytes() == dst.read_bytes()
    ids, status, prob, hap = parse_map_file(dst, L)
    assert len(ids) == a.shape[0]
    assert np.array_equal(status, out["status"]) and prob.tobytes() == out["prob"].tobytes()
    assert hap.tobytes() == out["hap"].tobytes()
    ext = tmp_path / "ext.tsv"
    r = subprocess.run([CLI, "--output-map", str(ext), "--extended-range", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert parse_map_file(ext, L)[3].tobytes() == hap.tobytes()
    r = subprocess.run([CLI, "--output-map"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--output-map" in r.stderr
