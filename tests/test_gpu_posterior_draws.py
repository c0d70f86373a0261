"""hmc_posterior_draws (exact_query.hip exact_posterior_draws) on the GPU: whole
haplotype pairs drawn from the exact posterior, against exhaustive enumeration
(tests/draw_enumeration.py), against the marginals the library already pins
(switch and genotype posteriors) and against itself across everything a draw
must not depend on.

Bound of one `prob` against the enumerated posterior of the pair drawn
(draw_k), u = 2^-53, L loci, M the enumerator's count of ordered phasings of
the individual (enumeration.phasing_count):
  path product   per record (the head record and the L - head_len above it, at
        most L + 1) the state's product of two transition probabilities (one
        rounding) multiplied into the running value (one): at most 2L + 2;
  doubling       exact;
  P(genotype), the divisor   2L + 2 + M (check_estep's total: the same chain
        and sums that merge at most M phasings);
  the division   1.
Together 4L + 5 + M roundings: gamma(4L + 5 + M) relative, at most
gamma(4 * 10 + 5 + 1960) = 2.3e-13 on these panels (asserted <= 1e-12).

The frequencies of the drawn pairs are held with draw_enumeration.
check_frequencies: Bernstein's bound at delta = 1e-12 per comparison, about
2e4 comparisons in this module (printed by the tests), so a correct sampler
fails with probability below 1e-7, once: the seeds are fixed.
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
from test_enumeration_oracle import build_panel, head_len
from test_gpu_enumeration import feed, gpu_model
from test_gpu_posteriors import BITS_BUDGETS, BITS_SHAPE, MIXED_L, mixed_panel, mosaic_with_heads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
D_ENUM, D_LARGE, SEED = 16384, 4096, 20261020
PANEL_S = [("snp", 2), ("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5), ("minlen2", 10)]


class ValueMismatch(AssertionError):
    """prob of a draw is outside its bound of the enumerated posterior of the pair."""


def draw_k(L, M):
    return 4 * L + 5 + M


def check_genotype(hap, g, syms, quirk_below=0):
    """Every draw hap[D, 2, L] is a phasing of genotype g[2, L]: known alleles
    reproduced as an unordered pair per locus, missing ones filled from the
    locus's alleles of positive frequency.  quirk_below = head_len for an
    individual with a missing allele at a head locus: the reference's head
    pairing (enumeration.HEAD_QUIRK) includes pairs that are no phasings of
    the genotype at the head loci, and the draws follow it, so below head_len
    only the allele table is held for such an individual."""
    lo, hi = hap.min(axis=1), hap.max(axis=1)
    for k in range(g.shape[1]):
        x, y = int(g[0, k]), int(g[1, k])
        ok = np.isin(hap[:, :, k], syms[k]).all(axis=1)
        if k < quirk_below:
            pass
        elif x >= 0 and y >= 0:
            ok &= (lo[:, k] == min(x, y)) & (hi[:, k] == max(x, y))
        elif x >= 0 or y >= 0:
            ok &= (hap[:, :, k] == max(x, y)).any(axis=1)
        assert ok.all(), (k, x, y, hap[~ok][0].tolist())


def pair_counts(hap):
    """{unordered pair: (count, draws that gave it)} of hap[D, 2, L]."""
    D, _, L = hap.shape
    swap = np.zeros(D, bool)  # order the two haplotypes of every draw lexicographically
    undecided = np.ones(D, bool)
    for k in range(L):
        swap |= undecided & (hap[:, 0, k] > hap[:, 1, k])
        undecided &= hap[:, 0, k] == hap[:, 1, k]
    keyed = np.where(swap[:, None, None], hap[:, ::-1], hap).reshape(D, 2 * L)
    uniq, inv = np.unique(keyed, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return {(tuple(int(v) for v in u[:L]), tuple(int(v) for v in u[L:])): np.nonzero(inv == j)[0] for j, u in enumerate(uniq)}


def check_draws(m, a, pt, hl, require_mixed=True):
    """Draws of every individual against enumeration; returns statistics."""
    N, _, L = a.shape
    out = m.posterior_draws(D_ENUM, SEED)
    assert out["hap"].shape == (N, D_ENUM, 2, L) and out["prob"].shape == (N, D_ENUM) and not out["status"].any()
    ta = en.allele_table(a)
    syms = [[s for s, f in ta[k] if f > 0] for k in range(L)]
    exact = de.pair_posteriors_exact(a, pt, hl)
    quirk = en.head_quirk(a, hl)
    assert quirk.sum() <= 1 and quirk.sum() <= N / 4
    mixed = de.mixed_individuals(exact)
    if require_mixed:
        assert len(mixed) >= 1  # the statistical part is not vacuous
    worst, loosest, compared, distinct = 0.0, Fraction(0), 0, 0
    for i in range(N):
        check_genotype(out["hap"][i], a[i], syms, hl if quirk[i] else 0)
        if quirk[i]:  # the head pairing is no phasing model: genotype consistency only
            continue
        g = en.gamma(draw_k(L, en.phasing_count(a[i], ta)))
        assert g <= 1e-12
        loosest = max(loosest, g)
        pc = pair_counts(out["hap"][i])
        for key, where in pc.items():
            e = exact[i].get(key, 0)
            assert e > 0, (i, key)
            for p in np.unique(out["prob"][i, where]):
                if not en.within(float(p), e, g):
                    raise ValueMismatch((i, key, en.relerr(float(p), e)))
                worst = max(worst, en.relerr(float(p), e))
        compared += de.check_frequencies({k: len(w) for k, w in pc.items()}, D_ENUM, exact[i])
        distinct += len(pc)
    return dict(worst_u=worst / float(en.U), loosest_bound=float(loosest), comparisons=compared, distinct_pairs=distinct,
                mixed=mixed, stats=m.draw_stats())


@pytest.mark.parametrize("name,S", PANEL_S)
def test_against_enumeration(name, S):
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    hl = head_len(name)
    assert m.head_len() == hl
    pt = m.patterns()
    m.resolve_all()
    print(name, S, check_draws(m, a, pt, hl))


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
        check_draws(m2, a, pt, 1)
    assert 0 < ei.value.args[0][2] < 1e-8  # the size of the perturbation


def a3_model(windowed=False):
    a = build_panel("a3")
    m = gpu_model("a3", 3, a)
    if windowed:
        m.set_estep_windows("always", 3)
    m.find_patterns()
    pt = m.patterns()
    m.resolve_all()
    return a, m, pt


def same(x, y, rows_x=slice(None), rows_y=slice(None)):
    for k in ("hap", "prob", "status"):
        assert np.ascontiguousarray(x[k][rows_x]).tobytes() == np.ascontiguousarray(y[k][rows_y]).tobytes(), k


def test_determinism_and_independence_small():
    a, m, pt = a3_model()
    N = a.shape[0]
    big = m.posterior_draws(8192, SEED)
    same(big, m.posterior_draws(8192, SEED))  # two calls
    few = m.posterior_draws(8, SEED)
    for k in ("hap", "prob"):  # draw d of 8 is draw d of 8 192
        assert few[k].tobytes() == np.ascontiguousarray(big[k][:, :8]).tobytes(), k
    pick = [7, 2, 2, 9, 0, 7]  # a subset, permuted, with repeats
    sub = m.posterior_draws(8192, SEED, pick)
    same(sub, big, rows_y=pick)
    # the prefix sums in device memory, the backward half of exact_fb run as well
    for chunks, fwd in ((0, True), (0, False), (-1, False)):
        m.set_draw_tuning(chunks, fwd)
        same(m.posterior_draws(8192, SEED), big)
    m.set_draw_tuning()
    m.set_shard(3, 8)
    m.resolve_all()
    part = m.posterior_draws(8192, SEED)
    same(part, big, rows_y=slice(3, 8))
    same(m.posterior_draws(8192, SEED, [7, 3]), big, rows_y=[7, 3])
    _, mw, _ = a3_model(windowed=True)  # a windowed E-step before the call
    assert mw.estep_windows()["windows"] == -(-a.shape[2] // 3)
    same(mw.posterior_draws(8192, SEED), big)
    # another seed: other draws wherever the posterior is mixed
    other = a3_model()[1].posterior_draws(8192, SEED + 1)
    mixed = de.mixed_individuals(de.pair_posteriors_exact(a, pt, 1))
    assert mixed and all(other["hap"][i].tobytes() != big["hap"][i].tobytes() for i in mixed)
    assert N == 10


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


def check_marginals(m, a, out, D):
    """The draws' one- and two-locus marginals against hmc_switch_posteriors
    (fraction of draws that are cis at every site) and hmc_genotype_posteriors
    (fraction per bin at every missing-allele site)."""
    i0 = getattr(m, "i0", 0)
    num, sym, _ = m.allele_table()
    sw, gp = m.switch_posteriors(), m.genotype_posteriors()
    n = 0
    for q in np.nonzero(sw["status"] == 0)[0]:
        i, x, y = int(sw["indiv"][q]) - i0, int(sw["locus_a"][q]), int(sw["locus_b"][q])
        h = out["hap"][i]
        cis = int(((h[:, 0, x] < h[:, 1, x]) == (h[:, 0, y] < h[:, 1, y])).sum())
        n += de.check_frequencies({"cis": cis, "trans": D - cis}, D, {"cis": float(sw["post"][q, 0]), "trans": float(sw["post"][q, 1])})
    pairs = gp["pairs"].tolist()
    for q in np.nonzero(gp["status"] == 0)[0]:
        i, k = int(gp["indiv"][q]) - i0, int(gp["locus"][q])
        h = out["hap"][i][:, :, k]
        idx = np.searchsorted(sym[k, :num[k]], h)  # symbols ascending: the allele table's index
        assert (sym[k, :num[k]][idx] == h).all()
        lo, hi = idx.min(axis=1), idx.max(axis=1)
        bins = hi * (hi + 1) // 2 + lo
        cnt = np.bincount(bins, minlength=len(pairs))
        n += de.check_frequencies({b: int(c) for b, c in enumerate(cnt)}, D, {b: float(p) for b, p in enumerate(gp["post"][q])})
    return dict(switch_sites=int((sw["status"] == 0).sum()), missing_sites=int((gp["status"] == 0).sum()), comparisons=n)


def test_large_panel_marginals_and_paths():
    """The 60 x 120 mosaic (frontiers of up to 890 states: several chunks in
    the final record): marginals of 4 096 draws against the pinned posteriors;
    one group, forced groups and a shard give the same bits."""
    N, L = BITS_SHAPE
    a = mosaic_with_heads(N, L, 3, 0.05, 7)
    m = large_model(a)
    assert int(m.frontier_max().max()) > 256
    ref = m.posterior_draws(D_LARGE, SEED)
    s1 = m.draw_stats()
    assert s1["groups"] == 1 and not ref["status"].any()
    ta = en.allele_table(a)
    syms = [[s for s, f in ta[k] if f > 0] for k in range(L)]
    for i in range(N):
        check_genotype(ref["hap"][i], a[i], syms)
    assert (ref["prob"] > 0).all() and (ref["prob"] <= 1 + 1e-12).all()
    print(check_marginals(m, a, ref, D_LARGE), s1)
    m2 = large_model(a, budgets=BITS_BUDGETS)
    got = m2.posterior_draws(D_LARGE, SEED)
    print(m2.draw_stats())
    assert m2.draw_stats()["groups"] >= 2
    same(got, ref)
    m3 = large_model(a, shard=(20, 40))
    same(m3.posterior_draws(D_LARGE, SEED), ref, rows_y=slice(20, 40))
    m.set_draw_tuning(0, False)
    same(m.posterior_draws(D_LARGE, SEED), ref)


def test_unresolved_and_subnormal_individuals():
    """The mixed panel of test_resolved_next_to_unresolved (1 200 loci):
    unresolved individuals (status 1) and the one whose P(genotype) is below
    DBL_MIN (status 2) carry the input genotype in every draw and prob 0; the
    others' draws pass the marginal checks."""
    a = mixed_panel(MIXED_L)
    m = large_model(a)
    er = m.estep_results()
    st, total = er["status"], er["total"]
    out = m.posterior_draws(D_LARGE, SEED)
    resolved = (st == 0) & (total > 0)
    assert np.array_equal(out["status"] == 1, ~resolved)
    assert np.array_equal(out["status"] == 2, resolved & (total < 2.0 ** -1022))
    assert (out["status"] == 1).sum() >= 1 and (out["status"] == 2).sum() >= 1 and (out["status"] == 0).sum() >= 4
    ta = en.allele_table(a)
    syms = [[s for s, f in ta[k] if f > 0] for k in range(a.shape[2])]
    for i in range(a.shape[0]):
        if out["status"][i] != 0:
            assert (out["hap"][i] == a[i][None]).all() and not out["prob"][i].any()
        else:
            check_genotype(out["hap"][i], a[i], syms)
            assert (out["prob"][i] >= 0).all()
    print(out["status"].tolist(), check_marginals(m, a, out, D_LARGE), m.draw_stats())


def test_errors_and_empty_calls():
    a = build_panel("a3")
    m = gpu_model("a3", 3, a)
    m.find_patterns()
    pt = m.patterns()
    with pytest.raises(HMCError) as ei:
        m.posterior_draws(4, 0)
    assert ei.value.code == -1 and "E-step" in str(ei.value)  # HMC_EARG: no E-step yet
    m.resolve_all()
    assert m.posterior_draws(4, 0)["hap"].shape == (10, 4, 2, a.shape[2])
    m.find_patterns()  # an M-step: P(genotype) of that E-step no longer belongs to the table
    with pytest.raises(HMCError) as ei:
        m.posterior_draws(4, 0)
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    m.posterior_draws(4, 0)
    feed(m, pt)  # set_patterns after the E-step
    with pytest.raises(HMCError) as ei:
        m.posterior_draws(4, 0)
    assert ei.value.code == -1 and "model changed" in str(ei.value)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.posterior_draws(0, 0)
    assert ei.value.code == -1 and "draws = 0" in str(ei.value)
    with pytest.raises(HMCError) as ei:
        m.posterior_draws(4, 0, [1, 10, 11])
    assert ei.value.code == -1 and "individual 10" in str(ei.value)
    m.set_shard(2, 6)
    m.resolve_all()
    with pytest.raises(HMCError) as ei:
        m.posterior_draws(4, 0, [3, 1])
    assert ei.value.code == -1 and "individual 1 " in str(ei.value)
    out = m.posterior_draws(4, 0, [])  # n = 0
    assert out["hap"].shape == (0, 4, 2, a.shape[2]) and m.draw_stats()["groups"] == 0
    with pytest.raises(HMCError):
        m.set_draw_tuning(2000, True)


def test_leaves_the_em_untouched():
    """find_patterns, resolve_all, [posterior_draws], find_patterns,
    resolve_all: the same bits with and without the call."""
    a = build_panel("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.find_patterns()
        _, H, _ = m.resolve_all()
        if call:
            before = (m.estep_results(), m.samples(H), m.switch_posteriors())
            assert m.posterior_draws(64, 5)["prob"].all()
            after = (m.estep_results(), m.samples(H), m.switch_posteriors())
            assert repr(before) == repr(after)
        m.find_patterns()
        pt = m.patterns()
        ll, H2, re = m.resolve_all()
        return repr((pt, ll, H2, re, m.samples(H2), m.estep_results(), m.resolutions()))

    with np.printoptions(threshold=1 << 30, floatmode="unique"):
        assert chain(True) == chain(False)


def test_cli_output_draws(tmp_path):
    """hmc_resolve --output-draws on a3 as a PHASE file: one line per
    individual and draw, the numbers read back to the API's doubles, the
    haplotypes are the API's symbols; the phased output is byte-identical to a
    run without the option; --draws without --output-draws is a usage error."""
    a = build_panel("a3")
    src = tmp_path / "a3.inp"
    synth.write_phase(synth.Panel(a, "S" * a.shape[2]), str(src))
    r = subprocess.run([CLI, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "a3.inp.reconstructed").read_bytes()
    dst = tmp_path / "draws.tsv"
    r = subprocess.run([CLI, "--output-draws", str(dst), "--draws", "7", "--seed", "99", str(src)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a3.inp.reconstructed").read_bytes() == plain
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    out = m.posterior_draws(7, 99)
    lines = dst.read_text().splitlines()
    assert lines[0] == "Id\tDraw\tPosterior\tHaplotype0\tHaplotype1"
    assert not out["status"].any() and len(lines) - 1 == a.shape[0] * 7
    for n, ln in enumerate(lines[1:]):
        i, d = divmod(n, 7)
        f = ln.split("\t")
        assert len(f) == 5 and f[0].lstrip("#") == str(i + 1) and int(f[1]) == d
        assert float(f[2]) == float(out["prob"][i, d])
        for side in range(2):
            assert [ord(c) for c in f[3 + side].split(" ")] == out["hap"][i, d, side].tolist()
    r = subprocess.run([CLI, "--output-draws", str(dst), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(dst.read_text().splitlines()) - 1 == a.shape[0] * 100  # the default D
    for args in (["--draws", "5"], ["--seed", "1"], ["--output-draws", str(dst), "--draws", "0"]):
        r = subprocess.run([CLI, *args, str(src)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--output-draws" in r.stderr and "Usage" in r.stderr, r.stderr
