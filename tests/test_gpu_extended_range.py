"""Extended-range posteriors (hmc_set_posterior_range, hmc_genotype_likelihoods)
on the GPU: exact_fb's scaled pass and the four consumers that cancel its
exponents, against exhaustive enumeration where the panel is small and against
themselves and the regular mode where it is not.

Underflow at enumerable sizes comes from scaled tables (tests/
test_scaled_tables.py, which asserts the trick without a GPU): every freq and
tp times 2^-c multiplies every phasing's prior by 2^(-2 c L) and leaves every
posterior as it is, so the enumeration of the unscaled table is the reference
and the existing bounds hold unchanged — a power of two adds no rounding:
  genotype, switch and pair posteriors   gamma(6L + 4M + 14)  (test_gpu_posteriors.posterior_k,
                                          test_gpu_switch_posteriors.switch_k)
  prob of a draw                          gamma(4L + 5 + M)    (test_gpu_posterior_draws.draw_k)
  genotype_likelihoods                    gamma(2L + 2 + M)    (enumeration.check_estep's total),
                                          compared as exact rationals, mantissa x 2^exponent
                                          against the enumerated total of the scaled table.
Regular against extended on one table: both are within g of the exact value e,
so |x - y| <= 2 g e <= 2 g y / (1 - g): "within the sum of the two bounds".

What the regular mode does with the scaled tables (measured on the MI355X and
asserted): at ZERO_C every site, query and individual has status 1; at
SUBNORMAL_C every one has status 2 (no individual's value-pass forward values
hit 0 on the way, so none is unresolved in the E-step).

On the long panels nothing can be enumerated.  There every row must sum to 1
within gamma(rowsum_k) alone — the underflow term of check_rows_sum_to_one is
dropped, nothing underflows in extended range — and a row the regular mode
answers (status 0) must agree with it: each value carries at most
gamma(rowsum_k) relative and, on the regular side, the absolute underflow term
(6 L F^2 + 2F) ETA / P(genotype) of check_rows_sum_to_one, so
|x - y| <= g (x + y) / (1 - g) + (6 L F^2 + 2F) ETA / P(genotype).
No individual of these three panels is expected to have a dead lattice: the M0
table was mined from these very genotypes, so each individual's own phasings
have patterns all along; asserted (no status 1 in extended range).
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hmc_amd
from hmc_amd import synth
from hmc_amd._lib import HMCError, lib

import draw_enumeration as de
import enumeration as en
import pair_enumeration as pe
import switch_enumeration as se
import test_pair_enumeration
import test_switch_enumeration
from test_enumeration_oracle import PANELS, build_panel, head_len, perturbed_tables
from test_gpu_enumeration import feed, gpu_model, gpu_view
from test_gpu_pair_posteriors import SLOTS, ask, check_pairs
from test_gpu_posterior_draws import SEED, check_draws, check_genotype
from test_gpu_posteriors import (BITS_BUDGETS, BITS_SHAPE, DBL_MIN, ETA, MIXED_L, BinMismatch, check_posteriors, exact_sum,
                                 mixed_panel, mosaic_with_heads, posterior_k, rowsum_k)
from test_gpu_switch_posteriors import ValueMismatch, check_switches, switch_k
from test_scaled_tables import INDIVIDUALS, SCALED_PANELS, SUBNORMAL_C, ZERO_C, prior_shift, scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tools", "hmc_resolve")
D_BYTES = 256    # draws per individual where only bytes are compared (draw d does not depend on the number of draws)
D_LONG = 4096    # draws per individual for the marginals on the long panels
LARGE_C = 4      # the 60 x 120 panel: priors times 2^-960, beyond the regular mode
_cache = {}


def mined(name):
    """(panel, its mined table) of an enumerable panel, once."""
    if name not in _cache:
        a = build_panel(name)
        m = gpu_model(name, PANELS[name]["S"][0], a)
        m.find_patterns()
        assert m.head_len() == head_len(name)
        _cache[name] = (a, m.patterns())
    return _cache[name]


def fed(name, pt):
    a, _ = mined(name)
    m = gpu_model(name, PANELS[name]["S"][0], a)
    feed(m, pt)
    m.resolve_all()
    return m


def bundle(m, a, D, queries=None):
    """The four calls and the likelihoods in the model's current range."""
    if queries is None:
        queries = pe.all_pairs(a)
    i0 = getattr(m, "i0", 0)
    out = dict(gp=m.genotype_posteriors(), sw=m.switch_posteriors(), pr=ask(m, queries), dr=m.posterior_draws(D, SEED),
               lk=m.genotype_likelihoods())
    out["n_pruned"] = (m.posterior_stats()["n_pruned"], m.switch_stats()["n_pruned"], m.pair_stats()["n_pruned"],
                       m.draw_stats()["n_pruned"])
    assert i0 == getattr(m, "i0", 0)
    return out


def same_bundles(x, y, what, likelihoods=True):
    for call, keys in (("gp", ("indiv", "locus", "status", "post")), ("sw", ("indiv", "locus_a", "locus_b", "status", "post")),
                       ("pr", ("status", "post")), ("dr", ("hap", "prob", "status"))):
        for k in keys:
            assert x[call][k].tobytes() == y[call][k].tobytes(), (what, call, k)
    if likelihoods:
        for k in ("mantissa", "exponent", "status"):
            assert x["lk"][k].tobytes() == y["lk"][k].tobytes(), (what, "lk", k)


def statuses(b):
    """Every status of a bundle's four calls."""
    return np.concatenate([b[c]["status"] for c in ("gp", "sw", "pr", "dr")])


def unscaled_extended(name):
    key = ("ext0", name)
    if key not in _cache:
        a, pt = mined(name)
        m = fed(name, pt)
        m.set_posterior_range(True)
        _cache[key] = bundle(m, a, D_BYTES)
    return _cache[key]


@pytest.mark.parametrize("name", SCALED_PANELS)
def test_regular_mode_gives_the_scaled_tables_up(name):
    """The guard on the GPU side: in the regular mode no row of a scaled table
    has status 0: all 1 at ZERO_C, all 2 at SUBNORMAL_C (as measured)."""
    a, pt = mined(name)
    m = fed(name, scaled(pt, ZERO_C))
    assert not (m.estep_results()["total"] > 0).any()
    z = bundle(m, a, 8)
    assert (statuses(z) == 1).all() and (z["lk"]["status"] == 0).all()
    m = fed(name, scaled(pt, SUBNORMAL_C[name]))
    s = bundle(m, a, 8)
    st = statuses(s)
    print(name, "subnormal c:", {k: int((st == k).sum()) for k in (0, 1, 2)}, "draw status", s["dr"]["status"].tolist(),
          "E-step totals", m.estep_results()["total"].tolist())
    assert (st == 2).all()


@pytest.mark.parametrize("c_kind", ["subnormal", "zero"])
@pytest.mark.parametrize("name", SCALED_PANELS)
def test_scaled_tables_against_enumeration(name, c_kind):
    """Extended range on a table the regular mode cannot use: the four calls
    against the enumeration of the unscaled table within the existing bounds,
    the likelihoods against the enumerated totals of the scaled one, and every
    byte equal to the extended run on the unscaled table."""
    a, pt = mined(name)
    N, _, L = a.shape
    c = SUBNORMAL_C[name] if c_kind == "subnormal" else ZERO_C
    spt = scaled(pt, c)
    m = fed(name, spt)
    regular = m.posterior_draws(1, SEED)["status"]
    assert (regular != 0).all()
    m.set_posterior_range(True)
    res = dict(gp=check_posteriors(m, a, pt, 1), sw=check_switches(m, a, pt, 1, test_switch_enumeration.COUNTS[name]),
               pr=check_pairs(m, a, pt, 1, test_pair_enumeration.COUNTS[name], schedules=c_kind == "subnormal"),
               dr=check_draws(m, a, pt, 1))
    assert m.posterior_stats()["n_pruned"] == m.switch_stats()["n_pruned"] == m.pair_stats()["n_pruned"] == 0
    assert m.draw_stats()["n_pruned"] == 0
    # the likelihoods: mantissa x 2^exponent against the enumerated total of the scaled table
    lk = m.genotype_likelihoods()
    assert not lk["status"].any() and ((lk["mantissa"] >= 0.5) & (lk["mantissa"] < 1)).all()
    ta = en.allele_table(a)
    worst, n = 0.0, 0
    for i, e in enumerate(en.estep(a, spt, 1)):
        if e is None:
            continue
        got = Fraction(float(lk["mantissa"][i])) * Fraction(2) ** int(lk["exponent"][i])
        g = en.gamma(2 * L + 2 + en.phasing_count(a[i], ta))
        assert abs(got - e["total"]) <= g * e["total"], (i, float(got / e["total"] - 1))
        worst = max(worst, float(abs(got / e["total"] - 1) / en.U))
        n += 1
    assert n == INDIVIDUALS[name]
    assert (lk["exponent"] < -1022).all()
    sub = m.genotype_likelihoods([N - 1, 0, N - 1])  # a subset, permuted, with a repeat
    for k in ("mantissa", "exponent", "status"):
        assert sub[k].tolist() == lk[k][[N - 1, 0, N - 1]].tolist()
    # every byte of the unscaled table's extended run; the exponents move by exactly 2 c L
    ref, got = unscaled_extended(name), bundle(m, a, D_BYTES)
    same_bundles(got, ref, (name, c), likelihoods=False)
    assert got["lk"]["mantissa"].tobytes() == ref["lk"]["mantissa"].tobytes()
    assert ((ref["lk"]["exponent"] - got["lk"]["exponent"]) == prior_shift(c, L)).all()
    assert (ref["lk"]["exponent"] > -60).all()
    print(name, c, "individuals recovered", int((regular != 0).sum()), "of", N, "sites", len(got["gp"]["indiv"]),
          len(got["sw"]["indiv"]), len(got["pr"]["status"]), "largest exponent magnitude", int(np.abs(lk["exponent"]).max()),
          "likelihood worst_u", worst, {k: v["worst_u"] for k, v in res.items()})
    assert (regular != 0).sum() == N and (got["dr"]["status"] == 0).all()


def test_negative_control():
    """One tp off by 1e-9 in the table the kernels run on, scaled like the
    others: the value comparisons of the extended range raise."""
    name = "a3"
    a, pt = mined(name)
    m = gpu_model(name, 3, a)
    m.find_patterns()
    bad_tp, _ = perturbed_tables(a, pt, gpu_view(m), 1)
    m2 = fed(name, scaled(bad_tp, SUBNORMAL_C[name]))
    m2.set_posterior_range(True)
    with pytest.raises(BinMismatch) as ei:
        check_posteriors(m2, a, pt, 1)
    assert 0 < ei.value.args[0][4] < 1e-8  # the size of the perturbation, not a wrong table
    with pytest.raises(ValueMismatch) as ei:
        check_switches(m2, a, pt, 1)
    assert 0 < ei.value.args[0][4] < 1e-8
    m3 = fed(name, scaled(pt, SUBNORMAL_C[name]))  # the same calls pass on the true table
    m3.set_posterior_range(True)
    check_posteriors(m3, a, pt, 1)
    check_switches(m3, a, pt, 1)


def close(x, y, g):
    """|x - y| within the sum of the two bounds g of one exact value (module docstring)."""
    x, y = Fraction(float(x)), Fraction(float(y))
    return abs(x - y) <= 2 * g * max(x, y) / (1 - g)


@pytest.mark.parametrize("name", sorted(PANELS))
def test_regular_against_extended(name):
    """On the mined (unscaled) tables of the seven panels, where the regular
    mode answers everything: each value within the sum of the two bounds of
    the other, the draws' haplotypes equal.  Prints the byte-identical rows."""
    a = build_panel(name)
    m = gpu_model(name, PANELS[name]["S"][0], a)
    m.find_patterns()
    m.resolve_all()
    N, _, L = a.shape
    ta = en.allele_table(a)
    g = [en.gamma(posterior_k(L, en.phasing_count(a[i], ta))) for i in range(N)]
    reg = bundle(m, a, D_BYTES)
    m.set_posterior_range(True)
    ext = bundle(m, a, D_BYTES)
    m.set_posterior_range(False)
    same_bundles(bundle(m, a, D_BYTES), reg, "regular again")
    assert not statuses(reg).any() and not statuses(ext).any()
    queries = pe.all_pairs(a)
    ident = {}
    for call, who in (("gp", reg["gp"]["indiv"]), ("sw", reg["sw"]["indiv"]), ("pr", np.array([q[0] for q in queries], np.int32))):
        x, y = reg[call]["post"], ext[call]["post"]
        assert x.shape == y.shape and len(who) == len(x)
        for q in range(len(x)):
            assert all(close(p, r, g[who[q]]) for p, r in zip(x[q], y[q])), (call, q, x[q].tolist(), y[q].tolist())
        ident[call] = (int(sum(x[q].tobytes() == y[q].tobytes() for q in range(len(x)))), len(x))
    assert reg["dr"]["hap"].tobytes() == ext["dr"]["hap"].tobytes()
    for i in range(N):
        gd = en.gamma(4 * L + 5 + en.phasing_count(a[i], ta))
        assert all(close(p, r, gd) for p, r in zip(reg["dr"]["prob"][i], ext["dr"]["prob"][i])), i
    ident["dr"] = (int(sum(reg["dr"]["prob"][i].tobytes() == ext["dr"]["prob"][i].tobytes() for i in range(N))), N)
    # the divisor: the E-step's total against the scaled pass's own
    tot = m.estep_results()["total"]
    lk = ext["lk"]
    own = np.ldexp(lk["mantissa"], lk["exponent"])
    ident["total"] = (int((own == tot).sum()), N)
    print(name, "byte-identical rows (of):", ident)
    # seen to hold on the MI355X on all seven panels: the value pass's total has the bits of the scaled pass's own,
    # and then so has every row (a finding about these kernels, DESIGN.md section 4, not a promise of the interface)
    assert all(x == n for x, n in ident.values()), ident


# ---------------------------------------------------------------- 60 x 120 ----
def large_tables():
    if "large" not in _cache:
        N, L = BITS_SHAPE
        a = mosaic_with_heads(N, L, 3, 0.05, 7)
        m = hmc_amd.HaploModel()
        m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * L))
        m.find_patterns()
        assert m.head_len() == 1
        pt = m.patterns()
        _cache["large"] = (a, pt, scaled(pt, LARGE_C))
    return _cache["large"]


def large_queries(a):
    return pe.span_list(a, 3)


def large_model(table, budgets=None, shard=None, windows=None):
    a = large_tables()[0]
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * a.shape[2]))
    if budgets:
        m.set_store_budgets(*budgets)
    if windows:
        m.set_estep_windows("always", windows)
    feed(m, table)
    if shard:
        m.set_shard(*shard)
    m.resolve_all()
    return m


def large_reference():
    """Extended range on the scaled table of the 60 x 120 panel, one group."""
    if "large_ref" not in _cache:
        a, _, spt = large_tables()
        m = large_model(spt)
        assert int(m.frontier_max().max()) > 256
        reg = bundle(m, a, 8, large_queries(a))
        given_up = reg["dr"]["status"] != 0  # a run the regular mode cannot do: it gives these individuals up
        assert given_up.any() and np.array_equal(reg["sw"]["status"] != 0, given_up[reg["sw"]["indiv"]])
        _cache["large_given_up"] = int(given_up.sum())
        m.set_posterior_range(True)
        ref = bundle(m, a, D_BYTES, large_queries(a))
        assert m.posterior_stats()["groups"] == 1 and not statuses(ref).any() and not any(ref["n_pruned"])
        _cache["large_ref"] = ref
    return _cache["large_ref"]


def test_large_panel_scaled_against_unscaled():
    """Frontiers of up to 890 states, both stores in play: the extended range
    gives the scaled table (priors times 2^-960) the bytes of the unscaled one."""
    a, pt, spt = large_tables()
    N, L = BITS_SHAPE
    ref = large_reference()
    m = large_model(pt)
    m.set_posterior_range(True)
    got = bundle(m, a, D_BYTES, large_queries(a))
    same_bundles(got, ref, "unscaled", likelihoods=False)
    assert got["lk"]["mantissa"].tobytes() == ref["lk"]["mantissa"].tobytes() and not got["lk"]["status"].any()
    assert ((got["lk"]["exponent"] - ref["lk"]["exponent"]) == prior_shift(LARGE_C, L)).all()
    assert ((ref["lk"]["exponent"] < -1022).sum()) == _cache["large_given_up"]
    ta = en.allele_table(a)
    syms = [[s for s, f in ta[k] if f > 0] for k in range(L)]
    for i in range(0, N, 7):
        check_genotype(ref["dr"]["hap"][i], a[i], syms)
    print("individuals the regular mode gives up on the scaled table", _cache["large_given_up"], "of", N,
          "sites", len(ref["gp"]["indiv"]), len(ref["sw"]["indiv"]), len(ref["pr"]["status"]), "exponents",
          int(ref["lk"]["exponent"].min()), int(ref["lk"]["exponent"].max()), "unscaled", int(got["lk"]["exponent"].min()),
          int(got["lk"]["exponent"].max()))
    assert len(ref["gp"]["indiv"]) > 100 and len(ref["sw"]["indiv"]) > 100


@pytest.mark.parametrize("path", ["groups", "shard", "tier1", "slots", "windowed"])
def test_large_panel_bits_independent_of_path(path):
    """Forced store groups, a shard, the switch tier of 1, every instantiated NS
    and a windowed E-step before the call: the same bytes in extended range."""
    a, _, spt = large_tables()
    ref = large_reference()
    qs = large_queries(a)
    if path == "groups":
        m = large_model(spt, budgets=BITS_BUDGETS)
        m.set_posterior_range(True)
        same_bundles(bundle(m, a, D_BYTES, qs), ref, path)
        assert m.posterior_stats()["groups"] >= 2 and m.switch_stats()["groups"] >= 2 and m.pair_stats()["groups"] >= 2
        assert m.draw_stats()["groups"] >= 2 and m.likelihood_stats()["groups"] >= 2
    elif path == "shard":
        m = large_model(spt, shard=(20, 40))
        m.set_posterior_range(True)
        got = bundle(m, a, D_BYTES, [q for q in qs if 20 <= q[0] < 40])
        for call, who in (("gp", ref["gp"]["indiv"]), ("sw", ref["sw"]["indiv"]), ("pr", np.array([q[0] for q in qs]))):
            sel = (who >= 20) & (who < 40)
            assert sel.sum() > 0
            for k in ("status", "post"):
                assert got[call][k].tobytes() == np.ascontiguousarray(ref[call][k][sel]).tobytes(), (call, k)
        for k in ("hap", "prob", "status"):
            assert got["dr"][k].tobytes() == np.ascontiguousarray(ref["dr"][k][20:40]).tobytes(), k
        for k in ("mantissa", "exponent", "status"):
            assert got["lk"][k].tobytes() == np.ascontiguousarray(ref["lk"][k][20:40]).tobytes(), k
    elif path == "tier1":
        m = large_model(spt)
        m.set_posterior_range(True)
        m.set_switch_tier(1)
        sw = m.switch_posteriors()
        assert m.switch_stats()["n_spilled"] > 0
        assert sw["status"].tobytes() == ref["sw"]["status"].tobytes() and sw["post"].tobytes() == ref["sw"]["post"].tobytes()
    elif path == "slots":
        m = large_model(spt)
        m.set_posterior_range(True)
        for ns in SLOTS:
            for tier in (0, 1):
                m.set_pair_tuning(ns, tier)
                pr = ask(m, qs)
                assert m.pair_stats()["slots"] == ns and (tier == 0 or m.pair_stats()["n_spilled"] > 0)
                assert pr["status"].tobytes() == ref["pr"]["status"].tobytes(), (ns, tier)
                assert pr["post"].tobytes() == ref["pr"]["post"].tobytes(), (ns, tier)
    else:
        m = large_model(spt, windows=16)
        assert m.estep_windows()["windows"] == -(-BITS_SHAPE[1] // 16)
        m.set_posterior_range(True)
        same_bundles(bundle(m, a, D_BYTES, qs), ref, path)


# -------------------------------------------------------------- long panels ----
def long_panel(which):
    if which == "mixed_12x1200":
        return mixed_panel(MIXED_L)
    if which == "pruned_60x1600":
        a = synth.founder_mosaic(60, 1600, A=2, seed=1).alleles.copy()
        miss = np.random.default_rng(3).random((60, 2, 1600)) < 0.01
        miss[:, :, 0] = False
        a[miss] = -1
        return a
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 2, (6, 2, 2500)) + ord("1")).astype(np.int32)
    r2 = np.random.default_rng(11)
    for _ in range(20):
        a[r2.integers(0, 6), r2.integers(0, 2), r2.integers(1, 2500)] = -1
    return a


# individuals the regular mode gives up on (status 1 or 2) although their lattice is alive
# (60 x 1 600: two individuals have a subnormal P(genotype); one of them has the 54 missing-allele sites of
# test_pruned_records, the other none)
GIVEN_UP = {"mixed_12x1200": 7, "pruned_60x1600": 2, "iid_6x2500": 6}


@pytest.mark.parametrize("which", sorted(GIVEN_UP))
def test_long_panels(which):
    a = long_panel(which)
    N, _, L = a.shape
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * L))
    m.find_patterns()
    m.resolve_all()
    er = m.estep_results()
    resolved = (er["status"] == 0) & (er["total"] > 0)
    given_up = ~resolved | (er["total"] < DBL_MIN)
    assert given_up.sum() == GIVEN_UP[which]
    reg_gp, reg_sw = m.genotype_posteriors(), m.switch_posteriors()
    assert np.array_equal(reg_gp["status"] != 0, given_up[reg_gp["indiv"]])
    assert np.array_equal(reg_sw["status"] != 0, given_up[reg_sw["indiv"]])
    m.set_posterior_range(True)
    gp, sw, lk = m.genotype_posteriors(), m.switch_posteriors(), m.genotype_likelihoods()
    assert m.posterior_stats()["n_pruned"] == 0 and m.switch_stats()["n_pruned"] == 0
    # nobody is dead, nobody is given up
    assert not gp["status"].any() and not sw["status"].any() and not lk["status"].any()
    assert np.array_equal(lk["exponent"] < -1022, given_up), (lk["exponent"].tolist(), given_up.tolist())
    F = int(m.frontier_max().max())
    g = en.gamma(rowsum_k(L, F))
    assert g < 1e-7
    worst = 0.0
    for out in (gp, sw):
        for row in out["post"]:
            d = abs(exact_sum(row) - 1)
            assert d <= g, (float(d), float(g))
            worst = max(worst, float(d))
    # rows the regular mode answers: the same numbers
    agree = identical = 0
    for reg, out in ((reg_gp, gp), (reg_sw, sw)):
        assert np.array_equal(reg["indiv"], out["indiv"])
        for q in np.nonzero(reg["status"] == 0)[0]:
            under = (6 * L * F * F + 2 * F) * ETA / Fraction(float(er["total"][reg["indiv"][q]]))
            for x, y in zip(reg["post"][q], out["post"][q]):
                x, y = Fraction(float(x)), Fraction(float(y))
                assert abs(x - y) <= g * (x + y) / (1 - g) + under, (q, float(x), float(y))
            agree += 1
            identical += reg["post"][q].tobytes() == out["post"][q].tobytes()
    # the draws of the individuals the regular mode gives up on: marginals against the switch posteriors
    who = np.nonzero(given_up)[0].astype(np.int32)
    dr = m.posterior_draws(D_LONG, SEED, who)
    assert m.draw_stats()["n_pruned"] == 0 and not dr["status"].any()
    assert (dr["prob"] >= 0).all() and (dr["prob"] <= 1 + 1e-12).all()
    ta = en.allele_table(a)
    syms = [[s for s, f in ta[k] if f > 0] for k in range(L)]
    compared = 0
    for r, i in enumerate(who):
        check_genotype(dr["hap"][r], a[i], syms)
        h = dr["hap"][r]
        for q in np.nonzero(sw["indiv"] == i)[0]:
            x, y = int(sw["locus_a"][q]), int(sw["locus_b"][q])
            cis = int(((h[:, 0, x] < h[:, 1, x]) == (h[:, 0, y] < h[:, 1, y])).sum())
            compared += de.check_frequencies({"cis": cis, "trans": D_LONG - cis}, D_LONG,
                                             {"cis": float(sw["post"][q, 0]), "trans": float(sw["post"][q, 1])})
    rec_sites = int(given_up[gp["indiv"]].sum()) + int(given_up[sw["indiv"]].sum())
    print(which, "individuals recovered", int(given_up.sum()), "of", N, "their sites", rec_sites, "of", len(gp["indiv"]) + len(sw["indiv"]),
          "rows compared with the regular mode", agree, "byte-identical", int(identical), "worst row-sum deviation", worst,
          "bound", float(g), "F", F, "exponents", int(lk["exponent"].min()), int(lk["exponent"].max()),
          "marginal comparisons", compared, m.posterior_stats(), m.switch_stats(), m.draw_stats())
    assert rec_sites > 0 and compared > 0


# ------------------------------------------------------- the EM, call order ----
def same(x, y):
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    return x == y


@pytest.mark.parametrize("exact", [False, True])
def test_leaves_the_em_untouched(exact):
    """The chain of test_gpu_posteriors.test_leaves_the_em_untouched with the
    extended-range calls in between: the same bits; and the regular range
    afterwards answers its own bytes again."""
    a = build_panel("a4")

    def chain(call):
        m = gpu_model("a4", 6, a)
        m.exact_estimate = exact
        m.find_patterns()
        _, H, _ = m.resolve_all()
        state = []
        if call:
            reg0 = bundle(m, a, 64)
            before = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            m.set_posterior_range(True)
            ext = bundle(m, a, 64)
            assert not statuses(ext).any() and len(ext["gp"]["indiv"]) > 0
            after = (m.estep_results(), m.samples(H), m.estep_split_stats(), m.estep_frontier())
            m.set_posterior_range(False)
            state = [before, after, reg0, bundle(m, a, 64)]
            if call == "stay":
                m.set_posterior_range(True)
        m.find_patterns()
        pt = m.patterns()
        ll, H2, re = m.resolve_all()
        al, w, tw = m.samples(H2)
        er = m.estep_results()
        return state, (pt, ll, H2, re, al, w, tw, er, m.resolutions())

    state, with_call = chain("back")
    _, stay = chain("stay")
    _, without = chain(None)
    assert same(state[0], state[1]), "hmc_get_estep rows, samples or E-step statistics moved"
    assert same(state[2], state[3]), "the regular range no longer answers its own bytes"
    assert same(with_call, without) and same(stay, without)


def test_call_order_and_arguments():
    a, _ = mined("a3")
    m = gpu_model("a3", 3, a)
    m.set_posterior_range(True)
    m.find_patterns()
    calls = (m.genotype_likelihoods, m.genotype_posteriors, m.switch_posteriors, lambda: m.posterior_draws(4, 0),
             lambda: ask(m, pe.all_pairs(a)[:3]))
    for f in calls:
        with pytest.raises(HMCError) as ei:
            f()
        assert ei.value.code == -1  # HMC_EARG: no E-step yet
    m.resolve_all()
    lk = m.genotype_likelihoods()
    assert len(lk["status"]) == a.shape[0] and not lk["status"].any()
    assert len(m.genotype_likelihoods([])["status"]) == 0
    with pytest.raises(HMCError) as ei:
        m.genotype_likelihoods([a.shape[0]])
    assert ei.value.code == -1 and "outside" in str(ei.value)
    m.find_patterns()  # an M-step: the forward pass would run on another table than the E-step's
    for f in calls:
        with pytest.raises(HMCError) as ei:
            f()
        assert ei.value.code == -1
    m.resolve_all()
    lk2 = m.genotype_likelihoods()
    assert not lk2["status"].any() and same(lk2, m.genotype_likelihoods())
    with pytest.raises(HMCError) as ei:  # neither 0 nor 1
        m._check(lib().hmc_set_posterior_range(m._h, 2))
    assert ei.value.code == -1


def test_cli_extended_range(tmp_path):
    """hmc_resolve --extended-range --output-switch-posteriors on the 12 x 1 200
    panel: lines for the individuals that have none without the flag, the
    numbers those of the API."""
    a = mixed_panel(MIXED_L)
    src = tmp_path / "mixed.inp"
    synth.write_phase(synth.Panel(a, "S" * a.shape[2]), str(src))

    def run(*flags):
        r = subprocess.run([CLI, *flags, "--output-switch-posteriors", str(src)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return (tmp_path / "mixed.inp.switches").read_text().splitlines()

    plain = run()
    lines = run("--extended-range")
    m = hmc_amd.HaploModel()
    m.load_phase(str(src))
    m.run()
    reg = m.switch_posteriors()
    m.set_posterior_range(True)
    out = m.switch_posteriors()
    assert not out["status"].any() and len(lines) - 1 == len(out["indiv"]) == len(se.sites(a))
    assert len(plain) - 1 == int((reg["status"] == 0).sum()) < len(lines) - 1
    for ln, q in zip(lines[1:], range(len(out["indiv"]))):
        f = ln.split("\t")
        assert len(f) == 7 and f[0].lstrip("#") == str(int(out["indiv"][q]) + 1)
        assert (float(f[5]), float(f[6])) == (float(out["post"][q, 0]), float(out["post"][q, 1]))
    ids = lambda ls: {ln.split("\t")[0] for ln in ls[1:]}
    gone = {str(i + 1) for i in set(reg["indiv"][reg["status"] != 0].tolist())}
    assert gone and not ({x.lstrip("#") for x in ids(plain)} & gone) and gone <= {x.lstrip("#") for x in ids(lines)}
    r = subprocess.run([CLI, "--extended-range", str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--extended-range needs" in r.stderr
