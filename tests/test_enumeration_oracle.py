"""The CPU restatement against exhaustive enumeration (tests/enumeration.py).

Every other parity test compares the library with oracle/hmc_oracle.cpp, a
restatement of the reference written next to the kernels; a misreading of the
model shared by both would pass them all.  Here the restatement's E-step
(pair DP, state merging, reversed / homozygous flags, k-best lists, traceback,
weights), its mining and its exact M-step are checked against definitions
that need none of that machinery: every phasing of every genotype listed and
scored in exact rational arithmetic.  tests/test_gpu_enumeration.py runs the
same panels and checks on the library.

The tolerances are derived from operation counts in the docstrings of
enumeration.check_estep / check_mined_table / check_mstep, not fitted.
Individuals with a missing allele at a head locus follow the reference's
initHeadList (HaploBuilder.cpp:153-224), which the enumerated model does not
describe (enumeration.HEAD_QUIRK); the panels keep at most one such
individual (never more than one in four, asserted), and none for the exact
M-step, which sums over everyone.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enumeration as en  # noqa: E402
from hmc_amd import synth  # noqa: E402

# name: panel (founder mosaic, seeds fixed here), sample sizes, model parameters.  The seeds are
# chosen so that every individual has at most 4 096 ordered phasings, one individual keeps a missing
# head allele on the panels with missing data, the last locus has missing data, and no mining
# candidate sits within 1e-9 of min_freq (all asserted where used).  S = 17 and 33 on the
# 4-allele panel reach the library's one-link-per-lane lists and its two-slot lists.
PANELS = {
    "snp": dict(gen=dict(N=12, L=10, A=2, K=6, rho=0.1, missing=0.0, seed=100), S=[1, 2, 10]),
    "a3": dict(gen=dict(N=10, L=8, A=3, K=6, rho=0.1, missing=0.10, seed=100), S=[3, 4]),
    "a4": dict(gen=dict(N=8, L=6, A=4, K=6, rho=0.1, missing=0.15, seed=154), S=[6, 17, 33]),
    "mc": dict(gen=dict(N=10, L=8, A=2, K=6, rho=0.1, missing=0.05, seed=115), S=[4], model="MC", mc_order=1),
    "short": dict(gen=dict(N=12, L=10, A=2, K=6, rho=0.1, missing=0.05, seed=122), S=[5], max_len=3),
    "minlen2": dict(gen=dict(N=10, L=8, A=2, K=6, rho=0.1, missing=0.0, seed=105), S=[10], min_len=2),
    # three individuals made homozygous, then (individual, loci with both alleles missing, loci with
    # one missing): their phasings mix homozygous pairs (prior P(h)^2) with heterozygous ones
    # (2 P(h0) P(h1)), which the final list must rank on the doubled likelihood (HaploBuilder.cpp:98)
    "hom": dict(gen=dict(N=10, L=8, A=3, K=6, rho=0.1, missing=0.0, seed=107), S=[1, 2, 3],
                hom=[(0, [3], []), (1, [], [2, 5]), (2, [7], [1])]),
}
MIN_FREQ_ABS = 1.5
ESTEP_CASES = [(n, S) for n in PANELS for S in PANELS[n]["S"]]
# `hom` has missing data at five loci only, so candidates that avoid them have dyadic frequencies
# and some equal min_freq exactly: its pattern set is not compared
MINED = sorted(n for n in PANELS if n != "hom")


def head_len(name):
    c = PANELS[name]
    return c["mc_order"] + 1 if c.get("model") == "MC" else max(1, c.get("min_len", 1))


def mining_params(name, N):
    """(min_freq, min_len, max_len) of searchPattern: MC mines every string
    of length order + 1 (findPatternBlock, PatternManager.cpp:75-88)."""
    c = PANELS[name]
    if c.get("model") == "MC":
        return Fraction(-1), c["mc_order"] + 1, c["mc_order"] + 1
    return Fraction(MIN_FREQ_ABS) / (2 * N), c.get("min_len", 1), c.get("max_len", 30)


def build_panel(name, quirk=True):
    """The panel's alleles[N][2][L].  Missing alleles at the head loci are put
    back from the same mosaic drawn without missing data, for every individual
    but the first one that has them (`quirk`), or for all."""
    g = dict(PANELS[name]["gen"])
    a = synth.founder_mosaic(**g).alleles.copy()
    full = synth.founder_mosaic(**dict(g, missing=0.0)).alleles
    hl = head_len(name)
    rows = np.nonzero(en.head_quirk(a, hl))[0]
    for i in rows[1:] if quirk else rows:
        a[i, :, :hl] = full[i, :, :hl]
    for i, both, one in PANELS[name].get("hom", []):
        a[i, 1] = a[i, 0]
        a[i, :, both] = -1
        a[i, 1, one] = -1
    left = en.head_quirk(a, hl)
    assert left.sum() <= (1 if quirk else 0) and left.sum() <= a.shape[0] / 4
    if (a < 0).any():  # missing data stays everywhere else, the last locus included
        assert (a[~left][:, :, -1] < 0).any(), "no missing allele at the last locus"
        assert (a[~left][:, :, hl:-1] < 0).any()
    ta = en.allele_table(a)
    assert max(en.phasing_count(a[i], ta) for i in range(a.shape[0])) <= en.MAX_PHASINGS
    return a


def types_of(a):
    return "S" * a.shape[2]


def make_oracle(oracle_mod, name, S, a):
    c = PANELS[name]
    o = oracle_mod.Oracle(a, types_of(a), min_freq_abs=MIN_FREQ_ABS, min_len=c.get("min_len", 1),
                          max_len=c.get("max_len", 30), sample_size=S)
    if c.get("model"):
        o.set_model(c["model"], c["mc_order"])
    return o


def oracle_view(o, ll):
    nc, gp = o.estep_summary()
    al, w, tw = o.samples()
    view = dict(ll=ll, total=gp, ncand=nc, prior=[], posterior=[], weight=[], haps=[], resolutions=o.resolutions())
    k = 0
    for i in range(o.N):
        pr, po, ww, hh = [], [], [], []
        for c in range(nc[i]):
            hap, p, q = o.candidate(i, c)
            h0, h1 = tuple(int(x) for x in hap[0]), tuple(int(x) for x in hap[1])
            # the candidate's two haplotypes are the samples, both with its weight
            assert tuple(al[k]) == h0 and tuple(al[k + 1]) == h1 and w[k] == w[k + 1]
            pr.append(p), po.append(q), ww.append(w[k]), hh.append((h0, h1))
            k += 2
        view["prior"].append(pr), view["posterior"].append(po), view["weight"].append(ww), view["haps"].append(hh)
    assert k == len(w)
    assert abs(tw - float(sum(Fraction(float(x)) for x in w))) <= len(w) * 2.0 ** -53 * tw
    return view


def prune(pt, ta, L):
    """The hand-pruned table: of the patterns of length >= 2 in (start,
    symbols) order every third is deleted — prefixes go while their extensions
    stay, so some kept patterns lose a suffix or a prefix — and the successors
    are rebuilt by the rule."""
    order = sorted((int(pt["start"][i]), tuple(int(x) for x in pt["alleles"][i, :pt["len"][i]]), i)
                   for i in range(len(pt["start"])) if pt["len"][i] >= 2)
    drop = {i for k, (_, _, i) in enumerate(order) if k % 3 == 0}
    keep = [i for i in range(len(pt["start"])) if i not in drop]
    out = {k: np.ascontiguousarray(v[keep]) for k, v in pt.items()}
    out["succ"] = en.rebuild_successors(out, ta, L)
    if out["succ"].shape[1] < pt["succ"].shape[1]:
        out["succ"] = np.pad(out["succ"], ((0, 0), (0, pt["succ"].shape[1] - out["succ"].shape[1])), constant_values=-1)
    return out, len(drop)


def perturbed_tables(a, pt, view, hl):
    """The negative controls' tables: on the individual with the fewest
    phasings (its best pair holds at least 1 / M of its total, so a relative
    1e-9 on one factor moves the total by far more than the bound), the second
    pattern of the best pair's first haplotype gets tp * (1 + 1e-9); and the
    successor that leads to it is redirected to another pattern ending at the
    same locus."""
    ta = en.allele_table(a)
    ok = ~en.head_quirk(a, hl)
    i = min((i for i in range(a.shape[0]) if ok[i]), key=lambda i: en.phasing_count(a[i], ta))
    h = view["haps"][i][0][0]
    t = en.Table(pt)
    cur = t.index[(0, h[:hl])]
    nxt = t.longest(h, hl + 1, t.start[cur])
    bad_tp = {k: v.copy() for k, v in pt.items()}
    bad_tp["tp"][nxt] *= 1.0 + 1e-9
    assert bad_tp["tp"][nxt] != pt["tp"][nxt]
    j = [s for s, _ in ta[hl]].index(h[hl])
    assert pt["succ"][cur, j] == nxt
    other = next(q for q in range(t.n) if q != nxt and t.start[q] + t.len[q] == hl + 1 and t.tp[q] != t.tp[nxt])
    bad_succ = {k: v.copy() for k, v in pt.items()}
    bad_succ["succ"][cur, j] = other
    return bad_tp, bad_succ


# ------------------------------------------------------------------ tests ----
@pytest.mark.parametrize("name", sorted(PANELS))
def test_allele_table(oracle_mod, name):
    a = build_panel(name)
    o = make_oracle(oracle_mod, name, 1, a)
    num, sym, fr = o.allele_table()
    ta = en.allele_table(a)
    assert num.tolist() == [len(x) for x in ta]
    for k, col in enumerate(ta):
        assert sym[k, :len(col)].tolist() == [s for s, _ in col]
        assert all(en.within(fr[k, j], f, en.gamma(1)) for j, (_, f) in enumerate(col))


@pytest.mark.parametrize("name,S", ESTEP_CASES)
def test_estep_on_m0(oracle_mod, name, S):
    """E1 on the genotype-mined table: totals, the S best priors, posteriors,
    weights, LL, and every candidate a phasing with its enumerated prior.  On
    a mined table the successor chain equals the global longest match."""
    a = build_panel(name)
    o = make_oracle(oracle_mod, name, S, a)
    o.find_patterns()
    assert o.head_len() == head_len(name)
    pt = o.patterns()
    assert en.check_chain_equals_global(a, pt, head_len(name)) == 0
    view = oracle_view(o, o.resolve_all())
    print(name, S, en.check_estep(view, a, pt, head_len(name), S))


@pytest.mark.parametrize("name", MINED)
def test_mined_tables(oracle_mod, name):
    """M0 from the genotypes and M1 from the samples of E1: the pattern set,
    freq, prefix, tp and every successor."""
    a = build_panel(name)
    S = PANELS[name]["S"][-1]
    o = make_oracle(oracle_mod, name, S, a)
    mf, mnl, mxl = mining_params(name, a.shape[0])
    o.find_patterns()
    print(name, "M0", en.check_mined_table(o.patterns(), a, mf, mnl, mxl, allow_equal=not (a < 0).any()))
    o.resolve_all()
    al, w, _ = o.samples()
    o.find_patterns()
    print(name, "M1", en.check_mined_table(o.patterns(), a, mf, mnl, mxl, samples=(al, w)))


@pytest.mark.parametrize("mode", ["reference", "device"])
@pytest.mark.parametrize("name", sorted(PANELS))
def test_exact_mstep(oracle_mod, name, mode):
    """One exact M-step after M0 and E1 in both summation orders; the panel
    without head-locus missing data (the M-step sums over every individual).
    Bound: enumeration.check_mstep."""
    a = build_panel(name, quirk=False)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][-1], a)
    o.set_exact_order(mode)
    o.find_patterns()
    prev = o.patterns()
    o.resolve_all()
    o.estimate_patterns()
    new = o.patterns()
    worst = en.check_mstep(new, a, prev, head_len(name), fixed_point=mode == "device")
    print(name, mode, worst)
    assert worst["loosest_rel_bound"] <= 1e-9
    en.check_successors(new, en.allele_table(a), a.shape[2])


@pytest.mark.parametrize("name,S", [("snp", 10), ("a3", 3)])
def test_hand_pruned_table_follows_the_chain(oracle_mod, name, S):
    """A table no miner produces: a third of the longer patterns deleted, so
    the successor's start constraint binds and the chain differs from the
    global longest match; the E-step must follow the chain."""
    a = build_panel(name)
    o = make_oracle(oracle_mod, name, S, a)
    o.find_patterns()
    pruned, ndrop = prune(o.patterns(), en.allele_table(a), a.shape[2])
    assert ndrop >= 3
    assert en.check_chain_equals_global(a, pruned, 1) > 0
    o.set_patterns(pruned)
    view = oracle_view(o, o.resolve_all())
    print(name, S, en.check_estep(view, a, pruned, 1, S))


def test_negative_controls(oracle_mod):
    """The checks are not vacuous: with one tp off by 1e-9 relative, or one
    successor redirected, in the table the implementation runs on (the
    enumerator keeps the true one) the totals check fails."""
    name, S = "a3", 3
    a = build_panel(name)
    o = make_oracle(oracle_mod, name, S, a)
    o.find_patterns()
    pt = o.patterns()
    view = oracle_view(o, o.resolve_all())
    en.check_estep(view, a, pt, 1, S)
    for bad in perturbed_tables(a, pt, view, 1):
        o.set_patterns(bad)
        v = oracle_view(o, o.resolve_all())
        totals = [en.within(v["total"][i], e["total"], en.gamma(2 * a.shape[2] + 2 + e["M"]))
                  for i, e in enumerate(en.estep(a, pt, 1)) if e is not None]
        assert not all(totals)
        with pytest.raises(AssertionError):
            en.check_estep(v, a, pt, 1, S)
