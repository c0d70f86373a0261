"""The library against exhaustive enumeration (tests/enumeration.py): the
panels and checks of tests/test_enumeration_oracle.py with hmc_amd.HaploModel
in place of the CPU restatement, which this file never touches.  The HIP
E-step (structure pass, value pass, k-best lists, traceback, weights), the
mining kernels and the exact M-step's trie walk are compared with sums over
every phasing in exact rational arithmetic, within bounds derived from
operation counts (enumeration.check_estep / check_mined_table / check_mstep).

The panels are tiny, so the launch rule picks one path; the other E-step
paths are forced one by one (PATHS).  Every case is a panel of at most 12
individuals x 10 loci; the enumeration is cached across cases.
"""
import numpy as np
import pytest

import hmc_amd

import enumeration as en
from test_enumeration_oracle import (ESTEP_CASES, MIN_FREQ_ABS, MINED, PANELS, build_panel, head_len, mining_params,
                                     perturbed_tables, prune, types_of)

pytestmark = pytest.mark.gpu


def gpu_model(name, S, a):
    c = PANELS[name]
    m = hmc_amd.HaploModel()
    m.sample_size = S
    m.min_freq_abs = MIN_FREQ_ABS
    m.min_pattern_len = c.get("min_len", 1)
    m.max_pattern_len = c.get("max_len", 30)
    if c.get("model"):
        m.model, m.mc_order = c["model"], c["mc_order"]
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), types_of(a)))
    return m


def last_symbols(pt):
    return np.array([pt["alleles"][i, pt["len"][i] - 1] for i in range(len(pt["len"]))], np.int32)


def feed(m, pt):
    m.set_patterns(pt["start"], pt["len"], pt["freq"], pt["tp"], pt["succ"], last_symbols(pt))


def gpu_view(m):
    """E-step results of the last resolve_all as enumeration.check_estep reads
    them: candidates' haplotypes are the samples, two per candidate."""
    ll, H, _ = m.resolve_all()
    er = m.estep_results()
    al, w, tw = m.samples(H)
    assert H == 2 * int(er["ncand"].sum())
    haps, k = [], 0
    for i in range(m.N):
        hh = []
        for c in range(er["ncand"][i]):
            assert w[k] == w[k + 1] == er["weight"][i, c], (i, c)
            hh.append((tuple(int(x) for x in al[k]), tuple(int(x) for x in al[k + 1])))
            k += 2
        haps.append(hh)
    assert abs(tw - float(sum(en.Fraction(float(x)) for x in w))) <= len(w) * 2.0 ** -53 * tw
    return dict(ll=ll, total=er["total"], ncand=er["ncand"], prior=er["prior"], posterior=er["posterior"],
                weight=er["weight"], haps=haps, resolutions=m.resolutions())


# includes S = 17 (one link per lane) and S = 33 (a list over two lanes' slots) on the 4-allele panel
@pytest.mark.parametrize("name,S", ESTEP_CASES)
def test_estep_on_m0(name, S):
    """E1 on the table the library mined from the genotypes."""
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    assert m.head_len() == head_len(name)
    pt = m.patterns()
    assert en.check_chain_equals_global(a, pt, head_len(name)) == 0
    print(name, S, en.check_estep(gpu_view(m), a, pt, head_len(name), S))


PATHS = {
    "layout0": lambda m: m.set_value_layout(0),
    "layout2": lambda m: m.set_value_layout(2),
    "fast": lambda m: m.set_value_mode("fast"),
    "shapes_1_8_2_8": lambda m: m.set_pass_shapes(1, 8, 2, 8),
    "shapes_16_1_16_1": lambda m: m.set_pass_shapes(16, 1, 16, 1),
    "id_order": lambda m: m.set_end_order(False),
    "windows3": lambda m: m.set_estep_windows("always", 3),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_estep_paths(path):
    """The E-step paths the launch rule does not pick at this size, on the
    3-allele panel with missing data."""
    name, S = "a3", 4
    a = build_panel(name)
    m = gpu_model(name, S, a)
    PATHS[path](m)
    m.find_patterns()
    pt = m.patterns()
    view = gpu_view(m)
    if path == "windows3":
        assert m.estep_windows()["windows"] == -(-a.shape[2] // 3)
    print(path, en.check_estep(view, a, pt, 1, S))


@pytest.mark.parametrize("name,S", [("snp", 10), ("a3", 3)])
def test_hand_pruned_table_follows_the_chain(name, S):
    """A table with a third of its longer patterns deleted, through
    set_patterns: the chain differs from the global longest match there, and
    the E-step follows the chain."""
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pruned, ndrop = prune(m.patterns(), en.allele_table(a), a.shape[2])
    assert ndrop >= 3 and en.check_chain_equals_global(a, pruned, 1) > 0
    m2 = gpu_model(name, S, a)
    feed(m2, pruned)
    print(name, S, en.check_estep(gpu_view(m2), a, pruned, 1, S))


def test_negative_controls():
    """One tp off by 1e-9 relative, or one successor redirected, in the table
    the kernels run on: the totals check fails."""
    name, S = "a3", 3
    a = build_panel(name)
    m = gpu_model(name, S, a)
    m.find_patterns()
    pt = m.patterns()
    view = gpu_view(m)
    en.check_estep(view, a, pt, 1, S)
    for bad in perturbed_tables(a, pt, view, 1):
        m2 = gpu_model(name, S, a)
        feed(m2, bad)
        v = gpu_view(m2)
        totals = [en.within(v["total"][i], e["total"], en.gamma(2 * a.shape[2] + 2 + e["M"]))
                  for i, e in enumerate(en.estep(a, pt, 1)) if e is not None]
        assert not all(totals)
        with pytest.raises(AssertionError):
            en.check_estep(v, a, pt, 1, S)


@pytest.mark.parametrize("name", MINED)
def test_mined_tables(name):
    """M0 from the genotypes and M1 from the samples of E1: pattern set, freq,
    prefix, tp, successors."""
    a = build_panel(name)
    m = gpu_model(name, PANELS[name]["S"][-1], a)
    mf, mnl, mxl = mining_params(name, a.shape[0])
    m.find_patterns()
    print(name, "M0", en.check_mined_table(m.patterns(), a, mf, mnl, mxl, allow_equal=not (a < 0).any()))
    _, H, _ = m.resolve_all()
    al, w, _ = m.samples(H)
    m.find_patterns()
    print(name, "M1", en.check_mined_table(m.patterns(), a, mf, mnl, mxl, samples=(al, w)))


@pytest.mark.parametrize("name", sorted(PANELS))
def test_exact_mstep(name):
    """One exact M-step (exact_estimate) after M0 and E1.  Bound
    (enumeration.check_mstep): per frequency N addends, each rounded to a
    multiple of the fixed-point quantum 2^-44 (exact.hpp:9, exact.hip:604-605
    and :891-892, ctx_exact.cpp:160-164), so N * 2^-45 / N = 2^-45 absolute on
    freq and prefix, plus gamma(max_i (6L + 8 + 3 M_i) + N + 1) relative for
    the floating-point walk; on these panels that is below 1e-9 relative at
    the smallest non-zero frequency (asserted)."""
    a = build_panel(name, quirk=False)
    m = gpu_model(name, PANELS[name]["S"][-1], a)
    m.exact_estimate = True
    m.find_patterns()
    prev = m.patterns()
    m.resolve_all()
    m.find_patterns()
    new = m.patterns()
    worst = en.check_mstep(new, a, prev, head_len(name), fixed_point=True)
    print(name, worst)
    assert worst["loosest_rel_bound"] <= 1e-9
    en.check_successors(new, en.allele_table(a), a.shape[2])
