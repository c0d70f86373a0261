"""The value pass built with the sample size fixed at compile time
(estep_split.hip: estep_values<..., PAIR, SC = 10>, dispatched when S = 10 in
the pair layout) next to the run-time instantiations every other S and the
one-link layout keep: an E-step on the restatement's M0 model equals
HaploModel::resolveAll bit for bit through either, in one launch or in
windows, down to the final selection of the candidates."""
import pytest

from hmc_amd import synth
from test_gpu_parity import assert_estep_equal, gpu_model, last_symbols, panel

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(oracle_mod, key, p, S):
    """The restatement's M0 table and E-step for (panel, S), computed once and
    shared by the tests (nothing below changes it)."""
    k = (key, S)
    if k not in _REF:
        o = oracle_mod.Oracle(p.alleles, p.types, sample_size=S)
        o.find_patterns()
        pt = o.patterns()
        o.reset_counters()
        _REF[k] = (o, pt, o.resolve_all())
    return _REF[k]


def _check(oracle_mod, key, p, S, layout=None, shape=None, windows=0):
    o, pt, ll_o = _reference(oracle_mod, key, p, S)
    m = gpu_model(p, S)
    if layout is not None:
        m.set_value_layout(layout)
    if shape:
        m.set_pass_shapes(*shape)
    if windows:
        m.set_estep_windows("always", windows)
    m.set_patterns(pt["start"], pt["len"], pt["freq"], pt["tp"], pt["succ"], last_symbols(pt))
    ll_g, H, re_g = m.resolve_all()
    assert_estep_equal(m, o, ll_g, ll_o, H, re_g)
    return m


# cfg1, n60: biallelic (ties); a3miss5, a8: multi-allelic with missing genotypes.
# S = 10 runs the fixed-S instantiations of the pair layout, the others the
# run-time ones; layout 2 = two links per lane for every group, 0 = one link.
@pytest.mark.parametrize("layout", [2, 0], ids=["pair", "one_link"])
@pytest.mark.parametrize("S", [1, 3, 10, 16])
@pytest.mark.parametrize("name", ["cfg1", "n60", "a3miss5", "a8"])
def test_fixed_and_runtime_sample_size(oracle_mod, name, S, layout):
    _check(oracle_mod, name, panel(name), S, layout=layout)


@pytest.mark.parametrize("S", [3, 10])
@pytest.mark.parametrize("name", ["cfg1", "n60", "a3miss5", "a8"])
def test_windows_of_seven_loci(oracle_mod, name, S):
    """Windows of 7 loci: every window's launch starts from a checkpointed
    frontier, and only the last one reaches the final selection."""
    m = _check(oracle_mod, name, panel(name), S, windows=7)
    assert m.estep_windows()["windows"] > 1


def test_large_sample_size(oracle_mod):
    """n60 at S = 40 (one list per wave): most frontiers hold fewer than S + 1
    links, and the biallelic panel's candidates tie or are zero."""
    _check(oracle_mod, "n60", panel("n60"), 40)


def _duplicates_panel():
    p = panel("n60")
    al = p.alleles.copy()
    al[1] = al[0]
    al[2] = al[0]
    al[7] = al[6][::-1]           # the same genotype with the haplotypes exchanged
    al[3, 1] = al[3, 0]           # homozygous at every locus
    al[4, 1] = al[4, 0]
    return synth.Panel(alleles=al, types=p.types)


@pytest.mark.parametrize("layout", [2, 0], ids=["pair", "one_link"])
@pytest.mark.parametrize("S", [3, 10])
def test_duplicate_and_homozygous_individuals(oracle_mod, S, layout):
    _check(oracle_mod, "dups", _duplicates_panel(), S, layout=layout)


def _wide_end_panel():
    """a8 with the last four loci missing for every second individual: their
    frontiers are widest at the end of the chromosome."""
    p = panel("a8")
    al = p.alleles.copy()
    al[::2, :, -4:] = -1
    return synth.Panel(alleles=al, types=p.types)


@pytest.mark.parametrize("layout,S,tier", [(2, 10, 4), (0, 10, 12), (2, 3, 12)],
                         ids=["pair-S10", "one_link-S10", "pair-S3"])
def test_smallest_lds_tier(oracle_mod, layout, S, tier):
    """One wave per individual at 32 individuals per CU leaves the value pass
    the smallest LDS tier the shape hook can force (`tier` states per
    frontier), so nearly every state of these wide frontiers, the last one
    included, lives in the HBM tier."""
    p = _wide_end_panel()
    m = _check(oracle_mod, "wide_end", p, S, layout=layout, shape=(0, 0, 1, 32))
    assert int(m.frontier_max()[::2].max()) > 8 * tier
