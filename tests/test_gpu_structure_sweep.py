"""GPU parity of the structure pass's tail (estep_split.hip, estep_structure):
the record allocated from the chunk loop's own count of valid contributions,
the one sweep over the new frontier (counts scan, record fields, chain buckets
and the key-table clear together) and the allele-pair list kept in registers
at loci without a missing allele.  Every case runs E1 on M0 and the E-step
after one M-step and compares LL, R_E, the candidates and the samples with the
CPU restatement bit for bit — the bar of test_gpu_parity.py."""
import numpy as np
import pytest

import hmc_amd

from test_gpu_parity import _assert_table_bits, assert_estep_equal, gpu_model, panel

pytestmark = pytest.mark.gpu

NBUCKET_BYTES = 32 * 4


def _two_esteps(oracle_mod, name, setup, after=None, S=10):
    """E1 on M0 and E2 on M1 against the restatement; setup(m) before the
    panel's first E-step, after(m) after each."""
    p = panel(name)
    o = oracle_mod.Oracle(p.alleles, p.types, sample_size=S)
    m = gpu_model(p, S)
    setup(m)
    for step in range(2):
        o.find_patterns()
        m.find_patterns()
        ll_g, H, re_g = m.resolve_all()
        o.reset_counters()
        assert_estep_equal(m, o, ll_g, o.resolve_all(), H, re_g)
        if after:
            after(m, p)
    m.close()


@pytest.mark.parametrize("nw", [1, 4, 8, 16])
@pytest.mark.parametrize("name", ["miss2", "a3miss5", "a8"])
def test_pair_paths_alternate(oracle_mod, name, nw):
    """Loci with none, one and two missing alleles in one walk: the register
    pair (no hand-off) and the LDS pair list alternate, bi- and multi-allelic,
    in every instantiation of the kernel (1, 4, 8, 16 waves per individual)."""
    p = panel(name)
    miss = (p.alleles < 0).sum(axis=1)  # per individual and locus: 0, 1 or 2 missing alleles
    assert all((miss == k).any() for k in (0, 1, 2)), name
    _two_esteps(oracle_mod, name, lambda m: m.set_pass_shapes(structure_waves=nw))


def _al16(x):
    return (x + 15) & ~15


def _s1_tier(budget, amax, nw, km, cm):
    """The structure pass's LDS split as the host computes it (ctx.hpp s1_tier,
    estep_split.hip k1_plan): LDS states, key slots and contributions."""
    npm = amax * (amax + 1) // 2
    lid = nw <= 4
    for f in range(2048, 15, -16):
        h = max(16, km * f // 10)
        h = 1 << (h - 1).bit_length()
        c = max(16, cm * f // 10)
        b = (_al16((npm + 2) * 4 + 3 * npm) + _al16(NBUCKET_BYTES) + _al16((2 * nw + 4) * 8) + 3 * _al16(3 * f * 4)
             + _al16(h * (20 if lid else 16 + 8 * nw)) + _al16(64 * nw * nw * 8 if lid else 0) + _al16(3 * c * 4))
        if b <= budget:
            return f, h, c
    return 0, 16, 0


@pytest.mark.parametrize("nw,ipc", [(1, 20), (4, 8)])
@pytest.mark.parametrize("name", ["n300", "a4"])
def test_sweep_rounds_and_hbm_tiers(oracle_mod, name, nw, ipc):
    """A small LDS tier (a 20th / an 8th of the CU's LDS per block, and
    hmc_set_structure_tier at one key slot per ten states and 16 contributions
    per state, the largest share the contributions can take) and a small first
    state capacity (frontier_cap 8: the walk restarts with larger ones):
    frontiers pass the LDS tier of states, so the sweep's scan carries across
    rounds of the block and reads and writes HBM-tier states; the keys
    outnumber the 16 LDS slots, so the clear reaches HBM-tier slots.  `n300`
    (379 states at its widest locus) has more new states at a locus than one
    round of the block at one wave (64) and at four (256); `a4`, the
    multi-allelic panel, reaches 63 and checks the tiers only."""
    km, cm = 1, 160
    p = panel(name)
    fc, hc, cc = _s1_tier(160 * 1024 // ipc - 256, p.alleles.max() - ord("1") + 1, nw, km, cm)
    assert 16 <= fc <= 64 and hc == 16, (fc, hc, cc)

    def setup(m):
        m.set_pass_shapes(structure_waves=nw, structure_ipc=ipc)
        m.set_structure_tier(km, cm)
        m.set_tuning(frontier_cap=8)

    seen = []

    def after(m, p_):
        fr = m.estep_frontier()
        seen.append(fr["max_states"])

    _two_esteps(oracle_mod, name, setup, after)
    print(f"{name} {nw} waves: LDS tier {fc} states, {hc} key slots; largest frontiers {seen}", flush=True)
    assert seen[0] > fc and seen[0] > hc, (seen, fc, hc)  # E1 on M0: past the LDS tiers of states and of keys
    if name == "n300":  # (a4's frontiers end at 63 states: one round at any block width)
        assert seen[0] > 64 * nw, seen  # more new states at a locus than one round of the block


def test_counting_clears_slots(oracle_mod):
    """A record store too small for the panel (hmc_set_store_budgets): the
    individuals whose records do not fit walk on without writing records
    (`counting`) and are run again in later groups — their key slots must be
    cleared at every locus all the same."""
    passes = []

    def after(m, p_):
        passes.append(m.estep_split_stats()["structure_passes"])

    _two_esteps(oracle_mod, "n60", lambda m: m.set_store_budgets(record_bytes=1 << 16), after)
    assert passes[0] >= 2, passes  # E1's records (M0's large frontiers) do not fit one pass


@pytest.mark.parametrize("name", ["miss2", "n300"])
def test_windowed_checkpoints(oracle_mod, name):
    """Windows of 7 loci: every window ends in a checkpoint of the frontier the
    new tail left (LO, HI, NL) and the next one starts from it."""
    def after(m, p):
        assert m.estep_windows()["windows"] == -(-p.L // 7)

    _two_esteps(oracle_mod, name, lambda m: m.set_estep_windows("always", window_loci=7), after)


def test_prune_rerun(oracle_mod):
    """Prune mode (the panel of test_windowed_underflow_hands_over: forward
    likelihoods underflow on 2 500 i.i.d. loci): the re-run with extend()'s
    forward test reads the records the sweep wrote and clears the slots; LL
    (-inf) and the resolutions equal the reference's."""
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 2, (6, 2, 2500)) + ord("1")).astype(np.int32)
    o = oracle_mod.Oracle(a, "S" * 2500, sample_size=4, max_iter=3)
    r = o.run()
    m = hmc_amd.HaploModel()
    m.set_pass_shapes(structure_waves=4)
    m.sample_size = 4
    m.max_iteration = 3
    res = m.run(hmc_amd.GenoData(a, "S" * 2500))
    assert [x["ll"] for x in m.log] == r["ll"].tolist()
    assert np.array_equal(res, r["resolutions"])
    assert m.estep_split_stats()["n_fallback"] > 0


@pytest.mark.parametrize("nw", [1, 4])
@pytest.mark.parametrize("name", ["cfg1", "a3miss5"])
def test_exact_records(oracle_mod, name, nw):
    """The exact layout (contributions in extendAll order, then each pair's
    orientation count — from the register at a locus without a missing allele):
    E1 on M0, the exact M-step's table from those records, and the E-step on
    it.  `cfg1` is the exact M-step's smallest panel; `a3miss5` has the LDS
    pair list too."""
    p = panel(name)
    o = oracle_mod.Oracle(p.alleles, p.types, sample_size=10)
    m = gpu_model(p)
    m.exact_estimate = True
    m.set_pass_shapes(structure_waves=nw)
    o.find_patterns()
    m.find_patterns()
    for step in range(2):
        ll_g, H, re_g = m.resolve_all()
        o.reset_counters()
        assert_estep_equal(m, o, ll_g, o.resolve_all(), H, re_g)
        if step == 0:
            P_o, _ = o.estimate_patterns()
            P_g, _ = m.find_patterns()  # after an E-step: estimatePatterns
            assert P_g == P_o
            _assert_table_bits(m.patterns(), o.patterns())
    m.close()
