"""GPU parity of the trace collection of the windowed E-step (estep_trace_gc,
estep_split.hip): the backward walk that keeps the reached list entries as a
bitmap while they are more than 64 and as a sorted list, one entry per lane,
from then on, with the locus metadata loaded 64 loci at a time.  Every case
runs the E-step in forced windows and in the classic passes of the same
library and compares LL, R_E, samples, weights, resolutions and the
per-individual E-step results bit for bit.

The library counts what the collections of an E-step did
(HaploModel.collection_stats): the cases chosen for one path of the kernel
assert on those counts that the path was taken — the dense -> sparse switch
inside a collected window, whole windows written from bitmaps, lists from the
first locus on — so a panel that loses its property fails instead of passing
on another path.  (The CPU restatement does not expose the k-best links of a
locus, so the property cannot be read off it.)"""
import functools

import numpy as np
import pytest

from hmc_amd import synth

from test_gpu_parity import gpu_model, panel

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _panel(key):
    if key == "m40":  # the seeded founder mosaic of the window-length cases
        return synth.founder_mosaic(40, 200, A=2, seed=21)
    return panel(key)


def _estep(m):
    ll, H, re = m.resolve_all()
    al, w, tw = m.samples(H)
    er = m.estep_results()
    return (float(ll).hex(), re, H, al.tobytes(), w.tobytes(), float(tw).hex(), m.resolutions().tobytes(),
            tuple((k, er[k].tobytes()) for k in sorted(er)))


@functools.lru_cache(maxsize=None)
def _classic(key, S, model="MV", order=1):
    """The classic passes' E-step on the GPU's own M0 (computed once per panel, S and model)."""
    m = gpu_model(_panel(key), S, model=model, mc_order=order)
    m.set_estep_windows("never")
    m.find_patterns()
    out = _estep(m)
    assert m.estep_windows()["windows"] == 0
    m.close()
    return out


def _windowed(key, S, wl, model="MV", order=1):
    p = _panel(key)
    m = gpu_model(p, S, model=model, mc_order=order)
    m.set_estep_windows("always", wl)
    m.find_patterns()
    out = _estep(m)
    w = m.estep_windows()
    st = m.collection_stats()
    hl = m.head_len()
    m.close()
    assert w["windows"] == -(-(p.L + 1 - hl) // wl), w
    print(f"{key} S={S} wl={wl}: {w['windows']} windows, {st}", flush=True)
    return out, w, st


@pytest.mark.parametrize("wl", [63, 64, 65])
def test_metadata_batch_boundaries(wl):
    """Windows of 63, 64 and 65 loci (four windows of the 200 loci): a walk
    over two windows crosses the 64-locus metadata batches at every phase."""
    out, w, st = _windowed("m40", 10, wl)
    assert w["windows"] >= 3
    assert st["sparse_steps"] > 0
    assert out == _classic("m40", 10)


@pytest.mark.parametrize("wl", [1, 2])
def test_shortest_windows(wl):
    """Windows of one and two loci: mid - lo0 = 1 (one locus collected per
    launch, every predecessor through the boundary list) and 2."""
    out, w, st = _windowed("m40", 10, wl)
    assert out == _classic("m40", 10)


def test_dense_to_sparse_inside_a_window():
    """More than 64 list entries at the end of a window that coalesce to a
    list inside the collected window: bitmap loci above list loci in one
    compaction (the counts: switches inside a window, loci written from
    bitmaps, and list steps)."""
    out, w, st = _windowed("a3miss5", 10, 6)
    assert st["switches_in_window"] > 0 and st["dense_loci_written"] > 0 and st["sparse_steps"] > 0, st
    assert out == _classic("a3miss5", 10)


@pytest.mark.parametrize("key,S,wl", [("a8", 10, 3), ("a3miss5", 10, 2)])
def test_dense_for_whole_windows(key, S, wl):
    """Many alleles with missing data, short windows: the reached entries stay
    above 64 across whole collected windows, which are then written from
    bitmaps alone (more loci written from bitmaps than switches could leave)."""
    out, w, st = _windowed(key, S, wl)
    assert st["dense_loci_written"] > wl * st["switches_in_window"], st
    assert out == _classic(key, S)


@pytest.mark.parametrize("S,wl", [(1, 5), (40, 6)])
def test_sample_sizes(S, wl):
    """S = 1 (one entry per state: lists from the last locus on for small
    frontiers) and S = 40 (bit index t S + k with S above a mark word)."""
    out, w, st = _windowed("a3miss5", S, wl)
    assert st["dense_steps"] + st["sparse_steps"] > 0
    assert out == _classic("a3miss5", S)


def test_locus_marks_past_lds():
    """An individual without any genotype on 8 alleles per locus, patterns
    mined down to a low threshold: a frontier whose F x S marks exceed the
    largest LDS mark buffer (2 x 7 680 words per block), so its loci mark in
    global scratch while the other individuals' stay in LDS."""
    rng = np.random.default_rng(1)
    N, L, A = 100, 6, 8
    al = (rng.integers(0, A, size=(N, 2, L)) + ord("1")).astype(np.int32)
    al[0] = -1
    p = synth.Panel(al, "S" * L)
    outs = []
    for mode, wl in (("never", 0), ("always", 2)):
        m = gpu_model(p, min_freq_abs=0.3, max_pattern_len=L)
        m.set_estep_windows(mode, wl)
        m.find_patterns()
        outs.append(_estep(m))
        if mode == "always":
            st = m.collection_stats()
            print(m.estep_frontier(), st, flush=True)
            assert m.estep_frontier()["max_states"] * 10 > 32 * 7680
            assert m.estep_windows()["windows"] == 3 and st["dense_steps"] > 0
        m.close()
    assert outs[0] == outs[1]


def test_head_length_above_one():
    """MC order 2 (head_len 3): the first collected window starts at the head
    pairs, whose entries have no predecessor."""
    out, w, st = _windowed("n60", 10, 4, model="MC", order=2)
    assert out == _classic("n60", 10, model="MC", order=2)


def test_two_esteps_on_one_context():
    """E1 on M0 and E2 on M1 on one context, windowed against classic: the
    second E-step's collections run on the first one's scratch, node store
    and boundary lists."""
    p = _panel("miss2")
    outs = []
    for mode, wl in (("never", 0), ("always", 9)):
        m = gpu_model(p, 10)
        m.set_estep_windows(mode, wl)
        m.find_patterns()
        o = [_estep(m)]
        m.find_patterns()
        o.append(_estep(m))
        if mode == "always":
            assert m.estep_windows()["windows"] >= 3 and m.collection_stats()["sparse_steps"] > 0
        m.close()
        outs.append(o)
    assert outs[0][0] != outs[0][1]  # the two models differ
    assert outs[0] == outs[1]
