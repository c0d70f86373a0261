"""The statistics of the eight posterior queries (hmc_last_*_stats) on the GPU:
each query kind has a record of its own.  Another kind's call leaves it alone,
although all eight run the same pass over the shard (xp_pass), and so does a
call that fails on its arguments, its own kind's included: a record is zeroed
only once a call's arguments have been accepted.  The records are stored
numbers, so the comparisons are exact."""
import numpy as np
import pytest

import hmc_amd
from hmc_amd._lib import HMCError

from test_gpu_posteriors import large_model, mosaic_with_heads

pytestmark = pytest.mark.gpu
SHAPE = (12, 24)


def queries(m, a):
    """(name, call, stats) of the eight queries with small arguments."""
    pq = m.pair_span_list(2)
    n = min(len(pq["indiv"]), 9)
    assert n > 0
    pq = {k: v[:n] for k, v in pq.items()}
    row = a[0, 0]
    starts, pats = [0, 5], [row[0:3].tolist(), row[5:9].tolist()]
    return [
        ("genotype", m.genotype_posteriors, m.posterior_stats),
        ("switch", m.switch_posteriors, m.switch_stats),
        ("pair", lambda: m.pair_posteriors(pq["indiv"], pq["locus_a"], pq["locus_b"]), m.pair_stats),
        ("draws", lambda: m.posterior_draws(4, 11), m.draw_stats),
        ("likelihoods", m.genotype_likelihoods, m.likelihood_stats),
        ("dosages", lambda: m.haplotype_dosages(starts, pats), m.dosage_stats),
        ("map", m.map_phase, m.map_stats),
        ("ranked", lambda: m.ranked_phasings(2), m.ranked_stats),
    ]


def test_a_querys_stats_are_its_own():
    N, L = SHAPE
    a = mosaic_with_heads(N, L, 3, 0.05, 7)
    m = large_model(a)  # M0 + E1
    qs = queries(m, a)
    taken = {}
    for name, call, stats in qs:
        call()
        taken[name] = stats()
        assert taken[name]["groups"] >= 1 and taken[name]["structure_ms"] > 0 and taken[name]["fb_ms"] > 0, (name, taken[name])
    assert taken["pair"]["slots"] >= 1 and taken["dosages"]["slots"] >= 1 and taken["dosages"]["rounds"] >= 1
    assert taken["ranked"]["k_built"] >= 2 and taken["ranked"]["batches"] >= 1
    for name, _, stats in qs:
        assert stats() == taken[name], name
    # calls that fail on their arguments: no record changes, the failing kind's included
    for bad in (lambda: m.posterior_draws(0, 11), lambda: m.ranked_phasings(17), lambda: m.map_phase(indiv=[N]),
                lambda: m.genotype_likelihoods(indiv=[-1]), lambda: m.haplotype_dosages([L], [[1]])):
        with pytest.raises(HMCError):
            bad()
        for name, _, stats in qs:
            assert stats() == taken[name], name
    # and a second round of calls gives every kind a fresh record of the same counts
    for name, call, stats in qs:
        call()
        again = stats()
        for k, v in taken[name].items():
            if not k.endswith("_ms"):
                assert again[k] == v, (name, k)
