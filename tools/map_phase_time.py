"""MAP phasing (hmc_map_phase) next to the forward-only scaled pass over the
same records (hmc_genotype_likelihoods), the nearest existing cost.

Default: the 60 x 120 founder mosaic of tests/test_gpu_map_phase.py (3 alleles,
5 % missing, no missing allele at locus 0) after M0 + E1.
SLICE=n: instead, M0 + E1 on the first n individuals (hmc_set_shard) of the
bench's flagship panel (env CFG, default 3).

Per range (regular, extended), RUNS times (default 5) after one untimed call:
map_stats() of map_phase() and likelihood_stats() of genotype_likelihoods()
for the same individuals; min / median / max of every figure; the statuses,
the smallest and median prob, and how many MAP pairs differ from resolutions().

One JSON line on stdout."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hmc_amd  # noqa: E402
from hmc_amd import _lib, synth  # noqa: E402

RUNS = int(os.environ.get("RUNS", "5"))
SLICE = int(os.environ.get("SLICE", "0"))


def spread(rows, key):
    v = [r[key] for r in rows]
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def unordered_equal(x, y):
    return (x == y).all(axis=(1, 2)) | (x == y[:, ::-1]).all(axis=(1, 2))


out = dict(lib=_lib.lib_identity(), runs=RUNS)
m = hmc_amd.HaploModel()
if SLICE:
    cfg = int(os.environ.get("CFG", "3"))
    m.load(hmc_amd.GenoData.from_panel(synth.config_panel(cfg)))
    P0, _ = m.find_patterns()
    m.set_shard(0, SLICE)
    out.update(panel=f"synth.config_panel({cfg})", slice=SLICE)
else:
    N, L = 60, 120
    a = synth.founder_mosaic(N, L, A=3, missing=0.05, seed=7).alleles.copy()
    a[:, :, :1] = synth.founder_mosaic(N, L, A=3, missing=0.0, seed=7).alleles[:, :, :1]
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * L))
    P0, _ = m.find_patterns()
    out.update(panel="founder mosaic 60 x 120, A = 3, 5 % missing, seed 7")
m.resolve_all()
res = m.resolutions()
out.update(N=m.N, L=m.L, individuals=int(m.i1 - m.i0), patterns_m0=P0, frontier_max=int(m.frontier_max().max()))
for name, ext in (("regular", False), ("extended", True)):
    m.set_posterior_range(ext)
    m.map_phase()  # untimed: allocations
    m.genotype_likelihoods()
    mp, lk = [], []
    for _ in range(RUNS):
        r = m.map_phase()
        mp.append(m.map_stats())
        m.genotype_likelihoods()
        lk.append(m.likelihood_stats())
    ok = r["status"] == 0
    out[name] = dict(
        map=dict(runs=mp, **{k: spread(mp, k) for k in ("structure_ms", "fb_ms", "sweep_ms")}),
        likelihood=dict(runs=lk, **{k: spread(lk, k) for k in ("structure_ms", "fb_ms")}),
        sweep_over_forward=statistics.median(x["sweep_ms"] for x in mp) / statistics.median(x["fb_ms"] for x in lk),
        status={k: int((r["status"] == k).sum()) for k in (0, 1, 2)},
        prob=dict(min=float(r["prob"][ok].min()), median=float(np.median(r["prob"][ok]))) if ok.any() else None,
        map_differs_from_resolutions=int((~unordered_equal(r["hap"], res))[ok].sum()))
print(json.dumps(out))
