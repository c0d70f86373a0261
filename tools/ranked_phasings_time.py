"""Ranked phasings (hmc_ranked_phasings) at k = 1, 4, 8 and 16 (list widths 2,
4, 8, 16) next to hmc_map_phase from the same build over the same records.

Default: the 60 x 120 founder mosaic of tests/test_gpu_map_phase.py (3 alleles,
5 % missing, no missing allele at locus 0) after M0 + E1.
SLICE=n: instead, M0 + E1 on the first n individuals (hmc_set_shard) of the
bench's flagship panel (env CFG, default 3).

Per range (regular, extended), RUNS times (default 5) after one untimed call:
map_stats() of map_phase() and ranked_stats() of ranked_phasings(k); min /
median / max of every figure; the ratio of the sweeps' medians, the list
store's launches, the counts, and whether row 0 is map_phase's bytes.

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
KS = [int(x) for x in os.environ.get("KS", "1,4,8,16").split(",")]


def spread(rows, key):
    v = [r[key] for r in rows]
    return dict(min=min(v), median=statistics.median(v), max=max(v))


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
out.update(N=m.N, L=m.L, individuals=int(m.i1 - m.i0), patterns_m0=P0, frontier_max=int(m.frontier_max().max()))
for name, ext in (("regular", False), ("extended", True)):
    m.set_posterior_range(ext)
    ref = m.map_phase()  # untimed: allocations
    mp = []
    for _ in range(RUNS):
        m.map_phase()
        mp.append(m.map_stats())
    res = dict(map=dict(runs=mp, **{k: spread(mp, k) for k in ("structure_ms", "fb_ms", "sweep_ms")}))
    map_sweep = statistics.median(x["sweep_ms"] for x in mp)
    for k in KS:
        r = m.ranked_phasings(k)  # untimed: allocations
        rk = []
        for _ in range(RUNS):
            r = m.ranked_phasings(k)
            rk.append(m.ranked_stats())
        ok = r["status"] == 0
        res[f"k{k}"] = dict(
            runs=rk, **{f: spread(rk, f) for f in ("structure_ms", "fb_ms", "sweep_ms")},
            k_built=rk[-1]["k_built"], batches=rk[-1]["batches"], groups=rk[-1]["groups"],
            sweep_over_map_sweep=statistics.median(x["sweep_ms"] for x in rk) / map_sweep,
            status={s: int((r["status"] == s).sum()) for s in (0, 1, 2)},
            count=dict(min=int(r["count"][ok].min()), median=float(np.median(r["count"][ok]))) if ok.any() else None,
            covered=dict(min=float(r["prob"][ok].sum(axis=1).min()), median=float(np.median(r["prob"][ok].sum(axis=1))))
            if ok.any() else None,
            row0_is_map=bool(r["hap"][:, 0].tobytes() == ref["hap"].tobytes() and r["prob"][:, 0].tobytes() == ref["prob"].tobytes()
                             and r["status"].tobytes() == ref["status"].tobytes()))
    out[name] = res
print(json.dumps(out))
