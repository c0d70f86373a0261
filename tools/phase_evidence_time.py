"""MAP phasing given phase sets (hmc_map_phase_given) next to hmc_map_phase of
the same build on the same individuals.

Default: the 60 x 120 founder mosaic of tests/test_gpu_map_phase.py (3 alleles,
5 % missing, no missing allele at locus 0) after M0 + E1.
SLICE=n: instead, M0 + E1 on the first n individuals (hmc_set_shard) of the
bench's flagship panel (env CFG, default 3).

Evidence: every individual's consecutive heterozygous loci in sets of three,
spelled from resolutions(), so every individual runs the constrained sweep.

Per range (regular, extended), RUNS times (default 5) after one untimed call:
given_stats() of map_phase_given() and map_stats() of map_phase(); min /
median / max of every figure; the ratio of the sweeps' medians; the statuses,
the smallest and median evidence, and how many answers differ from map_phase's.

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
    panel = synth.config_panel(cfg)
    a = np.asarray(panel.alleles)
    m.load(hmc_amd.GenoData.from_panel(panel))
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
rows = []
for q, i in enumerate(range(m.i0, m.i1)):
    g = a[i]
    het = np.nonzero((g[0] >= 0) & (g[1] >= 0) & (g[0] != g[1]))[0]
    for s in range(0, len(het), 3):
        rows += [(i, int(k), s // 3, int(res[q, 0, k])) for k in het[s:s + 3]]  # (resolutions() is shard-local)
E = np.asarray(rows, np.int64).reshape(-1, 4)
out.update(N=m.N, L=m.L, individuals=int(m.i1 - m.i0), patterns_m0=P0, frontier_max=int(m.frontier_max().max()),
           evidence_entries=len(E))
for name, ext in (("regular", False), ("extended", True)):
    m.set_posterior_range(ext)
    m.map_phase()  # untimed: allocations
    m.map_phase_given(E)
    gv, mp = [], []
    for _ in range(RUNS):
        r = m.map_phase_given(E)
        gv.append(m.given_stats())
        p = m.map_phase()
        mp.append(m.map_stats())
    ok = r["status"] == 0
    out[name] = dict(
        given=dict(runs=gv, **{k: spread(gv, k) for k in ("structure_ms", "fb_ms", "sweep_ms")}),
        map=dict(runs=mp, **{k: spread(mp, k) for k in ("structure_ms", "fb_ms", "sweep_ms")}),
        sweep_over_map_sweep=statistics.median(x["sweep_ms"] for x in gv) / statistics.median(x["sweep_ms"] for x in mp),
        n_constrained=gv[-1]["n_constrained"],
        status={k: int((r["status"] == k).sum()) for k in (0, 1, 2, 3)},
        evidence=dict(min=float(r["evidence"][ok].min()), median=float(np.median(r["evidence"][ok]))) if ok.any() else None,
        differs_from_map_phase=int((~unordered_equal(r["hap"], p["hap"]))[ok].sum()))
print(json.dumps(out))
