"""Haplotype dosages (hmc_haplotype_dosages): device times of the call.

The panel of profiles/extended_range/ (cfg 2 with 2 % missing, 1 000 x 500)
after M0 + E1.  Pattern set: one-sided patterns of length 8 on windows stepping
8, the window haplotypes of the first four individuals' resolutions (distinct
ones).  The call RUNS times (default 5) in both ranges at automatic slots and
at NS = 1, 4 and 8: structure_ms, fb_ms and sweep_ms of every run, min / median
/ max, and sweep time per pattern-locus (patterns x 8 loci); next to them
hmc_switch_posteriors' sweep on the same panel and process.  STEP=n moves the
windows by n loci instead (STEP=2: four times the patterns, each locus under
four windows' patterns, so every NS takes rounds).

One JSON line on stdout."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hmc_amd  # noqa: E402
from hmc_amd import _lib, synth  # noqa: E402

RUNS = int(os.environ.get("RUNS", "5"))
LEN, STEP, SEEDS = 8, int(os.environ.get("STEP", "8")), 4


def spread(rows, key):
    v = [r[key] for r in rows]
    return dict(min=min(v), median=statistics.median(v), max=max(v))


out = dict(lib=_lib.lib_identity(), runs=RUNS, window_step=STEP)
m = hmc_amd.HaploModel()
p = synth.config_panel(2, 0.02)
m.load(hmc_amd.GenoData.from_panel(p))
P0, _ = m.find_patterns()
m.resolve_all()
res = m.resolutions()
pats = sorted({(s, tuple(int(x) for x in res[i, side, s:s + LEN])) for i in range(SEEDS) for side in range(2)
               for s in range(0, m.L - LEN + 1, STEP)})
start, rows = [s for s, _ in pats], [h for _, h in pats]
out.update(panel="synth.config_panel(2, 0.02)", N=m.N, L=m.L, patterns_m0=P0, dosage_patterns=len(pats),
           pattern_loci=len(pats) * LEN)
for name, ext in (("regular", False), ("extended", True)):
    m.set_posterior_range(ext)
    m.switch_posteriors()  # untimed: allocations
    sw = []
    for _ in range(RUNS):
        s = m.switch_posteriors()
        sw.append(m.switch_stats())
    mode = dict(switch=dict(runs=sw, sites=len(s["status"]), **{k: spread(sw, k) for k in ("structure_ms", "fb_ms", "sweep_ms")}))
    for ns in (0, 1, 4, 8):
        m.set_dosage_tuning(ns, 0)
        m.haplotype_dosages(start, rows)  # untimed: allocations
        ds = []
        for _ in range(RUNS):
            d = m.haplotype_dosages(start, rows)
            ds.append(m.dosage_stats())
        mode["auto" if ns == 0 else f"ns{ns}"] = dict(
            runs=ds, slots=ds[0]["slots"], rounds=ds[0]["rounds"], n_spilled=ds[0]["n_spilled"],
            status_nonzero=int((d["status"] != 0).sum()), mean_dosage=float(d["dosage"].mean()),
            sweep_ns_per_pattern_locus={k: v * 1e6 / (len(pats) * LEN) for k, v in spread(ds, "sweep_ms").items()},
            **{k: spread(ds, k) for k in ("structure_ms", "fb_ms", "sweep_ms")})
    m.set_dosage_tuning(0, 0)
    out[name] = mode
print(json.dumps(out))
