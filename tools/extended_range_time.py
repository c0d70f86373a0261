"""Posterior family, regular against extended range (hmc_set_posterior_range).

Default: the panel of profiles/posteriors/cfg2_miss2.json (cfg 2 with 2 %
missing) after M0 + E1; genotype and switch posteriors RUNS times (default 5)
in each range the loaded library has: structure_ms, fb_ms and the consumer's
ms of every run, and min / median / max.  HMC_AMD_LIB picks another build (the
parent commit's library has the regular range only), so the same command times
both sides of an A/B.

SLICE=n: instead, M0 + E1 on the first n individuals (hmc_set_shard) of the
bench's flagship panel (env CFG, default 3) and the number of individuals the
posterior family answers (status 0), gives up as unresolved (1) or as
subnormal (2) in each range, with the likelihood exponents of the slice.

One JSON line on stdout."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hmc_amd  # noqa: E402
from hmc_amd import _lib, synth  # noqa: E402

RUNS = int(os.environ.get("RUNS", "5"))
SLICE = int(os.environ.get("SLICE", "0"))
has_ext = hasattr(_lib.lib(), "hmc_set_posterior_range")
modes = [("regular", False)] + ([("extended", True)] if has_ext else [])


def spread(rows, key):
    v = [r[key] for r in rows]
    return dict(min=min(v), median=statistics.median(v), max=max(v))


out = dict(lib=_lib.lib_identity(), runs=RUNS)
m = hmc_amd.HaploModel()
if SLICE:
    cfg = int(os.environ.get("CFG", "3"))
    p = synth.config_panel(cfg)
    m.load(hmc_amd.GenoData.from_panel(p))
    t0 = time.perf_counter()
    P0, _ = m.find_patterns()
    m.set_shard(0, SLICE)
    t1 = time.perf_counter()
    m.resolve_all()
    t2 = time.perf_counter()
    er = m.estep_results()
    out.update(panel=f"synth.config_panel({cfg})", N=m.N, L=m.L, slice=SLICE, patterns_m0=P0, m0_wall_s=t1 - t0,
               e1_wall_s=t2 - t1, estep_unresolved=int((er["status"] != 0).sum()),
               estep_total_subnormal=int(((er["total"] > 0) & (er["total"] < 2.0 ** -1022)).sum()),
               estep_total_zero=int((er["total"] == 0).sum()))
    for name, ext in modes:
        if has_ext:
            m.set_posterior_range(ext)
        t0 = time.perf_counter()
        st = m.posterior_draws(1, 0)["status"]  # one status per individual
        sw = m.switch_posteriors()
        out[name] = dict(individuals={k: int((st == k).sum()) for k in (0, 1, 2)},
                         switch_sites={k: int((sw["status"] == k).sum()) for k in (0, 1, 2)},
                         draw_stats=m.draw_stats(), switch_stats=m.switch_stats(), wall_s=time.perf_counter() - t0)
    if has_ext:
        lk = m.genotype_likelihoods()
        out["likelihood_exponent"] = dict(min=int(lk["exponent"].min()), median=float(np.median(lk["exponent"])),
                                          max=int(lk["exponent"].max()), status_1=int((lk["status"] != 0).sum()),
                                          below_double_range=int((lk["exponent"] < -1022).sum()), stats=m.likelihood_stats())
else:
    p = synth.config_panel(2, 0.02)
    m.load(hmc_amd.GenoData.from_panel(p))
    P0, _ = m.find_patterns()
    m.resolve_all()
    out.update(panel="synth.config_panel(2, 0.02)", N=m.N, L=m.L, patterns_m0=P0)
    for name, ext in modes:
        if has_ext:
            m.set_posterior_range(ext)
        m.genotype_posteriors()  # untimed: allocations
        m.switch_posteriors()
        gp, sw = [], []
        for _ in range(RUNS):
            g = m.genotype_posteriors()
            gp.append(m.posterior_stats())
            s = m.switch_posteriors()
            sw.append(m.switch_stats())
        out[name] = dict(
            genotype=dict(runs=gp, **{k: spread(gp, k) for k in ("structure_ms", "fb_ms", "sites_ms")}),
            switch=dict(runs=sw, **{k: spread(sw, k) for k in ("structure_ms", "fb_ms", "sweep_ms")}),
            status_nonzero=dict(genotype=int((g["status"] != 0).sum()), switch=int((s["status"] != 0).sum())),
            sites=dict(genotype=len(g["status"]), switch=len(s["status"])))
print(json.dumps(out))
