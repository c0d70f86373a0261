"""Window phasings (hmc_window_phasings): device times of the call, next to the
only other route to the same numbers.

The panel of profiles/extended_range/ (cfg 2 with 2 % missing, 1 000 x 500)
after M0 + E1.  For window lengths 8, 16 and 32, windows tiling the panel,
k = 8: the call RUNS times (default 5) over the whole shard — structure_ms,
fb_ms and sweep_ms of every run, min / median / max — with the share of
(individual, window) pairs at status 4 and the widest NC that ran.

The comparison: hmc_haplotype_dosages fed the two-sided patterns of the rows
this call returned, which is already told the answer's support.  The rows are
individual-specific, so the route is one dosage call per individual with that
individual's patterns; it is timed over SUB individuals (default 50, evenly
spaced) and set against this call over the same SUB individuals, both summed
over RUNS runs' phases.  Also one dosage call over the union of the patterns of
UNION individuals (default 8) for all of them, against this call over those.

One JSON line on stdout."""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hmc_amd  # noqa: E402
from hmc_amd import _lib, synth  # noqa: E402

RUNS = int(os.environ.get("RUNS", "5"))
SUB = int(os.environ.get("SUB", "50"))
UNION = int(os.environ.get("UNION", "8"))
K = 8
PHASES = ("structure_ms", "fb_ms", "sweep_ms")


def spread(rows, key):
    v = [r[key] for r in rows]
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def row_patterns(out, q, start, length):
    """(start, A, B) of every real row of caller row q."""
    pats = []
    for w, (s, n) in enumerate(zip(start, length)):
        if out["status"][q, w] != 0:
            continue
        for r in range(int(out["count"][q, w])):
            pats.append((s, tuple(int(x) for x in out["hap"][q, w, r, 0, :n]), tuple(int(x) for x in out["hap"][q, w, r, 1, :n])))
    return pats


out = dict(lib=_lib.lib_identity(), runs=RUNS, k=K)
m = hmc_amd.HaploModel()
p = synth.config_panel(2, 0.02)
m.load(hmc_amd.GenoData.from_panel(p))
P0, _ = m.find_patterns()
m.resolve_all()
out.update(panel="synth.config_panel(2, 0.02)", N=m.N, L=m.L, patterns_m0=P0, frontier_max=int(m.frontier_max().max()))
who = [int(i) for i in np.linspace(0, m.N - 1, SUB).round()]
for n in (8, 16, 32):
    start = list(range(0, m.L - n + 1, n))
    length = [n] * len(start)
    m.window_phasings(start, length, K)  # untimed: allocations
    runs = []
    for _ in range(RUNS):
        full = m.window_phasings(start, length, K)
        runs.append(m.window_stats())
    rec = dict(windows=len(start), runs=runs, status4_share=float((full["status"] == 4).mean()),
               status_other=int(((full["status"] != 0) & (full["status"] != 4)).sum()), configs_built=runs[0]["configs_built"],
               n_spilled=runs[0]["n_spilled"], rows=int(full["count"].sum()), mean_n_config=float(full["n_config"].mean()),
               top_prob_mean=float(full["prob"][:, :, 0][full["status"] == 0].mean()),
               **{k: spread(runs, k) for k in PHASES})
    # the same SUB individuals through both routes
    m.window_phasings(start, length, K, who)
    sub_runs = []
    for _ in range(RUNS):
        sub = m.window_phasings(start, length, K, who)
        sub_runs.append(m.window_stats())
    rec["sub"] = dict(individuals=len(who), **{k: spread(sub_runs, k) for k in PHASES})
    per = [row_patterns(sub, q, start, length) for q in range(len(who))]
    route, mismatched = [], 0
    for _ in range(RUNS):
        tot = dict.fromkeys(PHASES, 0.0)
        slots = rounds = 0
        for q, i in enumerate(who):
            if not per[q]:
                continue
            d = m.haplotype_dosages([x[0] for x in per[q]], [x[1] for x in per[q]], [x[2] for x in per[q]], [i])
            st = m.dosage_stats()
            for k in PHASES:
                tot[k] += st[k]
            slots, rounds = max(slots, st["slots"]), max(rounds, st["rounds"])
            want = np.array([v * (0.5 if x[1] == x[2] else 1.0) for v, x in zip(d["dosage"][0], per[q])])
            got = np.concatenate([sub["prob"][q, w, :int(sub["count"][q, w])] for w in range(len(start)) if sub["status"][q, w] == 0])
            mismatched += int((want.tobytes() != got.tobytes()))
        route.append(tot)
    rec["dosage_route_per_individual"] = dict(calls=sum(1 for x in per if x), patterns=sum(len(x) for x in per), slots=slots,
                                              rounds=rounds, individuals_with_other_bytes=mismatched,
                                              **{k: spread(route, k) for k in PHASES})
    # one dosage call over the union of a few individuals' patterns
    few = who[:UNION]
    m.window_phasings(start, length, K, few)
    few_runs = []
    for _ in range(RUNS):
        m.window_phasings(start, length, K, few)
        few_runs.append(m.window_stats())
    union = sorted({x for q in range(len(few)) for x in per[q]})
    args = ([x[0] for x in union], [x[1] for x in union], [x[2] for x in union], few)
    m.haplotype_dosages(*args)
    un_runs = []
    for _ in range(RUNS):
        m.haplotype_dosages(*args)
        un_runs.append(m.dosage_stats())
    rec["union"] = dict(individuals=len(few), patterns=len(union), slots=un_runs[0]["slots"], rounds=un_runs[0]["rounds"],
                        window={k: spread(few_runs, k) for k in PHASES}, dosage={k: spread(un_runs, k) for k in PHASES})
    out[f"len{n}"] = rec
print(json.dumps(out))
