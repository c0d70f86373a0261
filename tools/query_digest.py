"""SHA-256 of every output array of every posterior query, after M0 + E1.

Three panels, each in the regular and in the extended range:
  mosaic  the 60 x 120 founder mosaic of tools/map_phase_time.py (frontiers to
          890 states: the LDS and the device-memory frontier store in one launch);
  mc      the head_len 2 panel of tests/test_gpu_pair_posteriors.py, so the
          head-pattern spelling runs;
  mixed   the 12 x 1 200 mixed panel of tests/test_gpu_posteriors.py, whose
          regular range gives individuals up with status 1 and status 2.
Queries: genotype posteriors, genotype likelihoods, switch, pair, draws,
dosages, MAP, MAP given evidence, ranked at k = 1, 4, 8 and 16; the status
arrays are digested like the values.  The inputs are the ones the GPU tests
build: bits_patterns / panel_patterns (dosages), mosaic_evidence (evidence),
span_list(3) / all_pairs (pair queries), SEED (draws).

One line per array on stdout: panel range query.array sha256.  --json FILE
writes the same as {panel: {range: {query.array: sha256}}}; that file, made
from the commit before a change to the query kernels, is
tests/golden/query_digests.json (tests/test_gpu_query_digests.py)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import hmc_amd  # noqa: E402

DRAWS = 64
RANKED_KS = (1, 4, 8, 16)


def sha(x):
    x = np.ascontiguousarray(x)
    return hashlib.sha256(str((x.dtype.str, x.shape)).encode() + x.tobytes()).hexdigest()


def mosaic_case():
    from test_gpu_haplotype_dosages import bits_patterns
    from test_gpu_posteriors import BITS_SHAPE, mosaic_with_heads
    import pair_enumeration as pe
    a = mosaic_with_heads(*BITS_SHAPE, 3, 0.05, 7)
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * a.shape[2]))
    m.find_patterns()
    m.resolve_all()
    return m, a, pe.span_list(a, 3), bits_patterns(a)


def mc_case():
    from test_enumeration_oracle import build_panel, head_len
    from test_gpu_enumeration import gpu_model
    import dosage_enumeration as dn
    import pair_enumeration as pe
    a = build_panel("mc")
    m = gpu_model("mc", 4, a)
    m.find_patterns()
    assert m.head_len() == head_len("mc") == 2
    pt = m.patterns()
    m.resolve_all()
    return m, a, pe.all_pairs(a), dn.panel_patterns(a, pt, 2)


def mixed_case():
    from test_gpu_haplotype_dosages import bits_patterns
    from test_gpu_posteriors import MIXED_L, mixed_panel
    import pair_enumeration as pe
    a = mixed_panel(MIXED_L)
    m = hmc_amd.HaploModel()
    m.load(hmc_amd.GenoData(np.ascontiguousarray(a, np.int32), "S" * a.shape[2]))
    m.find_patterns()
    m.resolve_all()
    return m, a, pe.span_list(a, 2), bits_patterns(a)[:24]


def queries(m, a, pairs, pats):
    """{query.array: sha256} in the range the model is set to."""
    from test_gpu_haplotype_dosages import ask as ask_dosages
    from test_gpu_map_phase_given import mosaic_evidence
    from test_gpu_posterior_draws import SEED
    q = np.array(pairs, np.int32).reshape(-1, 3)
    E = mosaic_evidence(a, m.resolutions(), keep=lambda i: i % 3 != 0)
    outs = dict(genotype_posteriors=m.genotype_posteriors(), genotype_likelihoods=m.genotype_likelihoods(),
                switch=m.switch_posteriors(), pair=m.pair_posteriors(q[:, 0], q[:, 1], q[:, 2]),
                draws=m.posterior_draws(DRAWS, SEED), dosages=ask_dosages(m, pats), map=m.map_phase(),
                map_given=m.map_phase_given(E), map_given_none=m.map_phase_given([]))
    for k in RANKED_KS:
        outs[f"ranked{k}"] = m.ranked_phasings(k)
    if os.environ.get("QUERY_DIGEST_VERBOSE"):
        print({name: np.bincount(out["status"], minlength=3).tolist() for name, out in outs.items()}, file=sys.stderr)
    return {f"{name}.{field}": sha(arr) for name, out in outs.items() for field, arr in sorted(out.items())}


def digests():
    out = {}
    for panel, case in (("mosaic", mosaic_case), ("mc", mc_case), ("mixed", mixed_case)):
        m, a, pairs, pats = case()
        out[panel] = {}
        for rng, ext in (("regular", False), ("extended", True)):
            m.set_posterior_range(ext)
            out[panel][rng] = queries(m, a, pairs, pats)
        m.set_posterior_range(False)
    return out


if __name__ == "__main__":
    d = digests()
    for panel, ranges in d.items():
        for rng, rows in ranges.items():
            for name, h in rows.items():
                print(panel, rng, name, h)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
            f.write("\n")
