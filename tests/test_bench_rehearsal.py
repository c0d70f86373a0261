"""bench.py's multi-rank path end to end on one GPU, with every rank on device
0 and the gloo host collective in place of RCCL (`--collective host`): the
driver's launch (`torch.distributed.run --nproc-per-node N bench.py --gpus N`)
and bench.py's own launch of N ranks when no launcher set WORLD_SIZE.  The
sharded EM with the ordered reduction must reproduce the one-rank chain
exactly (LL and pattern count of every step), and the timed steps must follow
the reference's converged chain (restart from M0 after the stop).  A plain run
reports only the headline; `--full` adds the steady leg, the CPU baseline and
the roofline blocks, and `--dump-outputs` writes the last timed step's outputs,
the same from run to run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--config", "2", "--steps", "4", "--warmup", "1", "--steady-steps", "0", "--no-cpu-baseline",
          "--trace-bytes", "16000000000"]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _last_json(out: str) -> dict:
    return json.loads(out.strip().splitlines()[-1])


def _run(cmd):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return _last_json(r.stdout)


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bench_dump")


@pytest.fixture(scope="module")
def one_rank(dump_dir):
    return _run([sys.executable, "bench.py", *COMMON, "--dump-outputs", str(dump_dir / "plain")])


def _load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_reports_the_headline_only(one_rank):
    assert one_rank["full"] is False
    for k in ("value_steady", "roofline", "roofline_iter", "cpu_baseline"):
        assert one_rank[k] is None, k
    assert one_rank["steps"] == 4 and len(one_rank["per_step"]) == 4
    assert one_rank["ms_per_step"] > 0
    assert one_rank["value"] == pytest.approx(1000 * 500 / (one_rank["ms_per_step"] / 1e3), rel=1e-9)
    # the E-steps the process ran: warmup + timed steps, nothing else
    assert len(one_rank["run_estep_log"]) == 1 + 4


def test_bench_dump_outputs_are_the_last_timed_step(one_rank, dump_dir):
    d = _load_dump(dump_dir / "plain")
    with open(dump_dir / "plain" / "manifest.json") as f:
        man = json.load(f)
    assert set(man["arrays"]) == set(d)
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    col = {c: i for i, c in enumerate(man["iter_log_columns"])}
    log = d["iter_log"]
    assert log.shape == (4, len(col))
    assert log[:, col["iteration"]].tolist() == [1, 2, 3, 1]
    assert log[:, col["log_likelihood"]].tolist() == pytest.approx([s["ll"] for s in one_rank["per_step"]], abs=1e-6)
    assert log[:, col["r_e"]].tolist() == [s["r_e"] for s in one_rank["per_step"]]
    # the last step is E1 + M1: all 1000 individuals' E-step, the resolutions phase
    # the genotypes' allele symbols, and the table sample is of M1's table
    assert d["estep_total"].shape == (1000,) and d["estep_posterior"].shape == (1000, 10)
    assert np.all(d["estep_ncand"] >= 1)
    w = d["estep_weight"].sum(axis=1)
    assert np.allclose(w, 1.0, rtol=0, atol=1e-9)
    assert d["resolutions"].shape == (1000, 2, 500) and d["resolutions_rows"].tolist() == list(range(1000))
    assert set(np.unique(d["resolutions"])) <= {float(ord("1")), float(ord("2"))}
    assert man["patterns"] == one_rank["per_step"][3]["P"]
    assert len(d["pattern_rows"]) == min(man["patterns"], 1 << 18)
    assert np.all(d["pattern_freq"] > 0) and np.all(d["pattern_len"] >= 1)


def test_bench_full_adds_the_legs_and_repeats_the_outputs(one_rank, dump_dir):
    """--full with the same steps: the steady leg, the sampled CPU baseline and
    the roofline blocks are there, and the dumped outputs equal the plain run's
    bit for bit (same inputs from run to run; later legs do not reach them)."""
    full = _run([sys.executable, "bench.py", "--full", "--config", "2", "--steps", "4", "--warmup", "1",
                 "--steady-steps", "2", "--cpu-indiv", "4", "--cpu-indiv-e1", "4", "--cpu-roots", "4",
                 "--trace-bytes", "16000000000", "--dump-outputs", str(dump_dir / "full")])
    assert full["full"] is True
    assert full["value_steady"]["iterations"] == [4, 5]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
    r = full["roofline"]
    assert r["kernel"] == "estep_values" and r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-12)
    assert full["roofline_iter"]["bytes_per_iter"] > 0
    assert [(s["ll"], s["P"]) for s in full["per_step"]] == [(s["ll"], s["P"]) for s in one_rank["per_step"]]
    a, b = _load_dump(dump_dir / "plain"), _load_dump(dump_dir / "full")
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_bench_steps_follow_the_converged_chain(one_rank):
    # cfg 2 stops after E3 (LL rises, then drops at iteration 3)
    assert [s["iteration"] for s in one_rank["per_step"]] == [1, 2, 3, 1]
    assert [s["go"] for s in one_rank["per_step"]] == [True, True, False, True]
    assert one_rank["per_step"][2]["mstep_ms"] == 0.0
    assert one_rank["per_step"][3]["ll"] == one_rank["per_step"][0]["ll"]  # the restart is E1 again
    assert one_rank["chain"]["iterations"] == [3]
    assert one_rank["library"]["path"].endswith("libhmc_amd.so")


def test_bench_two_ranks_equal_one(one_rank):
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
                *COMMON, "--collective", "host"])
    assert one_rank["n_gpus"] == 1 and two["n_gpus"] == 2
    assert "REHEARSAL" in two["config"]["parallelism"]
    assert [(s["ll"], s["P"]) for s in two["per_step"]] == [(s["ll"], s["P"]) for s in one_rank["per_step"]]
    assert two["m0"]["patterns"] == one_rank["m0"]["patterns"]


def test_bench_spawns_ranks_without_launcher(one_rank):
    """`python bench.py --gpus 2` with no WORLD_SIZE: bench.py starts the two
    ranks itself (fresh processes, before any GPU call)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", *COMMON, "--collective", "host"], cwd=ROOT,
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    two = _last_json(r.stdout)
    assert two["n_gpus"] == 2
    assert [(s["ll"], s["P"]) for s in two["per_step"]] == [(s["ll"], s["P"]) for s in one_rank["per_step"]]


def test_bench_rejects_gpus_world_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", *COMMON], cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 2
