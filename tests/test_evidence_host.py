"""Host sanitizer job for hmc_map_phase_given (CPU only): the GPU-free host
code — the plan builder and the evidence file reader (hmc_amd/csrc/
evidence_plan.hpp) — built into a stand-alone program (tests/sanitize/
evidence_main.cpp) with -fsanitize=address,undefined and run over empty
evidence, single-locus sets, adjacent spans, spans that start below head_len,
interleaving, duplicates, seeded tables and malformed lines.  Any report ends
the run with a non-zero status."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plan_and_reader_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "evidence_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe, "tests/sanitize/evidence_main.cpp"]
    subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "sanitized evidence host checks ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
