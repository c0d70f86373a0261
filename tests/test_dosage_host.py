"""Host sanitizer job for hmc_haplotype_dosages (CPU only): the GPU-free host
code — the plan builder (hmc_amd/csrc/dosage_plan.hpp: slots, rounds, event
order) and hmc_resolve's haplotype-list parser (tools/hmc_hapfile.hpp) — built
into a stand-alone program (tests/sanitize/dosage_main.cpp) with
-fsanitize=address,undefined and run over seeded pattern sets and malformed
lists.  Any report ends the run with a non-zero status."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plan_and_parser_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dosage_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe, "tests/sanitize/dosage_main.cpp"]
    subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "sanitized dosage host checks ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
