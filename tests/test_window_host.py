"""Host sanitizer job for hmc_window_phasings (CPU only): the GPU-free host code
— the configuration plan (hmc_amd/csrc/window_plan.hpp: C against brute force,
decode o encode = identity, swap an involution, the canonical order total) and
hmc_resolve's window-list parser (tools/hmc_winfile.hpp) — built into a
stand-alone program (tests/sanitize/window_main.cpp) with
-fsanitize=address,undefined and run over seeded genotypes and malformed
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
    exe = str(tmp_path / "window_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", exe, "tests/sanitize/window_main.cpp"]
    subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "sanitized window host checks ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
