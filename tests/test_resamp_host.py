"""The resampler's host plan (csrc/resamp_plan.h, the header csrc/resamp.hip compiles) on the CPU:
`make -C meteor-scatter_amd/csrc resamp_check` builds csrc/resamp_check.cpp with g++
-fsanitize=address,undefined, and the program (stand-alone, nothing preloaded) checks the refusals, the
output counts at the position limits, the branch / offset arithmetic for every coprime (L, M) with L <= 8,
M <= 9, the LDS layouts and the lane map, and the kernel's summation order in float64 against its counted
chain.  A sanitizer report aborts the program (-fno-sanitize-recover=all), which fails the test."""
import os
import shutil
import subprocess

import pytest

import resamp_ref as R
from meteorgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meteor-scatter_amd", "csrc")
EXE = os.path.join(CSRC, "build", "resamp_check_san")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed for the sanitizer build")


def test_host_plan_under_sanitizers():
    import fcntl
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    with open(os.path.join(CSRC, "build", ".resamp_check.lock"), "w") as lk:  # one build at a time (pytest-xdist)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", CSRC, "resamp_check"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), r.stdout
    heads = {ln.split()[1].rstrip(":") for ln in lines}
    assert {"refusals", "counts", "branches", "layout", "order"} <= heads, r.stdout
    # the program's geometry and chain per shape are the library's and the Python restatement's
    shapes = 0
    for ln in lines:
        if ln.startswith("ok layout "):
            L, M, ntaps = (int(v) for v in ln.split()[2].rstrip(":").split("/"))
            cfg = _lib.MsdResampCfg(_lib.DDC_REAL, L, M, ntaps, _lib.MSD_F64, 0, 0, 1, 1.0)
            assert float(ln.split("chain ")[1].split(",")[0]) == _lib.resamp_chain(cfg) == R.chain_py(False, L, M, ntaps), ln
            TM, G, K, I = R.plan(L, M, ntaps)
            assert f"TM {TM}, G {G}, K {K}, I {I}," in ln, ln
            shapes += 1
    assert shapes >= 10
