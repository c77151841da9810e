"""The down-converter's host plan (csrc/ddc_plan.h, the header csrc/ddc.hip compiles) on the CPU:
`make -C meteor-scatter_amd/csrc ddc_check` builds csrc/ddc_check.cpp with g++ -fsanitize=address,undefined,
and the program checks the refusals, r(n) at n = 2^62 and q = 2^24 - 3, the phase tables against long
double, the polyphase layout, the output counts at every pos0 mod D, and the kernel's summation order in
float64 against its counted chain.  A sanitizer report aborts the program (-fno-sanitize-recover=all), which
fails the test."""
import os
import shutil
import subprocess

import pytest

from meteorgpu import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meteor-scatter_amd", "csrc")
EXE = os.path.join(CSRC, "build", "ddc_check_san")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed for the sanitizer build")


def test_host_plan_under_sanitizers():
    import fcntl
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    with open(os.path.join(CSRC, "build", ".ddc_check.lock"), "w") as lk:  # one build at a time (pytest-xdist)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", CSRC, "ddc_check"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), r.stdout
    heads = {ln.split()[1].rstrip(":") for ln in lines}
    assert {"refusals", "phase", "tables", "layout", "counts", "order"} <= heads, r.stdout
    # the program's chain per shape is the library's (REAL: the layout lines)
    for ln in lines:
        if ln.startswith("ok layout "):
            D, ntaps = (int(v) for v in ln.split()[2].rstrip(":").split("/"))
            cfg = _lib.MsdDdcCfg(_lib.DDC_REAL, D, ntaps, _lib.MSD_F64, 0, 1, 1.0)
            assert float(ln.split("chain ")[1]) == _lib.ddc_chain(cfg), ln
