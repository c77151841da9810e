"""The pruned transform of the whole-band Welch row (csrc/welch_fft_plan.h, the header
csrc/welch_fft.hip compiles) on the CPU: `make -C meteor-scatter_amd/csrc welch_fft_check` builds
csrc/welch_fft_check.cpp with g++ -fsanitize=address,undefined, and the program runs the plan -- the
table of roots, the modulation, the fold, the Stockham passes, the bin ownership -- in float64 against a
long-double DFT for every (nperseg, nfft) of tests/welch_fft_signals.py and the plan's corners.
A sanitizer report aborts the program (-fno-sanitize-recover=all), which fails the test."""
import os
import shutil
import subprocess

import pytest

import welch_fft_signals as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meteor-scatter_amd", "csrc")
EXE = os.path.join(CSRC, "build", "welch_fft_check_san")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed for the sanitizer build")


def test_pruned_transform_against_long_double():
    import fcntl
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    with open(os.path.join(CSRC, "build", ".welch_fft_check.lock"), "w") as lk:  # one build at a time (pytest-xdist)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", CSRC, "welch_fft_check"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), r.stdout
    done = {ln.split()[1].rstrip(":") for ln in lines}
    for (_, nper, _, nfft), _ in W.SHAPES:  # every shape of the GPU test's table
        assert f"{nper}/{nfft}" in done, (nper, nfft, r.stdout)
    # the program's chain is the transform's part of the helper's: without the sample_scale product,
    # the detrend and the window (4)
    for ln in lines:
        nper, nfft = (int(v) for v in ln.split()[1].rstrip(":").split("/"))
        assert float(ln.split("chain ")[1].split(",")[0]) == W.chain(nper, nfft) - 4, ln
