"""The STFT kernels' butterflies (csrc/fft_butterfly.h, the header stft.hip, stft1024.hip and
cstft.hip compile) on the CPU: `make -C meteor-scatter_amd/csrc butterfly` builds
csrc/butterfly_check.cpp with g++ -fsanitize=address,undefined, and the program compares dft8 and
dft8_windowed with a long-double 8-point DFT on 10 000 random inputs and the unit vectors (4 float ulp
of the input norm per output), dft4 and dft16 with the 4- and 16-point DFT (2 and 14 ulp, the bounds
its header derives from their roundings).
A sanitizer report aborts the program (-fno-sanitize-recover=all), which fails the test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meteor-scatter_amd", "csrc")
EXE = os.path.join(CSRC, "build", "butterfly_check_san")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed for the sanitizer build")


def test_dft8_against_long_double():
    import fcntl
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    with open(os.path.join(CSRC, "build", ".butterfly.lock"), "w") as lk:  # one build at a time (pytest-xdist)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", CSRC, "butterfly"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "10000", "1"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("ok 10000 random + 16 unit inputs"), r.stdout
    assert lines[1].startswith("ok 10000 random + 32 unit inputs: worst error dft4") and "dft16" in lines[1], r.stdout
