"""bench.py's command line: what the argument parser refuses (CPU, before anything touches a
GPU), and on the GPU the plain run against --full and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DUMPED = ("delta", "thresholds", "detection_counts", "detections", "hour_counts", "spectrogram", "spectrogram_files")


def _run(*args, timeout=120):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MSD_RDZV_KEY"):
        e.pop(k, None)
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout,
                          env=e, cwd=ROOT)


@pytest.mark.parametrize("args, text", [
    (("--workload", "c5", "--dump-outputs", "x"), "--dump-outputs"),
    (("--steps", "0"), "--steps"),
])
def test_refused_arguments(args, text):
    r = _run(*args)
    assert r.returncode == 2 and text in r.stderr and not r.stdout
    assert not os.path.exists(os.path.join(ROOT, "x"))


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeat(tmp_path):
    """a plain run carries the headline alone (what --full adds is absent), --steps sets the timed
    steps, and two runs with the same arguments dump identical outputs of the expected shapes"""
    common = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--files", "9")
    d = _line(_run(*common, "--dump-outputs", str(tmp_path / "a")))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["roofline"]["frac"] > 0 and d["config"]["files_per_gpu"] == 9
    for k in ("cpu_baseline", "cpu_baseline_multicore", "c5", "live", "strong_scaling", "kernel_ms_per_step"):
        assert k not in d, k
    _line(_run(*common, "--dump-outputs", str(tmp_path / "b")))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in DUMPED)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in DUMPED}
    total = 0
    for n in DUMPED:
        assert a[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(a[n], np.load(tmp_path / "b" / (n + ".npy")), equal_nan=True), n
        assert d["dumped"][n] == list(a[n].shape)
        total += a[n].nbytes
    assert total <= 64 * 10 ** 6
    K, T, nb = d["config"]["bins"], d["config"]["frames_per_file"], 60 * 5
    assert a["delta"].shape == a["thresholds"].shape == (9, nb) and np.isfinite(a["delta"]).all()
    assert a["spectrogram"].dtype == np.float32 and a["spectrogram"].shape == (len(a["spectrogram_files"]), K, T)
    assert (a["spectrogram"] > 0).all() and len(a["spectrogram_files"]) >= 1
    assert a["detections"].shape == (int(a["detection_counts"].sum()), 4) and a["detection_counts"].shape == (9,)
    assert a["hour_counts"].sum() == a["detection_counts"].sum() == d["detections_per_step"] > 0
