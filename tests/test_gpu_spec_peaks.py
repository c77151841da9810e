"""GPU: the point extraction (csrc/cluster.hip, msd_spec_peaks_f64*) on synthetic float64 spectrograms
against the numpy restatement of tests/cluster_ref.py (pinned to np.lexsort by tests/test_cluster_ref.py):
points, cells, npts and ncand bit-equal."""
import numpy as np
import pytest

import cluster_ref as R

pytestmark = pytest.mark.gpu

SX, SY = 496 / 145, 366 / 164


def _check(spec, frames, k_lo, k_hi, thr, cap, sx=SX, sy=SY):
    from meteorgpu import cluster
    spec = np.asarray(spec, np.float64)
    batch = spec if spec.ndim == 3 else spec[None]
    res = cluster.spec_peaks(batch, k_lo, k_hi, thr, sx, sy, max_points=cap, frames=frames)
    thrs = np.broadcast_to(np.asarray(thr, np.float64), (batch.shape[0],))
    out = []
    for m in range(batch.shape[0]):
        pts, cells, ncand = R.spec_peaks(batch[m], frames, k_lo, k_hi, thrs[m], sx, sy, cap)
        assert res.ncand[m] == ncand, (m, res.ncand[m], ncand)
        assert np.array_equal(res.cells[m], cells), m
        assert res.points[m].tobytes() == pts.tobytes(), m
        out.append(ncand)
    return out


def _padded(rng, K, frames, ld, k_lo, k_hi, levels):
    """values quantised to `levels` inside the window; NaN / 1e300 in the padding columns and 1e300 in the
    rows outside [k_lo, k_hi], none of which may ever be picked"""
    spec = rng.integers(0, levels, size=(K, ld)).astype(np.float64) if levels else rng.random((K, ld))
    spec[:k_lo] = 1e300
    spec[k_hi + 1:] = 1e300
    spec[::2, frames:] = np.nan
    spec[1::2, frames:] = 1e300
    return spec


def test_small_shape_3x5():
    rng = np.random.default_rng(1)
    spec = _padded(rng, 5, 5, 32, 1, 3, 4)  # a 3-bin x 5-frame window
    for cap in (1, 2, 7, 15, 512):
        for thr in (-1.0, 0.0, 1.0, 2.0, 3.0):
            _check(spec, 5, 1, 3, thr, cap)
    _check(spec, 0, 1, 3, 0.0, 4)  # no frames


@pytest.mark.parametrize("levels", [2, 3, 17, 0])
def test_reference_window_counts_around_the_cap(levels):
    """the real window: 164 bins x 145 frames inside K = 1025, ld = 160; candidate counts 0, below, at and
    above the cap, with ties straddling the cut when the values are quantised"""
    rng = np.random.default_rng(40 + levels)
    K, frames, ld, k_lo, k_hi = 1025, 145, 160, 328, 491
    spec = _padded(rng, K, frames, ld, k_lo, k_hi, levels)
    win = spec[k_lo:k_hi + 1, :frames]
    top = np.sort(win.reshape(-1))[::-1]
    seen = set()
    for cap in (500, 512):
        # thresholds that leave 0, a few, exactly cap (where the values allow) and many candidates
        for thr in (top[0], top[3], np.nextafter(top[cap - 1], -np.inf), top[cap], top[cap + 1], top[5000], -1.0):
            seen.add(_check(spec, frames, k_lo, k_hi, float(thr), cap)[0] - cap)
    assert any(d < -400 for d in seen) and any(d > 1000 for d in seen)
    if levels == 0:  # distinct values: the count below, at and just above the cap
        assert {-500, 0, 1} <= seen or {-512, 0, 1} <= seen
    _check(spec, frames, k_lo, k_hi, -1.0, 1)


def test_plateau_inf_nan_and_per_image_threshold():
    K, frames, ld, k_lo, k_hi = 40, 70, 96, 4, 35
    flat = np.full((K, ld), 2.5)
    assert _check(flat, frames, k_lo, k_hi, 1.0, 500) == [32 * 70]  # an all-equal plateau: the first 500 cells
    assert _check(flat, frames, k_lo, k_hi, 2.5, 500) == [0]        # equal to the threshold is not above it
    rng = np.random.default_rng(8)
    spec = _padded(rng, K, frames, ld, k_lo, k_hi, 5)
    spec[k_lo + 3, 10] = np.inf
    spec[k_lo + 4, 10] = np.nan
    spec[k_hi, frames - 1] = np.inf
    spec[k_lo, 0] = -np.inf
    spec[k_lo + 1, 0] = -0.0
    for thr in (-np.inf, -1.0, 0.0, 3.0, 4.0, 1e308, np.inf, np.nan):
        for cap in (1, 2, 100, 512):
            _check(spec, frames, k_lo, k_hi, thr, cap)
    batch = np.stack([spec, flat, _padded(rng, K, frames, ld, k_lo, k_hi, 0), spec])
    got = _check(batch, frames, k_lo, k_hi, np.array([3.0, 1.0, 0.9, -1.0]), 500)
    assert got[0] < got[3] and got[1] == 32 * 70
    _check(batch, frames, k_lo, k_hi, 0.5, 33, sx=1.0, sy=1.0)


def test_host_form_one_image():
    import ctypes as C
    from meteorgpu import _lib
    from meteorgpu.dsp import context
    ctx = context(0)
    rng = np.random.default_rng(4)
    K, frames = 20, 37
    spec = rng.integers(0, 6, size=(K, frames)).astype(np.float64)
    for cap, thr in ((512, 2.0), (50, 2.0), (50, 7.0)):
        xy, cell = np.full((cap, 2), -7.0), np.full(cap, -7, np.int32)
        n, nc = C.c_int32(-1), C.c_int32(-1)
        _lib.check(ctx.lib.msd_spec_peaks_f64(ctx.h, _lib.ptr(spec), K, frames, 3, 17, thr, SX, SY, cap, _lib.ptr(xy),
                                              _lib.ptr(cell), C.byref(n), C.byref(nc)))
        pts, cells, ncand = R.spec_peaks(spec, frames, 3, 17, thr, SX, SY, cap)
        assert (n.value, nc.value) == (len(cells), ncand)
        assert np.array_equal(cell[: n.value], cells) and xy[: n.value].tobytes() == pts.tobytes()
        assert (cell[n.value:] == -7).all()
