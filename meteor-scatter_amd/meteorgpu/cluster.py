"""Time-frequency burst clustering (include/msdsp.h a11, csrc/cluster.hip): the DBSCAN stage of
meteor_detect_class/detector_and_classification.py:7-91 on the GPU, one workgroup per image.

    labels = dbscan(points)                                  # DBSCAN(eps=30, min_samples=5).fit(points).labels_
    res = cluster_points([points_a, points_b, ...])          # a batch: labels, boxes, critical / non-critical ids
    pk = spec_peaks(spec, k_lo, k_hi, thr, sx, sy)           # the points of a float64 spectrogram above a floor

``dbscan`` and ``cluster_points`` give sklearn's ``labels_`` exactly (tests/test_cluster_ref.py pins the
restatement to sklearn, tests/test_gpu_cluster.py the kernel to the restatement), the boxes
``(x_min, y_min, x_max, y_max)`` of :44-46 and the critical rule ``x_max - x_min >= 5`` of :48-50.
``spec_peaks`` stands where the reference runs ORB on the rendered JPEG (:12-16), which cannot be
reproduced; its points are the cells above the colour floor, so counts downstream differ from the
reference's even though the clustering is the reference's.  numpy only; all arithmetic is the library's.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .dsp import context

MAX_POINTS = _lib.CLUSTER_MAX_POINTS
DEFAULT_EPS = 30.0           # detector_and_classification.py:7
DEFAULT_MIN_SAMPLES = 5      # :7
CRITICAL_MIN_EXTENT = 5.0    # :50 ("entspricht ca. 0.5s")
ORB_NFEATURES = 500          # :12


@dataclass
class ClusterResult:
    """Per image: ``labels`` int32 [n] (-1 noise), ``boxes`` float64 [n_clusters][4] =
    (x_min, y_min, x_max, y_max), ``critical`` / ``non_critical`` the cluster ids on either side of the
    extent rule; ``summary`` the kernel's own counts (``_lib.CLUSTER_SUMMARY_DTYPE`` [nimg])."""
    labels: list = field(default_factory=list)
    boxes: list = field(default_factory=list)
    critical: list = field(default_factory=list)
    non_critical: list = field(default_factory=list)
    summary: np.ndarray | None = None


@dataclass
class PeaksResult:
    """Per image: ``points`` float64 [npts][2] = (t sx, (k - k_lo) sy) in cell order, ``cells`` int32 [npts]
    (c = t nk + k - k_lo); ``ncand`` int32 [nimg] the candidates before the cut to ``max_points``."""
    points: list = field(default_factory=list)
    cells: list = field(default_factory=list)
    ncand: np.ndarray | None = None


def _cfg(eps, min_samples, critical_min_extent, max_points) -> _lib.MsdClusterCfg:
    return _lib.MsdClusterCfg(float(eps), float(critical_min_extent), int(min_samples), int(max_points))


def _split(labels, boxes, summary, critical_min_extent) -> ClusterResult:
    res = ClusterResult(summary=summary)
    for m in range(summary.shape[0]):
        s = summary[m]
        if s["status"] != 0:
            raise _lib.MsdError(_lib.MSD_ERR_UNSUPPORTED, f"cluster: image {m} holds more points than max_points")
        nc = int(s["n_clusters"])
        b = boxes[m, :nc].copy()
        crit = (b[:, 2] - b[:, 0]) >= float(critical_min_extent)
        res.labels.append(labels[m, : int(s["n_points"])].copy())
        res.boxes.append(b)
        res.critical.append(np.nonzero(crit)[0].astype(np.int32))
        res.non_critical.append(np.nonzero(~crit)[0].astype(np.int32))
    return res


def cluster_dev(ctx: _lib.Context, d_xy: _lib.DeviceBuffer, d_npts: _lib.DeviceBuffer, nimg: int, max_points: int,
                eps=DEFAULT_EPS, min_samples=DEFAULT_MIN_SAMPLES,
                critical_min_extent=CRITICAL_MIN_EXTENT) -> ClusterResult:
    """msd_cluster_dev over points already on the device (xy float64 [nimg][max_points][2], npts int32
    [nimg], e.g. as msd_spec_peaks_f64_dev left them), then one download of labels, boxes and summaries."""
    cfg = _cfg(eps, min_samples, critical_min_extent, max_points)
    nimg, mp = int(nimg), int(max_points)
    d_lab = ctx.alloc(max(nimg * mp * 4, 8))
    d_box = ctx.alloc(max(nimg * mp * 32, 8))
    d_sum = ctx.alloc(max(nimg * _lib.CLUSTER_SUMMARY_DTYPE.itemsize, 8))
    _lib.check(ctx.lib.msd_cluster_dev(ctx.h, C.byref(cfg), d_xy.ptr, d_npts.ptr, nimg, d_lab.ptr, d_box.ptr,
                                       d_sum.ptr))
    labels = np.empty((nimg, mp), np.int32)
    boxes = np.empty((nimg, mp, 4), np.float64)
    summary = np.empty(nimg, _lib.CLUSTER_SUMMARY_DTYPE)
    if nimg:
        d_lab.download(labels)
        d_box.download(boxes)
        d_sum.download(summary)
    for d in (d_lab, d_box, d_sum):
        d.free()
    return _split(labels, boxes, summary, critical_min_extent)


def cluster_points(points_list, eps=DEFAULT_EPS, min_samples=DEFAULT_MIN_SAMPLES,
                   critical_min_extent=CRITICAL_MIN_EXTENT, max_points: int | None = None,
                   device: int = 0) -> ClusterResult:
    """DBSCAN, boxes and the critical rule over a batch of images in one launch.  ``points_list``: one
    float [n][2] array of (x, y) per image, n <= ``max_points`` (default: the largest n, at least 1) <= 512;
    more points in an image are refused, never clamped."""
    pts = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 2) for p in points_list]
    nimg = len(pts)
    if max_points is None:
        max_points = max([1] + [p.shape[0] for p in pts])
    mp = int(max_points)
    cfg = _cfg(eps, min_samples, critical_min_extent, mp)
    ctx = context(device)
    if nimg == 0 or not 1 <= mp <= MAX_POINTS:  # the library's refusals, with its codes and messages
        _lib.check(ctx.lib.msd_cluster_dev(ctx.h, C.byref(cfg), None, None, 0, None, None, None))
        return ClusterResult(summary=np.empty(0, _lib.CLUSTER_SUMMARY_DTYPE))
    for m, p in enumerate(pts):
        if p.shape[0] > mp:
            raise _lib.MsdError(_lib.MSD_ERR_UNSUPPORTED, f"cluster_points: image {m} holds {p.shape[0]} points, "
                                                          f"above max_points = {mp}")
        if not np.isfinite(p).all():
            raise _lib.MsdError(_lib.MSD_ERR_INVALID, f"cluster_points: image {m} holds a non-finite point")
    xy = np.zeros((nimg, mp, 2), np.float64)
    npts = np.empty(nimg, np.int32)
    for m, p in enumerate(pts):
        xy[m, : p.shape[0]] = p
        npts[m] = p.shape[0]
    d_xy, d_n = ctx.alloc(xy.nbytes), ctx.alloc(max(npts.nbytes, 8))
    d_xy.upload(xy)
    d_n.upload(npts)
    try:
        return cluster_dev(ctx, d_xy, d_n, nimg, mp, eps, min_samples, critical_min_extent)
    finally:
        d_xy.free()
        d_n.free()


def dbscan(points, eps=DEFAULT_EPS, min_samples=DEFAULT_MIN_SAMPLES, device: int = 0) -> np.ndarray:
    """``sklearn.cluster.DBSCAN(eps, min_samples).fit(points).labels_`` for up to 512 points [n][2], through
    the one-image host form msd_cluster."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n = p.shape[0]
    ctx = context(device)
    cfg = _cfg(eps, min_samples, CRITICAL_MIN_EXTENT, min(max(n, 1), MAX_POINTS))
    labels = np.empty(n, np.int32)
    s = _lib.MsdClusterSummary()
    _lib.check(ctx.lib.msd_cluster(ctx.h, C.byref(cfg), _lib.ptr(p), n, _lib.ptr(labels), None, C.byref(s)))
    return labels


def peaks_dev(ctx: _lib.Context, d_spec: _lib.DeviceBuffer, nimg: int, K: int, frames: int, ld: int, k_lo: int,
              k_hi: int, thr, sx: float, sy: float, max_points: int):
    """msd_spec_peaks_f64_dev over spectrograms on the device; the points stay there.  Returns
    (d_xy, d_cell, d_npts, d_ncand): float64 [nimg][max_points][2], int32 [nimg][max_points], int32 [nimg] x 2."""
    nimg, mp = int(nimg), int(max_points)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, np.float64), (nimg,)))
    d_thr = ctx.alloc(max(t.nbytes, 8))
    if nimg:
        d_thr.upload(t)
    d_xy, d_cell = ctx.alloc(max(nimg * mp * 16, 8)), ctx.alloc(max(nimg * mp * 4, 8))
    d_npts, d_ncand = ctx.alloc(max(nimg * 4, 8)), ctx.alloc(max(nimg * 4, 8))
    try:
        _lib.check(ctx.lib.msd_spec_peaks_f64_dev(ctx.h, d_spec.ptr, nimg, int(K), int(frames), int(ld), int(k_lo),
                                                  int(k_hi), d_thr.ptr, float(sx), float(sy), mp, d_xy.ptr,
                                                  d_cell.ptr, d_npts.ptr, d_ncand.ptr))
    except Exception:
        for d in (d_xy, d_cell, d_npts, d_ncand):
            d.free()
        raise
    finally:
        d_thr.free()  # (msd_dev_free drains the stream first: the kernel has read it)
    return d_xy, d_cell, d_npts, d_ncand


def download_peaks(d_xy, d_cell, d_npts, d_ncand, nimg: int, max_points: int) -> PeaksResult:
    nimg, mp = int(nimg), int(max_points)
    xy = np.empty((nimg, mp, 2), np.float64)
    cell = np.empty((nimg, mp), np.int32)
    npts = np.empty(nimg, np.int32)
    ncand = np.empty(nimg, np.int32)
    if nimg:
        d_xy.download(xy)
        d_cell.download(cell)
        d_npts.download(npts)
        d_ncand.download(ncand)
    res = PeaksResult(ncand=ncand)
    for m in range(nimg):
        res.points.append(xy[m, : npts[m]].copy())
        res.cells.append(cell[m, : npts[m]].copy())
    return res


def spec_peaks(spec, k_lo: int, k_hi: int, thr, sx: float = 1.0, sy: float = 1.0, max_points: int = ORB_NFEATURES,
               frames: int | None = None, device: int = 0) -> PeaksResult:
    """The cells ``k_lo <= k <= k_hi, t < frames`` of float64 spectrograms ``spec`` [nimg][K][ld] (or one
    [K][ld]) above ``thr`` (a scalar or one value per image), at most ``max_points`` per image: the
    largest by (value descending, cell ascending), in cell order c = t nk + (k - k_lo)."""
    s = np.ascontiguousarray(spec, dtype=np.float64)
    if s.ndim == 2:
        s = s[None]
    if s.ndim != 3:
        raise ValueError("spec must be [K][ld] or [nimg][K][ld]")
    nimg, K, ld = s.shape
    frames = ld if frames is None else int(frames)
    ctx = context(device)
    d_spec = ctx.alloc(max(s.nbytes, 8))
    if s.nbytes:
        d_spec.upload(s)
    try:
        bufs = peaks_dev(ctx, d_spec, nimg, K, frames, ld, k_lo, k_hi, thr, sx, sy, max_points)
    finally:
        d_spec.free()
    try:
        return download_peaks(*bufs, nimg, max_points)
    finally:
        for d in bufs:
            d.free()
