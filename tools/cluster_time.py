"""Time the burst clustering (K_CLUSTER: csrc/cluster.hip) and sklearn's DBSCAN over the same points in one run:

* msd_cluster_dev on a day of grabs, 2 880 images x 500 points resident in HBM (one launch, one workgroup per
  image), and on a single image;
* msd_spec_peaks_f64_dev on 360 float64 spectrograms [1025][160] (the 164 x 145 window, cap 500), candidates
  below and above the cap;
* sklearn.cluster.DBSCAN(eps=30, min_samples=5).fit(points) over the same 2 880 point sets on the CPU, and how
  many of its label vectors equal the GPU's;

each GPU figure the median of 10 timed launches after 3 warm-up launches (HIP events around the kernel alone),
plus the wall time of cluster_points (upload, launch, download) for the day.

The points: per image 2 to 6 echoes (a blob of cells around a random place of the 145 x 164 grid) plus scattered
single cells, 500 distinct cells, on the reference image's pixel grid (legacy.SPEC_SX, SPEC_SY).

usage (GPU box): python3 tools/cluster_time.py [--images 2880]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def day_of_points(np, nimg, npts, sx, sy, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nimg):
        parts = []
        for _ in range(int(rng.integers(2, 7))):
            t0, k0 = rng.integers(0, 145), rng.integers(0, 164)
            w, h, m = rng.integers(1, 12), rng.integers(2, 9), int(rng.integers(20, 110))
            t, k = t0 + rng.integers(-w, w + 1, size=m), k0 + rng.integers(-h, h + 1, size=m)
            ok = (t >= 0) & (t < 145) & (k >= 0) & (k < 164)
            parts.append(t[ok] * 164 + k[ok])
        parts.append(rng.integers(0, 145 * 164, size=2 * npts))  # scattered single cells fill up to npts
        c = np.concatenate(parts)
        c = c[np.sort(np.unique(c, return_index=True)[1])][:npts]  # the first npts distinct, echoes first
        c = np.sort(c)
        out.append(np.stack([(c // 164).astype(np.float64) * sx, (c % 164).astype(np.float64) * sy], axis=1))
    return out


def median_ms(ctx, _lib, run, n=10, warm=3):
    for _ in range(warm):
        run()
    ctx.synchronize()
    ms = []
    for _ in range(n):
        ctx.timing(True)
        ctx.timing_reset()
        run()
        ctx.synchronize()
        ms.append(ctx.timing_get(_lib.K_CLUSTER)[0])
    ctx.timing(False)
    ms.sort()
    return ms[n // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2880)
    ap.add_argument("--points", type=int, default=500)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "meteor-scatter_amd"))
    sys.path.insert(0, ROOT)
    import numpy as np
    from meteorgpu import _lib, cluster, legacy
    ctx = _lib.Context(0)
    nimg, mp = a.images, a.points
    pts = day_of_points(np, nimg, mp, legacy.SPEC_SX, legacy.SPEC_SY)
    xy = np.stack(pts)
    d_xy, d_n = ctx.alloc(xy.nbytes), ctx.alloc(4 * nimg)
    d_xy.upload(xy)
    d_n.upload(np.full(nimg, mp, np.int32))
    d_lab, d_box, d_sum = ctx.alloc(nimg * mp * 4), ctx.alloc(nimg * mp * 32), ctx.alloc(nimg * 32)
    cfg = _lib.MsdClusterCfg(30.0, 5.0, 5, mp)

    def run(n):
        _lib.check(ctx.lib.msd_cluster_dev(ctx.h, C.byref(cfg), d_xy.ptr, d_n.ptr, n, d_lab.ptr, d_box.ptr, d_sum.ptr))
    day = median_ms(ctx, _lib, lambda: run(nimg))
    one = median_ms(ctx, _lib, lambda: run(1))
    labels = np.empty((nimg, mp), np.int32)
    summ = np.empty(nimg, _lib.CLUSTER_SUMMARY_DTYPE)
    run(nimg)
    d_lab.download(labels)
    d_sum.download(summ)
    pairs = nimg * mp * mp
    print(f"msd_cluster_dev {nimg} images x {mp} points: median {day[0]:.3f} ms  min {day[1]:.3f}  max {day[2]:.3f}  "
          f"{pairs / day[0] * 1e-6:.1f} G pair tests/s  ({summ['n_clusters'].mean():.2f} clusters, "
          f"{summ['n_noise'].mean():.1f} noise points per image)", flush=True)
    print(f"msd_cluster_dev 1 image x {mp} points: median {one[0]:.4f} ms  min {one[1]:.4f}  max {one[2]:.4f}",
          flush=True)
    t0 = time.perf_counter()
    res = cluster.cluster_points(pts, 30.0, 5, 5.0, max_points=mp)
    wall = time.perf_counter() - t0
    print(f"cluster_points (upload, launch, download, split) for the day: {wall * 1e3:.1f} ms wall", flush=True)
    assert all(np.array_equal(res.labels[m], labels[m]) for m in range(nimg))

    # the point extraction on resident spectrograms
    nspec, K, ld, frames = 360, 1025, 160, 145
    rng = np.random.default_rng(2)
    spec = rng.exponential(1.0, size=(nspec, K, ld))
    d_spec = ctx.alloc(spec.nbytes)
    d_spec.upload(spec)
    for thr, what in ((6.0, "below the cap"), (3.0, "above the cap: radix select")):
        bufs = []

        def peaks():
            for b in bufs:
                b.free()
            bufs[:] = cluster.peaks_dev(ctx, d_spec, nspec, K, frames, ld, 328, 491, thr, legacy.SPEC_SX, legacy.SPEC_SY, mp)
        pk = median_ms(ctx, _lib, peaks)
        nc = cluster.download_peaks(*bufs, nspec, mp).ncand
        print(f"msd_spec_peaks_f64_dev {nspec} images, {nc.mean():.0f} candidates each ({what}): median {pk[0]:.3f} ms  "
              f"min {pk[1]:.3f}  max {pk[2]:.3f}  ({pk[0] / nspec * nimg:.2f} ms per {nimg})", flush=True)

    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        print("sklearn is not installed: no CPU figure")
        return
    t0 = time.perf_counter()
    sk = [DBSCAN(eps=30, min_samples=5).fit(p).labels_ for p in pts]
    t_sk = time.perf_counter() - t0
    t0 = time.perf_counter()
    DBSCAN(eps=30, min_samples=5).fit(pts[0])
    t_one = time.perf_counter() - t0
    same = sum(bool(np.array_equal(sk[m], labels[m])) for m in range(nimg))
    print(f"sklearn DBSCAN on the CPU, the same points: {t_sk * 1e3:.0f} ms for {nimg} images "
          f"({t_sk / nimg * 1e3:.3f} ms each; one alone {t_one * 1e3:.3f} ms); labels equal the GPU's in {same} of "
          f"{nimg} images; GPU kernel {t_sk * 1e3 / day[0]:.0f}x, end to end {t_sk / wall:.0f}x", flush=True)


if __name__ == "__main__":
    main()
