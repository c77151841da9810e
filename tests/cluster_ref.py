"""numpy restatements of the burst clustering's contract (include/msdsp.h a11, csrc/cluster_plan.h), the
reference of tests/test_gpu_cluster.py, test_gpu_spec_peaks.py and test_gpu_legacy_cluster.py.  Pinned to
sklearn, to a literal run of the reference's loop and to np.lexsort by tests/test_cluster_ref.py."""
import numpy as np


def adjacency(p, eps):
    """A[i][j] = (dx dx + dy dy) <= eps eps in float64, in that order (numpy does not contract)"""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    dx = p[:, None, 0] - p[None, :, 0]
    dy = p[:, None, 1] - p[None, :, 1]
    return (dx * dx + dy * dy) <= np.float64(eps) * np.float64(eps)


def dbscan(p, eps, min_samples):
    """labels int32 [n]: components of the core points numbered by their lowest-index core point, a
    border point takes the lowest id among its core neighbours, noise -1"""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    n = p.shape[0]
    A = adjacency(p, eps)
    core = A.sum(axis=1) >= min_samples
    labels = np.full(n, -1, np.int32)
    nxt = 0
    for s in range(n):
        if not core[s] or labels[s] >= 0:
            continue
        labels[s] = nxt
        stack = [s]
        while stack:
            i = stack.pop()
            for j in np.nonzero(A[i] & core & (labels < 0))[0]:
                labels[j] = nxt
                stack.append(int(j))
        nxt += 1
    for i in np.nonzero(~core)[0]:
        nb = np.nonzero(A[i] & core)[0]
        if nb.size:
            labels[i] = labels[nb].min()
    return labels


def boxes(p, labels, critical_min_extent=5.0):
    """(boxes float64 [n_clusters][4] = x_min, y_min, x_max, y_max; critical bool [n_clusters])"""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    nc = int(labels.max()) + 1 if labels.size else 0
    b = np.empty((nc, 4), np.float64)
    for c in range(nc):
        q = p[labels == c]
        b[c, :2] = q.min(axis=0)
        b[c, 2:] = q.max(axis=0)
    return b, (b[:, 2] - b[:, 0]) >= np.float64(critical_min_extent)


def cluster(p, eps=30.0, min_samples=5, critical_min_extent=5.0):
    """(labels, boxes, critical, summary) with summary = (n_clusters, n_critical, n_noncritical, n_noise)"""
    lab = dbscan(p, eps, min_samples)
    b, crit = boxes(p, lab, critical_min_extent)
    return lab, b, crit, (b.shape[0], int(crit.sum()), int((~crit).sum()), int((lab < 0).sum()))


def spec_peaks(spec, frames, k_lo, k_hi, thr, sx, sy, max_points):
    """one image spec [K][ld]: (points float64 [npts][2], cells int32 [npts], ncand).  The cut is taken at
    the max_points-th largest value: everything above it stays, and of its equals the lowest cells
    (no np.lexsort here: test_cluster_ref.py compares against one)"""
    spec = np.asarray(spec, np.float64)
    nk = k_hi - k_lo + 1
    win = spec[k_lo:k_hi + 1, :frames].T.reshape(-1)  # index c = t nk + (k - k_lo)
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(win > thr)[0]
    ncand = cand.size
    if ncand > max_points:
        v = win[cand]
        cutv = np.sort(v)[ncand - max_points]  # the max_points-th largest value
        above = cand[v > cutv]
        equal = cand[v == cutv]  # ascending c
        cand = np.sort(np.concatenate([above, equal[: max_points - above.size]]))
    t, kk = cand // nk, cand % nk
    pts = np.stack([t.astype(np.float64) * np.float64(sx), kk.astype(np.float64) * np.float64(sy)], axis=1)
    return pts.reshape(-1, 2), cand.astype(np.int32), int(ncand)
