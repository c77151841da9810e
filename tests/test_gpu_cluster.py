"""GPU: the DBSCAN kernel (csrc/cluster.hip, msd_cluster*) against the numpy restatement of
tests/cluster_ref.py, which tests/test_cluster_ref.py pins to sklearn: labels, boxes, critical flags and
summaries bit-equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import cluster_ref as R

pytestmark = pytest.mark.gpu


def _check(res, m, p, eps, ms, ext=5.0):
    lab, b, crit, summ = R.cluster(p, eps, ms, ext)
    assert np.array_equal(res.labels[m], lab), (m, len(p))
    assert res.boxes[m].tobytes() == b.tobytes(), (m, len(p))
    assert np.array_equal(res.critical[m], np.nonzero(crit)[0]), m
    assert np.array_equal(res.non_critical[m], np.nonzero(~crit)[0]), m
    s = res.summary[m]
    assert (s["n_clusters"], s["n_critical"], s["n_noncritical"], s["n_noise"]) == summ, m
    assert s["status"] == 0 and s["n_points"] == len(p)


def _one(p, eps, ms, ext=5.0, max_points=None):
    from meteorgpu import cluster
    p = np.asarray(p, np.float64).reshape(-1, 2)
    res = cluster.cluster_points([p], eps, ms, ext, max_points=max_points)
    _check(res, 0, p, eps, ms, ext)
    return res


def _rand(rng, n, span):
    return rng.integers(0, span, size=(n, 2)).astype(np.float64)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512])
def test_sizes(n):
    rng = np.random.default_rng(n)
    span = int(4 * np.sqrt(n + 1)) + 3
    for eps, ms in ((3, 3), (5, 5), (8, 5)):
        res = _one(_rand(rng, n, span), eps, ms)
    assert n < 63 or res.summary[0]["n_clusters"] >= 1
    _one(_rand(rng, n, 12 * span), 30, 5, max_points=512)


def test_chain_at_spacing_eps():
    """512 points 30 apart at eps = 30: neighbours only by the inclusive <=, the deepest propagation"""
    p = np.stack([np.arange(512) * 30.0, np.zeros(512)], axis=1)
    res = _one(p, 30.0, 3)
    assert (res.labels[0] == 0).all() and res.boxes[0][0, 2] == 30.0 * 511
    _one(p, 30.0, 2)
    assert (_one(p, 30.0, 4).labels[0] == -1).all()
    _one(p[::-1], 30.0, 3)
    rng = np.random.default_rng(5)
    _one(p[rng.permutation(512)], 30.0, 3)  # a chain whose index order is scrambled


def test_345_pair():
    assert list(_one([(0, 0), (3, 4)], 5.0, 2).labels[0]) == [0, 0]
    assert list(_one([(0, 0), (3, 4)], 4.999999, 1).labels[0]) == [0, 1]
    assert list(_one([(0, 0), (3, 4)], 5.0, 3).labels[0]) == [-1, -1]


def test_two_chains_joined_by_the_last_point():
    a = [(float(i), 0.0) for i in range(255)]
    b = [(float(i), 10.0) for i in range(255)]
    res = _one(a + b + [(254.0, 5.0)], 5.0, 2)
    assert res.summary[0]["n_clusters"] == 1 and (res.labels[0] == 0).all()
    res = _one(a + b, 5.0, 2)
    assert res.labels[0][0] == 0 and res.labels[0][255] == 1
    # interleaved: ids follow the lowest core index, not the order in which components close
    far = [(1000.0 + 100 * i, 500.0) for i in range(3)]
    res = _one(far[:1] + b[:200] + far[1:2] + a[:200] + [(199.0, 5.0)] + far[2:], 5.0, 1)
    assert [int(res.labels[0][i]) for i in (0, 1, 201, 202, 402, 403)] == [0, 1, 2, 1, 1, 3]


def test_contested_border_and_duplicates():
    a = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]
    b = [(8, 0), (9, 0), (8, 1), (9, 1), (9, 2)]
    mid = [(4.5, -3.5)]
    for p in (a + b + mid, mid + b + a, b + mid + a):
        res = _one(p, 5.0, 5)
        assert res.summary[0]["n_clusters"] == 2 and res.labels[0][p.index(mid[0])] == 0
    dup = [(7.0, 7.0)] * 6 + [(7.0, 7.0 + 1e-9)] * 2 + [(50.0, 50.0)] * 4 + [(90.0, 9.0)]
    res = _one(dup, 0.0, 5)  # eps = 0: only exact duplicates are neighbours
    assert list(res.labels[0]) == [0] * 6 + [-1] * 7
    _one(dup, 1e-9, 4)
    _one(dup * 30, 0.5, 5)


def test_min_samples_extremes():
    grid = np.array([(40.0 * (i % 32), 40.0 * (i // 32)) for i in range(512)])
    res = _one(grid, 30.0, 1)  # all core, nobody adjacent: n clusters
    assert np.array_equal(res.labels[0], np.arange(512)) and res.summary[0]["n_noncritical"] == 512
    res = _one(grid, 45.0, 513)  # more than n: all noise
    assert (res.labels[0] == -1).all() and res.summary[0]["n_noise"] == 512
    _one(grid[:100], 40.0, 100)
    _one(grid[:100], 1e4, 100)


def test_scaled_non_integer_coordinates():
    rng = np.random.default_rng(11)
    sx, sy = 496 / 145, 366 / 164
    for n in (200, 500):
        c = rng.choice(145 * 164, size=n, replace=False)
        p = np.stack([(c // 164).astype(np.float64) * sx, (c % 164).astype(np.float64) * sy], axis=1)
        for eps in (30.0, 10.0, 3.5):
            _one(p, eps, 5, max_points=500)


def test_extent_equal_to_the_bound_is_critical():
    p = [(0, 0), (5, 0), (5, 1), (0, 1), (2, 2)]
    res = _one(p, 6.0, 3, ext=5.0)
    assert list(res.critical[0]) == [0] and res.summary[0]["n_critical"] == 1
    res = _one(p, 6.0, 3, ext=np.nextafter(5.0, 6.0))
    assert list(res.non_critical[0]) == [0]
    q = np.array(p, np.float64) * 0.1 + 0.3  # (0.5 + 0.3) - 0.3 in float64 against the same expression in numpy
    _one(q, 0.6, 3, ext=0.5)


def test_ragged_batch_of_300_images():
    from meteorgpu import cluster
    rng = np.random.default_rng(300)
    sizes = [(0, 512, 0, 511, 1, 64, 65, 0, 300, 17)[m % 10] if m % 3 else int(rng.integers(0, 513)) for m in range(300)]
    pts = [_rand(rng, n, int(5 * np.sqrt(n + 1)) + 4) * np.array([1.0, 1.5]) for n in sizes]
    res = cluster.cluster_points(pts, 4.0, 4, 5.0, max_points=512)
    assert len(res.labels) == 300
    for m, p in enumerate(pts):
        _check(res, m, p, 4.0, 4, 5.0)


def test_oversize_entry_is_reported_not_clamped():
    from meteorgpu import _lib, cluster
    from meteorgpu.dsp import context
    ctx = context(0)
    rng = np.random.default_rng(2)
    mp = 64
    pts = [_rand(rng, n, 20) for n in (40, 64, 10)]
    xy = np.zeros((3, mp, 2))
    for m, p in enumerate(pts):
        xy[m, : len(p)] = p
    npts = np.array([40, 65, 10], np.int32)  # the middle entry is past max_points
    d_xy, d_n = ctx.alloc(xy.nbytes), ctx.alloc(16)
    d_lab, d_sum = ctx.alloc(3 * mp * 4), ctx.alloc(3 * 32)
    d_xy.upload(xy)
    d_n.upload(npts)
    d_lab.memset(0x55)
    cfg = _lib.MsdClusterCfg(5.0, 5.0, 3, mp)
    _lib.check(ctx.lib.msd_cluster_dev(ctx.h, C.byref(cfg), d_xy.ptr, d_n.ptr, 3, d_lab.ptr, None, d_sum.ptr))
    lab = np.empty((3, mp), np.int32)
    summ = np.empty(3, _lib.CLUSTER_SUMMARY_DTYPE)
    d_lab.download(lab)
    d_sum.download(summ)
    assert list(summ["status"]) == [0, _lib.CLUSTER_STATUS_NPTS, 0] and summ["n_clusters"][1] == 0
    assert (lab[1] == 0x55555555).all()
    for m in (0, 2):
        assert np.array_equal(lab[m, : npts[m]], R.dbscan(pts[m], 5.0, 3))
    with pytest.raises(_lib.MsdError) as e:
        cluster.cluster_points([np.zeros((65, 2))], max_points=64)
    assert e.value.code == _lib.MSD_ERR_UNSUPPORTED
    with pytest.raises(_lib.MsdError) as e:
        cluster.dbscan(np.zeros((513, 2)))
    assert e.value.code == _lib.MSD_ERR_UNSUPPORTED
    with pytest.raises(_lib.MsdError) as e:
        cluster.dbscan([(0.0, np.nan)])
    assert e.value.code == _lib.MSD_ERR_INVALID


def test_host_form_and_timing_id():
    from meteorgpu import _lib, cluster
    from meteorgpu.dsp import context
    ctx = context(0)
    rng = np.random.default_rng(9)
    p = _rand(rng, 333, 70)
    ctx.timing(True)
    try:
        ctx.timing_reset()
        lab = cluster.dbscan(p, 5.0, 4)
        ms, launches = ctx.timing_get(_lib.K_CLUSTER)
        assert launches == 1 and ms > 0
        cluster.spec_peaks(np.ones((4, 32)), 1, 2, 0.5, max_points=8)
        assert ctx.timing_get(_lib.K_CLUSTER)[1] == 2
    finally:
        ctx.timing(False)
        ctx.timing_reset()
    assert np.array_equal(lab, R.dbscan(p, 5.0, 4))
    assert cluster.dbscan(np.zeros((0, 2))).size == 0
