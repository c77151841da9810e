"""CPU: the numpy restatements of tests/cluster_ref.py against what they restate -- sklearn's DBSCAN as the
reference calls it (meteor_detect_class/detector_and_classification.py:20), a literal run of the reference's
box / critical loop (:38-67) on those labels, and an np.lexsort implementation of the point selection."""
import numpy as np
import pytest

import cluster_ref as R

sklearn_cluster = pytest.importorskip("sklearn.cluster")


def _sk(p, eps, ms):
    return sklearn_cluster.DBSCAN(eps=eps, min_samples=ms).fit(p).labels_


def contested_border():
    """two 5-point clumps 7 apart and one point midway, (4.5, -3.5): 3.5^2 + 3.5^2 = 24.5 <= 25 from (1, 0) and
    from (8, 0), farther from the rest, so with eps = 5, min_samples = 5 it has 3 neighbours (itself included):
    a border point that both clusters reach.  It belongs to the lower id."""
    a = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]
    b = [(8, 0), (9, 0), (8, 1), (9, 1), (9, 2)]
    return np.array(a + b + [(4.5, -3.5)], np.float64)


def test_contested_border_is_contested():
    p = contested_border()
    A = R.adjacency(p, 5.0)
    core = A.sum(axis=1) >= 5
    lab = R.dbscan(p, 5.0, 5)
    assert not core[10] and set(lab[np.nonzero(A[10] & core)[0]]) == {0, 1} and lab[10] == 0
    assert np.array_equal(lab, _sk(p, 5.0, 5))
    # the same border listed first: still the lower id, although the higher cluster's point is nearer in index
    q = np.concatenate([p[10:], p[5:10], p[:5]])
    lab = R.dbscan(q, 5.0, 5)
    assert lab[0] == 0 and np.array_equal(lab, _sk(q, 5.0, 5))


@pytest.mark.parametrize("eps", [3, 5, 8, 30])
@pytest.mark.parametrize("ms", [1, 2, 3, 5, 8])
def test_dbscan_equals_sklearn(eps, ms):
    rng = np.random.default_rng(1000 * eps + ms)
    for n, span in ((0, 10), (1, 10), (7, 10), (60, 25), (200, 60), (512, 120), (300, 400)):
        if n == 0:
            assert R.dbscan(np.zeros((0, 2)), eps, ms).size == 0
            continue
        p = rng.integers(0, span, size=(n, 2)).astype(np.float64)  # integers: distances are exact
        assert np.array_equal(R.dbscan(p, eps, ms), _sk(p, eps, ms)), (n, span)


def test_chain_and_inclusive_tie():
    p = np.stack([np.arange(512) * 30.0, np.zeros(512)], axis=1)  # spacing == eps: neighbours by the inclusive <=
    for ms in (2, 3):
        assert np.array_equal(R.dbscan(p, 30.0, ms), _sk(p, 30.0, ms))
    assert (R.dbscan(p, 30.0, 3) == 0).all() and (R.dbscan(p, 30.0, 4) == -1).all()
    p2 = np.array([(0, 0), (3, 4)], np.float64)
    assert list(R.dbscan(p2, 5.0, 2)) == [0, 0] and list(_sk(p2, 5.0, 2)) == [0, 0]


def _reference_loop(keypoints_coords, labels):
    """detector_and_classification.py:38-67 without the drawing"""
    critical_bursts, non_critical_bursts, rect_positions = [], [], {}
    unique_labels = set(labels)
    for label in unique_labels:
        if label == -1:
            continue
        cluster_points = keypoints_coords[labels == label]
        x_min, y_min = np.min(cluster_points, axis=0)
        x_max, y_max = np.max(cluster_points, axis=0)
        duration = x_max - x_min
        if duration >= 5:
            critical_bursts.append(label)
        else:
            non_critical_bursts.append(label)
        rect_positions[label] = (x_min, y_min, x_max, y_max)
    return critical_bursts, non_critical_bursts, rect_positions


def test_boxes_and_critical_equal_the_reference_loop():
    rng = np.random.default_rng(7)
    cases = [contested_border(), np.array([(0, 0), (5, 0), (5, 1), (0, 1), (2, 2)], np.float64)]  # extent == 5
    cases += [rng.integers(0, s, size=(n, 2)).astype(np.float64) * np.array([1.0, 3.0])
              for n, s in ((40, 12), (200, 60), (500, 200))]
    for p in cases:
        for eps, ms in ((5, 5), (8, 3), (30, 5)):
            lab, b, crit, summ = R.cluster(p, eps, ms, 5.0)
            c, nc, rects = _reference_loop(p, _sk(p, eps, ms))
            assert sorted(c) == list(np.nonzero(crit)[0]) and sorted(nc) == list(np.nonzero(~crit)[0])
            assert summ == (len(rects), len(c), len(nc), int((lab < 0).sum()))
            for k, r in rects.items():
                assert tuple(b[k]) == tuple(r)


def _lexsort_peaks(spec, frames, k_lo, k_hi, thr, sx, sy, max_points):
    nk = k_hi - k_lo + 1
    cells = [(t * nk + kk, spec[k_lo + kk, t]) for t in range(frames) for kk in range(nk) if spec[k_lo + kk, t] > thr]
    c = np.array([a for a, _ in cells], np.int64)
    v = np.array([b for _, b in cells], np.float64)
    order = np.lexsort((c, -v))[:max_points]  # value descending, then cell ascending
    keep = np.sort(c[order])
    pts = np.stack([(keep // nk).astype(np.float64) * sx, (keep % nk).astype(np.float64) * sy], axis=1)
    return pts.reshape(-1, 2), keep.astype(np.int32), len(cells)


def test_peaks_equal_lexsort():
    rng = np.random.default_rng(3)
    for K, ld, frames, k_lo, k_hi, cap, levels in ((3, 5, 5, 0, 2, 4, 3), (9, 40, 33, 2, 7, 25, 4), (9, 40, 33, 2, 7, 1, 2),
                                                    (40, 64, 50, 5, 30, 500, 6), (40, 64, 50, 5, 30, 512, 0)):
        spec = rng.random((K, ld)) if levels == 0 else rng.integers(0, levels, size=(K, ld)).astype(np.float64)
        spec[k_lo, 0], spec[k_hi, frames - 1] = np.inf, np.nan
        for thr in (-1.0, 0.0, 0.5, 1.0, 100.0):
            got = R.spec_peaks(spec, frames, k_lo, k_hi, thr, 3.42, 2.23, cap)
            want = _lexsort_peaks(spec, frames, k_lo, k_hi, thr, 3.42, 2.23, cap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
            assert got[1].size == min(cap, got[2])
