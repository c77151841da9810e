"""detect_kernel (csrc/detect.hip) through msd_detect_dev / msd_detect against the oracle
(oracle/dsp_oracle.py) over its whole contract: the rows of tests/detector_cases.py.

Every comparison is bit-exact, NaN equal to NaN at the same position: thresholds, start, stop, dB,
counts, status, histogram and margin.  The margin reference is the minimum of |delta - threshold
used| over the oracle's thresholds list, NaN terms ignored, +inf if none is left: the kernel forms
the same float64 subtraction and a minimum.  The padding columns [nb, ld) of delta hold NaN, so a
result that reads them shows at once.  Cases of one configuration share one launch.

Each class prints one line:  DET class: files, blocks, detections, ties, longest run, min margin.
"""
import ctypes as C
import datetime

import numpy as np
import pytest

from meteorgpu import _lib, dsp
from tests import detector_cases as D

pytestmark = pytest.mark.gpu

EPOCH = datetime.datetime(1970, 1, 1)


def _us(t):
    return (t - EPOCH) // datetime.timedelta(microseconds=1)


class Out:
    pass


def _launch(rows, k, cfg, cap=None, hist=None, pad=3):
    """one msd_detect_dev launch over delta rows of one configuration; hist = (start_us[F], base_us,
    bucket_us, nbuckets, block_sec, counts DeviceBuffer) or None"""
    ctx = dsp.context(0)
    F = len(rows)
    nbs = np.array([len(r) for r in rows], np.int64)
    ld = int(nbs.max()) + pad
    cap = ld // 2 + 2 if cap is None else cap
    host = np.full((F, ld), np.nan)
    for f, r in enumerate(rows):
        host[f, :len(r)] = r
    bufs = [ctx.alloc(n) for n in (F * ld * 8, F * 8, F * cap * D.DET.itemsize, F * 8, F * ld * 8, F * 8, F * 4)]
    d_delta, d_nb, d_dets, d_cnt, d_thr, d_mg, d_st = bufs
    d_delta.upload(host)
    d_nb.upload(nbs)
    d_dets.memset(0)
    d_thr.memset(0)
    hcfg = None
    if hist is not None:
        start_us, base_us, bucket_us, nbuckets, block_sec, d_counts = hist
        d_start = ctx.alloc(F * 8)
        d_start.upload(np.asarray(start_us, np.int64))
        bufs.append(d_start)
        hcfg = C.byref(_lib.MsdHistCfg(d_start.ptr, int(base_us), int(bucket_us), int(nbuckets), 0, float(block_sec),
                                       d_counts.ptr))
    dcfg = _lib.det_cfg(cfg is not None, k, *(cfg or ()))
    _lib.check(ctx.lib.msd_detect_dev(ctx.h, d_delta.ptr, d_nb.ptr, F, ld, C.byref(dcfg), d_dets.ptr, cap, d_cnt.ptr,
                                      d_thr.ptr, d_mg.ptr, d_st.ptr, hcfg))
    o = Out()
    o.cap, o.ld = cap, ld
    o.counts = d_cnt.download(np.empty(F, np.int64))
    o.dets = d_dets.download(np.empty((F, cap), D.DET))
    o.thr = d_thr.download(np.empty((F, ld), np.float64))
    o.margin = d_mg.download(np.empty(F, np.float64))
    o.status = d_st.download(np.empty(F, np.int32))
    for b in bufs:
        b.free()
    return o


def _check_file(c, r, o, f):
    """file f of launch o against reference r of case c"""
    nb, cap = len(c.delta), o.cap
    over = r.status == 0 and len(r.dets) > cap
    assert o.status[f] == (3 if over else r.status), c.name
    if c.cfg is None:
        assert D.same_floats(o.thr[f, :1], r.thr), c.name
    else:
        if not D.same_floats(o.thr[f, :nb], r.thr):
            bad = np.flatnonzero([not D.same_floats(a, b) for a, b in zip(o.thr[f, :nb], r.thr)])
            raise AssertionError((c.name, "thresholds differ first at block", bad[:1], o.thr[f, bad[:1]], r.thr[bad[:1]]))
    assert not o.thr[f, (1 if c.cfg is None else nb):].any(), c.name  # cleared before the launch, not written
    assert D.same_floats(o.margin[f:f + 1], [r.margin]), (c.name, o.margin[f], r.margin)
    if r.status == 1:  # the reference raises: no detections to compare
        return
    assert o.counts[f] == len(r.dets), c.name  # the full count, also past the capacity
    n = min(len(r.dets), cap)
    got = o.dets[f, :n]
    assert got["start"].tolist() == r.dets["start"][:n].tolist(), c.name
    assert got["stop"].tolist() == r.dets["stop"][:n].tolist(), c.name
    assert D.same_floats(got["db"], r.dets["db"][:n]), c.name


def _healthy(c):
    """a mixed row named by its block count, not one of the two the reference raises on"""
    return c.name.rsplit("-", 1)[1].isdigit()


def _groups(rows):
    g = {}
    for c in rows:
        g.setdefault((c.k, c.cfg), []).append(c)
    return g


def _run_rows(rows, cap=None):
    """every row through one launch per distinct configuration; {name: (launch, file index)}"""
    where = {}
    for (k, cfg), group in _groups(rows).items():
        o = _launch([c.delta for c in group], k, cfg, cap=cap)
        for f, c in enumerate(group):
            _check_file(c, D.reference(c.name), o, f)
            where[c.name] = (o, f)
    return where


def _det_line(cls, rows, refs=None):
    refs = refs or [D.reference(c.name) for c in rows]
    runs = [int(a["stop"] - a["start"]) for r in refs for a in r.dets]
    print(f"\nDET {cls}: files {len(rows)}, blocks {sum(len(c.delta) for c in rows)}, detections {len(runs)}, "
          f"ties {sum(r.ties for r in refs)}, longest run {max(runs, default=0)}, "
          f"min margin {min(r.margin for r in refs):.3e}")


@pytest.mark.parametrize("cls", D.CLASSES)
def test_class_matches_oracle(cls):
    rows = D.cases(cls)
    _run_rows(rows)
    _det_line(cls, rows)


@pytest.mark.parametrize("mode", ["adaptive", "global"])
def test_mixed_launch(mode):
    """files of 0 .. 3000 blocks in one launch with ld >= 3000: those that fit the LDS chunk beside those
    staged chunk by chunk; in global mode an empty file (status 2) and one whose only block above the
    threshold is the last (status 1) sit between healthy files and leave them as they are"""
    rows = [c for c in D.cases("mixed") if c.name.startswith(f"mixed/{mode}-")]
    if mode == "global":
        ok = [c for c in rows if _healthy(c)]
        rows = ok[:4] + [D.case("mixed/global-empty")] + ok[4:7] + [D.case("mixed/global-last_block_only")] + ok[7:]
    assert len({(c.k, c.cfg) for c in rows}) == 1 and max(len(c.delta) for c in rows) == 3000
    o = _launch([c.delta for c in rows], rows[0].k, rows[0].cfg, pad=5)
    for f, c in enumerate(rows):
        _check_file(c, D.reference(c.name), o, f)
    if mode == "global":
        st = dict(zip((c.name for c in rows), o.status.tolist()))
        assert st.pop("mixed/global-empty") == 2 and st.pop("mixed/global-last_block_only") == 1
        assert set(st.values()) == {0}
        f1 = [c.name for c in rows].index("mixed/global-last_block_only")  # the reference raises: include/msdsp.h
        assert o.counts[f1] == 1 and (o.dets[f1, 0]["start"], o.dets[f1, 0]["stop"]) == (49, 49)
        assert np.isnan(o.dets[f1, 0]["db"])
        healthy = [f for f, c in enumerate(rows) if _healthy(c)]
        assert len(healthy) == len(rows) - 2
        p = _launch([rows[f].delta for f in healthy], rows[0].k, None, pad=5)  # the launch without the two
        assert p.ld == o.ld and p.cap == o.cap
        for name in ("counts", "dets", "margin", "status"):
            assert getattr(o, name)[healthy].tobytes() == getattr(p, name).tobytes(), name
        assert o.thr[healthy, 0].tobytes() == p.thr[:, 0].tobytes()
    _det_line(f"mixed_{mode}", rows)


@pytest.mark.parametrize("mode", ["adaptive", "global"])
def test_capacity(mode):
    """the mixed launch with room for 3 detections per file: files above it report status 3, their full
    count and their first 3 detections complete; the others are untouched; the histogram counts the
    stored detections only (include/msdsp.h)"""
    cap, bs, bucket_us, nbuckets = 3, 0.2, 60 * 10 ** 6, 48
    rows = [c for c in D.cases("mixed") if c.name.startswith(f"mixed/{mode}-")]
    base = datetime.datetime(2025, 6, 25, 0, 0, 0)
    # a file every 97 s; the two global rows on which the reference raises lie a day before the histogram
    starts = [base + datetime.timedelta(seconds=97 * f) if D.reference(c.name).status == 0 else
              base - datetime.timedelta(days=1) for f, c in enumerate(rows)]
    refs = [D.reference(c.name, bs, t) for c, t in zip(rows, starts)]
    ctx = dsp.context(0)
    d_counts = ctx.alloc(nbuckets * 8)
    d_counts.memset(0)
    o = _launch([c.delta for c in rows], rows[0].k, rows[0].cfg, cap=cap, pad=5,
                hist=([_us(t) for t in starts], _us(base), bucket_us, nbuckets, bs, d_counts))
    hist = d_counts.download(np.empty(nbuckets, np.int64))
    d_counts.free()
    want = np.zeros(nbuckets, np.int64)
    for f, (c, r) in enumerate(zip(rows, refs)):
        _check_file(c, r, o, f)
        want += D.bucket_counts_ref(r.utc[:cap], base, bucket_us, nbuckets)
    n_over = sum(1 for r in refs if len(r.dets) > cap)
    assert 0 < n_over < len(rows) and (o.status == 3).sum() == n_over
    full = _run_rows(rows)  # with room for every detection: the same first entries, status 0 where it was 3
    for f, c in enumerate(rows):
        p, pf = full[c.name]
        n = min(int(o.counts[f]), cap)
        assert o.counts[f] == p.counts[pf] and o.dets[f, :n].tobytes() == p.dets[pf, :n].tobytes()
        assert o.margin[f:f + 1].tobytes() == p.margin[pf:pf + 1].tobytes()
    assert hist.tolist() == want.tolist()
    assert hist.sum() == sum(min(len(r.dets), cap) for r in refs if r.status == 0)
    assert hist.sum() < sum(len(r.dets) for r in refs)


HOST_CASES = ["ties/k0", "ties/k1", "lane_and_chunk_edges/gap_at_1023", "lane_and_chunk_edges/global_run_across",
              "long_runs/adaptive-1000", "long_runs/global-129", "nonfinite/posinf-adaptive",
              "window_sizes/bursts", "mixed/adaptive-0", "mixed/adaptive-1"]


def test_host_path():
    """msd_detect (host buffers, one file) on a subset, and once with too little room: MSD_ERR_CAPACITY,
    *count the full count, the first cap entries copied"""
    ctx = dsp.context(0)
    for name in HOST_CASES:
        c, r = D.case(name), D.reference(name)
        dets, thr, margin = _lib.detect(ctx, c.delta, _lib.det_cfg(c.cfg is not None, c.k, *(c.cfg or ())))
        assert D.same_floats(thr, r.thr), name
        assert D.same_floats([margin], [r.margin]), name
        assert dets["start"].tolist() == r.dets["start"].tolist() and dets["stop"].tolist() == r.dets["stop"].tolist()
        assert D.same_floats(dets["db"], r.dets["db"]), name
    c, r = D.case("mixed/adaptive-3000"), D.reference("mixed/adaptive-3000")
    cap, nb = 3, len(c.delta)
    assert len(r.dets) > cap
    dets = np.zeros(cap + 2, D.DET)
    dets["start"] = -7
    thr = np.empty(nb, np.float64)
    count, margin = C.c_int64(0), C.c_double(0)
    cfg = _lib.det_cfg(True, c.k, *c.cfg)
    rc = ctx.lib.msd_detect(ctx.h, _lib.ptr(c.delta), nb, C.byref(cfg), _lib.ptr(dets), cap, C.byref(count),
                            _lib.ptr(thr), C.byref(margin))
    assert rc == _lib.MSD_ERR_CAPACITY
    assert count.value == len(r.dets)
    assert dets["start"][:cap].tolist() == r.dets["start"][:cap].tolist()
    assert dets["stop"][:cap].tolist() == r.dets["stop"][:cap].tolist()
    assert D.same_floats(dets["db"][:cap], r.dets["db"][:cap])
    assert dets["start"][cap:].tolist() == [-7, -7]  # nothing past cap is written
    assert D.same_floats(thr, r.thr) and D.same_floats([margin.value], [r.margin])


@pytest.mark.parametrize("mode,bucket_us", [("adaptive", 3600 * 10 ** 6), ("adaptive", 600 * 10 ** 6),
                                            ("global", 3600 * 10 ** 6)])
def test_histogram(mode, bucket_us):
    """detection starts on a bucket boundary and 0.2 s before it, files before the base (negative
    buckets, floor division on a non-multiple), past the last bucket and across both ends, for hour
    buckets and 10-minute ones; the counts accumulate until the caller clears them"""
    prefix = "histogram/global-" if mode == "global" else "histogram/"
    rows = [D.case(prefix + name) for name in D.HIST_FILES]
    t0 = D.hist_starts(bucket_us)
    starts = [t0[name] for name in D.HIST_FILES]
    refs = [D.reference(c.name, D.HIST_BLOCK_SEC, t) for c, t in zip(rows, starts)]
    want = sum(D.bucket_counts_ref(r.utc, D.HIST_BASE, bucket_us, D.HIST_NBUCKETS) for r in refs)
    assert 0 < want.sum() < sum(len(r.dets) for r in refs)  # some are dropped on either side
    ctx = dsp.context(0)
    d_counts = ctx.alloc(D.HIST_NBUCKETS * 8)
    hist = ([_us(t) for t in starts], _us(D.HIST_BASE), bucket_us, D.HIST_NBUCKETS, D.HIST_BLOCK_SEC, d_counts)

    def run():
        o = _launch([c.delta for c in rows], rows[0].k, rows[0].cfg, hist=hist)
        for f, (c, r) in enumerate(zip(rows, refs)):
            _check_file(c, r, o, f)
        return d_counts.download(np.empty(D.HIST_NBUCKETS, np.int64))

    d_counts.memset(0)
    assert run().tolist() == want.tolist()
    assert run().tolist() == (2 * want).tolist()  # not cleared: the sum of two launches
    d_counts.memset(0)
    assert run().tolist() == want.tolist()
    d_counts.free()
    _det_line(f"histogram_{mode}_{bucket_us // 10 ** 6}s", rows, refs)
    print(f"DET histogram_{mode}_{bucket_us // 10 ** 6}s: buckets {want.tolist()}, dropped "
          f"{sum(len(r.dets) for r in refs) - int(want.sum())}")
