"""The C5 stream detector (csrc/stream.hip through meteorgpu/stream.py) against the oracle
(oracle/dsp_oracle.py) over its whole contract: the rows of tests/stream_cases.py, which are those of
tests/detector_cases.py plus the stream's own classes.

Every comparison is bit-exact, NaN equal to NaN at the same index (same_floats): the whole thresholds
list (res.thresholds adaptive, res.thr0 global), start, stop and dB of every detection, their count,
and res.margin against the minimum of |delta - threshold used| over the oracle's list (NaN terms
ignored, +inf if none is left).  Rows on which the reference raises must raise the same exception.
Without the thresholds output (run(False)) detections, dB and count are compared and thresholds is
None; the margin is then taken against predicted thresholds and is not compared.

Four paths, one test per class and path:
(a) native    stream.detect_stream with LocalComm (msd_stream_detect_local), seg_len 64 and
              cap_per_seg = seg_len // 2 + 1; window_tree and tile_and_segment_edges again at 512, 8192
(b) sharded   StreamDetector over DeviceStreamOps plans on rank-threads, one context per rank
(c) decisions run(False) at world 1
(d) listed    run(False) with MSD_OPT_STREAM_EPS_LOG2 = 100: every unfrozen frame is a near tie and
              fresh_list_kernel carries the whole detector

Each class and path prints one line:
STREAM class path: rows, frames, detections, ties, longest run, min margin, max rounds, max refined.
"""
import numpy as np
import pytest

from meteorgpu import _lib, dsp, stream
from tests import stream_cases as S
from tests.stream_np_ops import run_threads, shard_bounds

pytestmark = pytest.mark.gpu

SEG = 64
RAISES = {1: AssertionError, 2: IndexError}


def _params(c):
    """(adaptive, W, Fb, Fa, F0) of a row"""
    return (c.cfg is not None,) + (c.cfg or (0, 0, 0, 0))


def _plan(ctx, c, frame0=0, n_local=None, seg_len=SEG, head_frames=8192):
    adaptive, W, Fb, Fa, F0 = _params(c)
    n = len(c.delta)
    n_local = n if n_local is None else n_local
    plan = _lib.StreamPlan(ctx, _lib.det_cfg(adaptive, c.k, W, Fb, Fa, F0), n, frame0, n_local, seg_len=seg_len,
                           cap_per_seg=seg_len // 2 + 1, head_frames=head_frames)
    plan.set_delta(c.delta[frame0:frame0 + n_local])
    return plan


def _detector(plan, c, comm, head_frames=8192):
    adaptive, W, _, _, F0 = _params(c)
    return stream.StreamDetector(stream.DeviceStreamOps(plan), comm, adaptive, c.k, W, F0, head_frames=head_frames)


def _check_detections(c, r, res):
    assert len(res.detections) == len(r.dets), (c.name, len(res.detections), len(r.dets))
    assert res.detections["start"].tolist() == r.dets["start"].tolist(), c.name
    assert res.detections["stop"].tolist() == r.dets["stop"].tolist(), c.name
    assert S.same_floats(res.detections["db"], r.dets["db"]), c.name


def _check_thresholds(c, r, thr, thr0):
    if c.cfg is None:
        assert S.same_floats([thr0], r.thr), (c.name, thr0, r.thr)
        assert S.same_floats(thr, r.thr), c.name
    elif not S.same_floats(thr, r.thr):
        assert len(thr) == len(r.thr), (c.name, len(thr), len(r.thr))
        bad = np.flatnonzero([not S.same_floats(a, b) for a, b in zip(thr, r.thr)])
        raise AssertionError((c.name, "thresholds differ first at frame", bad[:1], thr[bad[:1]], r.thr[bad[:1]]))


def _check(c, r, res, thresholds=True):
    _check_detections(c, r, res)
    if not thresholds:
        assert res.thresholds is None, c.name
        return
    _check_thresholds(c, r, res.thresholds, res.thr0)
    assert S.same_floats([res.margin], [r.margin]), (c.name, res.margin, r.margin)


class Line:
    """the printed line of one class and path"""

    def __init__(self, cls, path):
        self.cls, self.path, self.rows, self.refs, self.rounds, self.refined = cls, path, [], [], 0, 0

    def add(self, c, r, results=()):
        self.rows.append(c)
        self.refs.append(r)
        for x in results:
            self.rounds, self.refined = max(self.rounds, x.rounds), max(self.refined, x.refined)

    def print(self):
        runs = [int(a["stop"] - a["start"]) for r in self.refs for a in r.dets]
        print(f"\nSTREAM {self.cls} {self.path}: rows {len(self.rows)}, frames {sum(len(c.delta) for c in self.rows)}, "
              f"detections {len(runs)}, ties {sum(r.ties for r in self.refs)}, longest run {max(runs, default=0)}, "
              f"min margin {min((r.margin for r in self.refs), default=S.D.INF):.3e}, rounds {self.rounds}, "
              f"refined {self.refined}")


# ------------------------------------------------------------------ (a) the native one-call path
def _native(ctx, c, seg_len):
    adaptive, W, Fb, Fa, F0 = _params(c)
    return stream.detect_stream(ctx, c.delta, len(c.delta), 0, adaptive=adaptive, k_std=c.k, window_blocks=W,
                                freeze_after_blocks=Fa, freeze_before_blocks=Fb, fixed_init_blocks=F0,
                                seg_len=seg_len, cap_per_seg=seg_len // 2 + 1)


def _run_native(cls, seg_len):
    ctx = dsp.context(0)
    line = Line(cls, f"native/{seg_len}")
    for c in S.cases(cls):
        r = S.reference(c.name)
        if r.status:
            with pytest.raises(RAISES[r.status]):
                _native(ctx, c, seg_len)
            line.add(c, r)
            continue
        res = _native(ctx, c, seg_len)
        _check(c, r, res)
        line.add(c, r, [res])
    line.print()


@pytest.mark.parametrize("cls", S.CLASSES)
def test_native(cls):
    _run_native(cls, SEG)


@pytest.mark.parametrize("seg_len", [512, 8192])
@pytest.mark.parametrize("cls", ["window_tree", "tile_and_segment_edges"])
def test_native_segments(cls, seg_len):
    _run_native(cls, seg_len)


@pytest.mark.parametrize("cls", S.CLASSES)
def test_native_plan_is_clean(cls):
    """one row of the class on a plan built by hand: the thresholds are the shard's n_local frames and
    no more; a decisions-only run and a second full run on the same plan leave nothing behind (states,
    need / done tiles, exact flags): the same bits"""
    ctx = dsp.context(0)
    rows = [c for c in S.cases(cls) if S.reference(c.name).status == 0 and len(c.delta)]
    c = rows[len(rows) // 2]
    r = S.reference(c.name)
    plan = _plan(ctx, c)
    try:
        det = _detector(plan, c, stream.LocalComm())
        first = det.run()
        assert plan.thresholds().shape == (len(c.delta),)
        _check(c, r, first)
        decided = det.run(False)
        _check(c, r, decided, thresholds=False)
        again = det.run()
        _check(c, r, again)
        assert first.detections.tobytes() == again.detections.tobytes() == decided.detections.tobytes()
        assert S.same_floats(first.thresholds, again.thresholds) and S.same_floats([first.margin], [again.margin])
    finally:
        plan.close()


# ------------------------------------------------------------------ (c), (d) decisions only
def _run_decisions(ctx, cls, rows, path):
    line = Line(cls, path)
    for c in rows:
        r = S.reference(c.name)
        if len(c.delta) == 0 or r.status:  # the plan of an empty stream runs nothing: through the same call
            if r.status:
                with pytest.raises(RAISES[r.status]):
                    _run_one_decision(ctx, c)
            else:
                assert len(_run_one_decision(ctx, c).detections) == 0
            line.add(c, r)
            continue
        res = _run_one_decision(ctx, c)
        _check(c, r, res, thresholds=False)
        line.add(c, r, [res])
    line.print()
    return line


def _run_one_decision(ctx, c):
    plan = _plan(ctx, c)
    try:
        return _detector(plan, c, stream.LocalComm()).run(False)
    finally:
        plan.close()


@pytest.mark.parametrize("cls", S.CLASSES)
def test_decisions_only(cls):
    _run_decisions(dsp.context(0), cls, S.cases(cls), "decisions")


LISTED = {"window_tree": [f"window_tree/W{W}" for W in (8191, 8195, 16383, 65537)],
          "huge_window": [c.name for c in S.cases("huge_window")],
          "nonfinite_stream": [c.name for c in S.cases("nonfinite_stream")]}


@pytest.mark.parametrize("cls", sorted(LISTED))
def test_listed_frames_carry_everything(cls):
    ctx = _lib.Context(0)
    try:
        ctx.set_option(_lib.OPT_STREAM_EPS_LOG2, 100)
        line = _run_decisions(ctx, cls, [S.case(n) for n in LISTED[cls]], "listed")
    finally:
        ctx.close()
    # every unfrozen frame past F0 was a near tie: at least the fresh full-window frames were made exact
    assert line.refined >= min(len(S.fresh_full(c)) for c in line.rows)


# ------------------------------------------------------------------ (b) the sharded protocol on device plans
def _sharded(jobs, world, head_frames=8192, seg_len=256):
    """jobs [(row, cut frames)] of one world size in one run_threads call: each rank-thread makes one
    context and loops over the jobs; returns, per job, the ranks' results"""
    def body(rank, comm):
        ctx = _lib.Context(0)
        try:
            out = []
            for c, cut in jobs:
                lo, hi = shard_bounds(len(c.delta), world, rank, list(cut))
                plan = _plan(ctx, c, lo, hi - lo, seg_len=seg_len, head_frames=head_frames)
                try:
                    out.append(_detector(plan, c, comm, head_frames).run())
                finally:
                    plan.close()
            return out
        finally:
            ctx.close()

    assert all(len(cut) == world - 1 for _, cut in jobs)
    return list(zip(*run_threads(world, body)))


def _check_sharded(cls, jobs, world, note="", **kw):
    line = Line(cls, f"sharded/{world}{note}")
    for c, _ in jobs:
        assert S.reference(c.name).status == 0 and len(c.delta), c.name
    for (c, cut), ranks in zip(jobs, _sharded(jobs, world, **kw)):
        r = S.reference(c.name)
        for res in ranks:  # every rank holds the whole stream's detections, thr0 and margin
            _check_detections(c, r, res)
            assert S.same_floats([res.margin], [r.margin]), (c.name, cut, res.margin, r.margin)
        thr = np.concatenate([x.thresholds for x in ranks]) if c.cfg is not None else ranks[0].thresholds
        _check_thresholds(c, r, thr, ranks[0].thr0)
        assert all(S.same_floats([x.thr0], [ranks[0].thr0]) for x in ranks), c.name
        line.add(c, r, ranks)
    line.print()


def _thirds(c):
    return (len(c.delta) // 3, len(c.delta) // 3 + 1)


@pytest.mark.parametrize("world", [2, 3, 4, 5])
def test_sharded_cut_sets(world):
    jobs = [(c, cut) for c in S.cases("shard_cuts") for cut in S.cuts(c.name) if len(cut) == world - 1]
    _check_sharded("shard_cuts", jobs, world)


@pytest.mark.parametrize("cls", ["tile_and_segment_edges", "nonfinite", "nonfinite_stream", "ties", "config_sweep"])
def test_sharded_thirds(cls):
    rows = S.cases(cls)[::5] if cls == "config_sweep" else S.cases(cls)
    _check_sharded(cls, [(c, _thirds(c)) for c in rows], 3)


def test_sharded_tile_cut():
    """tile_and_segment_edges once more, cut on both sides of frame 511: a one-frame shard on the edge"""
    _check_sharded("tile_and_segment_edges", [(c, (511, 512)) for c in S.cases("tile_and_segment_edges")], 3,
                   note="/cut_511_512")


def test_sharded_hbm_records():
    """W = 65537 cut at W + 10: the second shard's tail halo is the whole window, and its first tile
    straddles the cut"""
    c = S.case("window_tree/W65537")
    _check_sharded("window_tree", [(c, (c.cfg[0] + 10,))], 2)


def test_sharded_freeze_before():
    _check_sharded("freeze_before", [(c, (len(c.delta) // 2,)) for c in S.cases("freeze_before")], 2)


def test_sharded_long_runs():
    """a head halo of 32768 frames holds every run from its owner's shard on: the dB mean of 8193 and
    20000 frames is two and three numpy chunks, starting at an odd offset of the owner's buffer"""
    jobs = [(c, cut) for c in S.cases("long_runs_sharded") for cut in S.cuts(c.name)]
    _check_sharded("long_runs_sharded", jobs, 3, note="/halo_32768", head_frames=32768)


def test_sharded_long_runs_default_halo():
    """the default head halo of 8192 frames: the 20000-frame runs end past it and fail loudly
    (MSD_ERR_UNSUPPORTED from msd_stream_db), never with a wrong mean; the others, the 8193-frame runs
    cut 10 frames after their start among them, still fit"""
    jobs = [(c, cut) for c in S.cases("long_runs_sharded") for cut in S.cuts(c.name)]
    fits = [(c, cut) for c, cut in jobs if not c.name.endswith("-20000")]
    assert len(fits) == len(jobs) - 2
    for c, cut in fits:
        (s, e), = c.expect
        assert e <= cut[0] + 8192
    _check_sharded("long_runs_sharded", fits, 3, note="/halo_8192")
    for job in jobs:
        if job not in fits:
            with pytest.raises(_lib.MsdError) as err:
                _sharded([job], 3)
            assert err.value.code == _lib.MSD_ERR_UNSUPPORTED and "msd_stream_db" in err.value.msg
