"""CPU: the rows of tests/stream_cases.py held to their promises with the oracle alone, the record
facts of numpy's pairwise tree that every window_tree W is there for, and the host protocol
(meteorgpu/stream.py over the numpy stand-in, tests/stream_np_ops.py) on the same rows.

Every comparison is bit-exact (detector_cases.same_floats: NaN equals NaN at the same index)."""
import numpy as np
import pytest

from meteorgpu import stream
from tests import stream_cases as S
from tests.stream_np_ops import NumpyStreamOps, run_threads, shard_bounds

NEW_WITH_RUNS = ("window_tree", "huge_window", "tile_and_segment_edges", "shard_cuts", "long_runs_sharded",
                 "freeze_before", "nonfinite_stream")


# ------------------------------------------------------------------ generator promises
@pytest.mark.parametrize("cls", NEW_WITH_RUNS)
def test_planted_runs_are_detections(cls):
    for c in S.cases(cls):
        r = S.reference(c.name)
        assert r.status == 0 and c.expect, c.name
        got = set(zip(r.dets["start"].tolist(), r.dets["stop"].tolist()))
        want = set(c.expect)
        assert want <= got, (c.name, sorted(want - got), sorted(got))
        # past a fixed-init stretch nothing else fires in quiet noise (a non-finite frame may: +inf does)
        if c.cfg is None or (c.cfg[3] > 0 and cls != "nonfinite_stream"):
            assert want == got, (c.name, sorted(got - want))


@pytest.mark.parametrize("cls,least", [("window_tree", 500), ("huge_window", 200)])
def test_fresh_full_window_frames(cls, least):
    for c in S.cases(cls):
        assert len(S.fresh_full(c)) >= least, (c.name, len(S.fresh_full(c)))


def test_row_shapes():
    assert [c.cfg[0] for c in S.cases("window_tree")] == list(S.TREE_W)
    for c in S.cases("window_tree"):
        W = c.cfg[0]
        assert len(c.delta) == W + 1100 and c.cfg == (W, 0, 30, max(0, W - 700)) and c.k == 4.0
    for c, W in zip(S.cases("huge_window"), (524288, 532483)):
        assert len(c.delta) == W + 300 and c.cfg == (W, 0, 30, W - 100)
    assert -(-524288 // 8192) == 64 and divmod(532483, 8192) == (65, 3)
    assert all(len(c.delta) == 3000 and (c.cfg is None or c.cfg[0] == 50) for c in S.cases("tile_and_segment_edges"))
    assert [len(c.delta) for c in S.cases("shard_cuts")] == [6000, 6000]
    assert {len(cs) + 1 for cs in S.CUT_SETS} == {2, 3, 4, 5}
    assert all(list(cs) == sorted(cs) and 0 <= cs[0] and cs[-1] <= S.CUT_NB for cs in S.CUT_SETS)
    assert len(S.cases("long_runs_sharded")) == 8
    assert [len(c.delta) for c in S.cases("nonfinite_stream")] == [5000] * 8
    assert {c.name.split("/")[0] for cls in S.CLASSES for c in S.cases(cls)} == set(S.CLASSES)


def test_shard_cut_sets_hit_the_state():
    """the cut sets name what they cut: the first run's start, inside, stop, past it, the end of its
    freeze and the frame after, F0, W, both ends, a repeated cut and cuts one frame apart"""
    c = S.case("shard_cuts/adaptive")
    r = S.reference(c.name)
    W, _, Fa, F0 = c.cfg
    s, e = int(r.dets["start"][0]), int(r.dets["stop"][0])
    fz = e - 1 + Fa
    thr = r.thr
    assert S.same_floats(thr[s + 1:fz + 1], np.full(fz - s, thr[s])) and thr[fz + 1] != thr[fz]  # frozen to fz
    flat = {x for cs in S.CUT_SETS for x in cs}
    assert {s, s + 1, e, e + 1, fz, fz + 1, F0, W, 0, len(c.delta)} <= flat
    assert any(a == b for cs in S.CUT_SETS for a, b in zip(cs, cs[1:]))
    assert any(b == a + 1 for cs in S.CUT_SETS for a, b in zip(cs, cs[1:]))
    for name in (x.name for x in S.cases("long_runs_sharded")):
        (a, b), = S.case(name).expect
        assert S.cuts(name) == ((a + 10, (a + b) // 2),)


def test_tile_edge_freezes_end_on_the_edge():
    for fa in S.TILE_FA:
        c = S.case(f"tile_and_segment_edges/freeze_ends_{500 + fa}")
        thr = S.reference(c.name).thr
        assert thr[500 + fa] == thr[500] and thr[500 + fa + 1] != thr[500]
    assert [500 + fa for fa in S.TILE_FA] == [511, 512, 513]


def test_freeze_before_rows_show_the_parameter():
    """Fb = -40 with Fa = 5 freezes for 40 frames (main.py:491-493): other thresholds and one more
    detection than Fb = 0; 15, 55 and -3 change nothing"""
    from oracle import dsp_oracle as O
    rows = {c.cfg[1]: c for c in S.cases("freeze_before")}
    d = rows[15].delta
    W, _, Fa, F0 = rows[15].cfg
    _, thr0 = O.get_detections_adaptive_ref(d, 4.0, 1.0, W, 0, Fa, F0)
    for Fb, c in rows.items():
        assert c.delta is not None and np.array_equal(c.delta, d)
        same = S.same_floats(S.reference(c.name).thr, thr0)
        assert same == (Fb != -40), Fb
    assert len(S.reference(rows[-40].name).dets) == len(S.reference(rows[15].name).dets) + 1


def test_nonfinite_stream_rows():
    for c in S.cases("nonfinite_stream"):
        bad = np.flatnonzero(~np.isfinite(c.delta))
        assert bad.tolist() == ([0] if "nan_first" in c.name else [100])
        thr = S.reference(c.name).thr
        at = int(bad[0])
        W = c.cfg[0]  # every fresh window that holds the frame gives NaN (+inf fires and freezes first)
        assert np.isnan(thr[at + 1 + S.FA:at + 1 + W]).all() and np.isfinite(thr[at + 1 + W + S.FA:]).all()


# ------------------------------------------------------------------ the tree matters on these inputs
def _seq_sum(x):
    return np.cumsum(x)[-1]  # left to right in float64


def _seq_threshold(win, k):
    mean = _seq_sum(win) / len(win)
    return mean + k * np.sqrt(_seq_sum((win - mean) * (win - mean)) / len(win))


@pytest.mark.parametrize("name", [c.name for cls in ("window_tree", "huge_window") for c in S.cases(cls)
                                  if c.cfg[0] >= 9])
def test_tree_matters(name):
    """on at least one fresh full-window frame a left-to-right float64 sum gives another threshold
    than numpy's tree: a kernel with the wrong association fails this row"""
    c = S.case(name)
    W, thr = c.cfg[0], S.reference(name).thr
    for i in S.fresh_full(c)[:300]:
        t = _seq_threshold(c.delta[i - W:i], c.k)
        assert abs(t - thr[i]) < 1e-9
        if not S.same_floats([t], [thr[i]]):
            return
    raise AssertionError(f"{name}: a left-to-right sum gives numpy's thresholds on every fresh frame")


def test_sequential_mean_misses_the_long_run_db():
    c, r = S.case("long_runs_sharded/adaptive-1000"), S.reference("long_runs_sharded/adaptive-1000")
    (s, e), = c.expect
    assert r.dets["db"][0] == np.mean(c.delta[s:e])
    assert not S.same_floats([_seq_sum(c.delta[s:e]) / (e - s)], r.dets["db"][:1])


# ------------------------------------------------------------------ the record facts
def test_record_facts():
    nrec = {W: len(S.build_program(W)[0]) for W in (65536, 65537)}
    assert nrec == {65536: 512, 65537: 513}
    depth = {W: S.build_program(W)[1] for W in S.TREE_W}
    assert [depth[W] for W in (7689, 8191, 16383, 73727)] == [8] * 4 and depth[8192] == 7
    chunk = [S.build_program(m)[1] for m in range(1, 8193)]  # every length of one chunk
    full = [m for m, dep in enumerate(chunk, 1) if dep == 8]
    assert max(chunk) == 8  # stk_[FR_DEPTH + 1] of fresh_pass holds them
    assert len(full) == 441 and full[0] == 7689 and full[-1] == 8191

    def short(W):
        return [m for _, m, _, _ in S.build_program(W)[0] if m < 8]

    assert short(8193) == [1] and short(8195) == [3] and short(8199) == [7] and short(8200) == []
    assert [m for _, m, _, _ in S.build_program(8200)[0]][-1] == 8
    assert len(S.build_program(524288)[0]) == 4096 and len(S.build_program(532483)[0]) == 4161
    for W in S.TREE_W:  # the records tile the window in order, every chunk ends once
        rec = S.build_program(W)[0]
        assert rec[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(rec, rec[1:]))
        assert rec[-1][0] + rec[-1][1] == W and sum(r[3] for r in rec) == -(-W // 8192)
        assert all(1 <= r[1] <= 128 for r in rec)


@pytest.mark.parametrize("W", S.TREE_W)
def test_records_are_numpys_sum(W):
    rec, _ = S.build_program(W)
    rng = np.random.default_rng(9700 + W)
    for trial in range(2 if W > 20000 else 4):
        x = rng.standard_normal(W) * 10.0 ** rng.uniform(-3, 3, W)
        assert S.same_floats([S.run_program(rec, x)], [np.sum(x)]), (W, trial)
        m = np.sum(x) / W
        sq = (x - m) * (x - m)
        assert S.same_floats([S.run_program(rec, sq)], [np.sum(sq)]), (W, trial)


# ------------------------------------------------------------------ the host protocol on the same rows
def protocol(c, cut, stand_in_freeze=None, head_frames=32768):
    """StreamDetector over NumpyStreamOps, one rank-thread per shard of `cut`"""
    n, adaptive = len(c.delta), c.cfg is not None
    W, Fb, Fa, F0 = c.cfg or (0, 0, 0, 0)
    freeze = max(Fa, -Fb) if stand_in_freeze is None else stand_in_freeze  # the stand-in takes one length
    world = len(cut) + 1

    def body(r, comm):
        lo, hi = shard_bounds(n, world, r, list(cut))
        ops = NumpyStreamOps(c.delta[lo:hi], n, lo, adaptive, c.k, W, freeze, F0, head_frames=head_frames)
        return stream.StreamDetector(ops, comm, adaptive, c.k, W, F0, head_frames=head_frames).run()

    return run_threads(world, body)


def check_protocol(c, res):
    r = S.reference(c.name)
    for x in res:  # every rank returns the whole stream's detections
        assert x.detections["start"].tolist() == r.dets["start"].tolist(), c.name
        assert x.detections["stop"].tolist() == r.dets["stop"].tolist(), c.name
        assert S.same_floats(x.detections["db"], r.dets["db"]), c.name
        assert S.same_floats([x.margin], [r.margin]), (c.name, x.margin, r.margin)
    if c.cfg is not None:
        assert S.same_floats(np.concatenate([x.thresholds for x in res]), r.thr), c.name
    else:
        assert all(S.same_floats(x.thresholds, r.thr) and S.same_floats([x.thr0], r.thr) for x in res), c.name


@pytest.mark.parametrize("mode", ["adaptive", "global"])
def test_protocol_shard_cuts(mode):
    c = S.case(f"shard_cuts/{mode}")
    for cut in S.cuts(c.name):
        check_protocol(c, protocol(c, cut))


def test_protocol_long_runs_sharded():
    for c in S.cases("long_runs_sharded"):
        for cut in S.cuts(c.name):
            check_protocol(c, protocol(c, cut))


def test_protocol_tile_edges_world3():
    for c in S.cases("tile_and_segment_edges"):
        check_protocol(c, protocol(c, (len(c.delta) // 3, 2 * len(c.delta) // 3)))
        check_protocol(c, protocol(c, (511, 512)))


def test_protocol_freeze_before():
    for c in S.cases("freeze_before"):
        check_protocol(c, protocol(c, (len(c.delta) // 2,)))
    c = S.case("freeze_before/Fb-40_Fa5")
    with pytest.raises(AssertionError):  # Fa alone, not max(Fa, -Fb): the row bites
        check_protocol(c, protocol(c, (len(c.delta) // 2,), stand_in_freeze=c.cfg[2]))
