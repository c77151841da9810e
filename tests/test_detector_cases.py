"""CPU: the generators of tests/detector_cases.py deliver what they promise, by the oracle alone
(oracle/dsp_oracle.py).  tests/test_gpu_detect_contract.py holds detect_kernel to the same rows."""
import datetime

import numpy as np
import pytest

from oracle import dsp_oracle as O
from tests import detector_cases as D


def _runs(name):
    r = D.reference(name)
    return [(int(a["start"]), int(a["stop"])) for a in r.dets]


def test_config_sweep_contains_every_listed_value():
    params = D.sweep_params()
    assert len(params) == D.SWEEP_N
    assert {p[1] for p in params} == set(D.SWEEP_W)
    assert {p[3] for p in params} == set(D.SWEEP_FA)
    assert {p[5] for p in params} == set(D.SWEEP_K)
    assert all(300 <= p[0] <= 1500 for p in params)
    # Fb: 0, 15 and Fa + 50 (above freeze_after); F0: 0, 1, 50, nb and nb + 7
    assert {0, 15} <= {p[2] for p in params} and any(p[2] == p[3] + 50 for p in params)
    assert any(p[2] > p[3] for p in params)
    assert {0, 1, 50} <= {p[4] for p in params}
    assert any(p[4] == p[0] for p in params) and any(p[4] == p[0] + 7 for p in params)
    rows = D.cases("config_sweep")
    adaptive = [c for c in rows if c.cfg is not None]
    assert [(len(c.delta),) + c.cfg + (c.k,) for c in adaptive] == list(params)
    assert sorted({c.k for c in rows if c.cfg is None}) == list(D.SWEEP_GLOBAL_K)
    assert all(D.reference(c.name).status == 0 for c in rows)
    assert sum(len(D.reference(c.name).dets) for c in rows) > 1000


def test_window_sizes_row_takes_a_fresh_threshold_of_every_length():
    quiet, bursts = D.cases("window_sizes")
    nb = len(quiet.delta)
    W, Fb, Fa, F0 = quiet.cfg
    assert nb == 2100 and F0 == 0 and W == nb - 1 and bursts.cfg[0] == W and len(bursts.delta) == nb
    r = D.reference(quiet.name)
    assert len(r.dets) == 0  # nothing fires: no freeze, so block i reads the window delta[max(0, i - W):i]
    lengths = {i - max(0, i - W) for i in range(nb)}
    assert lengths == set(range(nb))  # 0 (NaN), the n < 8 leaf, every 8-tail, every NP_ITER_MAX edge, > 1928
    assert np.isnan(r.thr[0]) and not np.isnan(r.thr[1:]).any()
    for n in (1, 7, 8, 9, 15, 128, 129, 248, 249, 488, 489, 968, 969, 1928, 1929, 2099):
        w = quiet.delta[:n]
        assert r.thr[n] == np.mean(w) + quiet.k * np.std(w)
    rb = D.reference(bursts.name)
    assert len(rb.dets) > 5 and bursts.cfg[2] >= 1  # the same sizes while the scan freezes


@pytest.mark.parametrize("k", [0, 1])
def test_ties_rows_hold_exact_ties_that_do_not_fire(k):
    c = D.case(f"ties/k{k}")
    assert set(np.unique(c.delta)) <= {0.0, 1.0, 2.0, 3.0} and c.cfg == (8, 0, 2, 0) and c.k == k
    r = D.reference(c.name)
    tie = np.flatnonzero(c.delta == r.thr)
    assert r.ties == len(tie) >= 20
    inside = np.zeros(len(c.delta), bool)
    for a in r.dets:
        inside[a["start"]:a["stop"]] = True
    assert len(r.dets) > 20 and not inside[tie].any()  # a tie neither starts nor extends a detection
    assert r.margin == 0.0


def test_lane_and_chunk_edges_fire_exactly_where_planted():
    rows = D.cases("lane_and_chunk_edges")
    singles = set()
    for c in rows:
        assert len(c.delta) == D.EDGE_NB == 3000
        assert _runs(c.name) == list(c.expect), c.name
        assert D.reference(c.name).status == 0
        if c.cfg is not None:
            singles |= {s for s, e in c.expect if e == s + 1}
    assert set(D.EDGE_SINGLES) <= singles
    by = {c.name.split("/")[1]: c for c in rows}
    assert len(by["gap_at_1023"].expect) == len(by["gap_at_1024"].expect) == 2  # split across the restage
    assert by["gap_at_1023"].expect[0][1] == 1023 and by["gap_at_1024"].expect[0][1] == 1024
    assert (1020, 1031) in by["pairs_64_65_run_across"].expect  # one run over the restage
    starts = [s for s, _ in by["pairs_64_65_run_across"].expect]
    assert 264 - 200 == 64 and 465 - 400 == 65 and {200, 264, 400, 465} <= set(starts)
    for fa in D.EDGE_FA:  # the freeze of the event at 1000 ends on 1022 .. 1025, the next burst right behind
        c = by[f"freeze_ends_{1000 + fa}"]
        assert c.cfg[2] == fa and c.expect[1][0] == 1000 + fa + 1
        thr = D.reference(c.name).thr
        assert thr[1000 + fa] == thr[1000] != thr[1000 + fa + 1]  # held to the last frozen block, then fresh
    assert by["global_run_to_1023"].expect[0][1] == 1024 and by["global_run_from_1024"].expect[0][0] == 1024


def test_long_runs_are_one_detection_each():
    rows = D.cases("long_runs")
    assert sorted({c.expect[0][1] - c.expect[0][0] for c in rows}) == list(D.LONG_RUNS)
    for c in rows:
        assert _runs(c.name) == list(c.expect), c.name
        L = c.expect[0][1] - c.expect[0][0]
        assert (len(c.delta) <= 1024) == (L == 129)  # only the first plateau's dB mean reads the LDS copy
        if c.cfg is None:
            assert not c.delta[-1] > D.reference(c.name).thr[0]
        else:
            assert c.cfg[2] >= 1


def test_nonfinite_rows():
    rows = D.cases("nonfinite")
    assert len(rows) == 9
    for c in rows:
        bad = np.flatnonzero(~np.isfinite(c.delta))
        assert bad.tolist() == [250]
        r = D.reference(c.name)
        assert r.status == 0
        if c.cfg is None:
            assert np.isnan(r.thr[0]) and len(r.dets) == 0 and r.margin == D.INF
    # the +inf block is above every finite threshold: the reference reports it, with dB inf
    r = D.reference("nonfinite/posinf-adaptive_f0_0")
    assert any(a["start"] <= 250 < a["stop"] and a["db"] == np.inf for a in r.dets)


def test_mixed_rows():
    rows = D.cases("mixed")
    assert [len(c.delta) for c in rows if c.cfg is not None] == list(D.MIXED_NB)
    assert D.reference("mixed/global-empty").status == 2
    assert D.reference("mixed/global-last_block_only").status == 1
    assert all(D.reference(c.name).status == 0 for c in rows if c.name.split("-")[-1].isdigit())
    assert max(len(D.reference(c.name).dets) for c in rows) > 8  # a capacity of 3 cuts some files, not all
    assert 0 < min(len(D.reference(c.name).dets) for c in rows if len(c.delta) >= 1023) and \
        any(0 < len(D.reference(c.name).dets) <= 3 for c in rows)


@pytest.mark.parametrize("bucket_us", [3600 * 10 ** 6, 600 * 10 ** 6])
def test_histogram_rows_meet_the_bucket_edges(bucket_us):
    starts = D.hist_starts(bucket_us)
    width = datetime.timedelta(microseconds=bucket_us)
    total = np.zeros(D.HIST_NBUCKETS, np.int64)
    bucket_of = {}
    for name in D.HIST_FILES:
        c = D.case(f"histogram/{name}")
        r = D.reference(c.name, D.HIST_BLOCK_SEC, starts[name])
        assert [(int(a["start"]), int(a["stop"])) for a in r.dets] == list(c.expect)
        bucket_of[name] = [(u - D.HIST_BASE) // width for u in r.utc]
        total += D.bucket_counts_ref(r.utc, D.HIST_BASE, bucket_us, D.HIST_NBUCKETS)
        if bucket_us == 3600 * 10 ** 6:  # the generalised helper is count_per_hour_ref on hour buckets
            rd, _ = O.get_detections_adaptive_ref(c.delta, c.k, D.HIST_BLOCK_SEC, wav_start_date_time=starts[name])
            per_hour = O.count_per_hour_ref(rd)
            want = [per_hour.get(D.HIST_BASE + b * width, 0) for b in range(D.HIST_NBUCKETS)]
            assert D.bucket_counts_ref(r.utc, D.HIST_BASE, bucket_us, D.HIST_NBUCKETS).tolist() == want
    r = D.reference("histogram/on_boundary", D.HIST_BLOCK_SEC, starts["on_boundary"])
    assert r.utc[0] == D.HIST_BASE + width and bucket_of["on_boundary"][0] == 1  # on the boundary: the later bucket
    r = D.reference("histogram/before_boundary", D.HIST_BLOCK_SEC, starts["before_boundary"])
    assert D.HIST_BASE + width - r.utc[0] == datetime.timedelta(seconds=0.2) and bucket_of["before_boundary"][0] == 0
    assert max(bucket_of["before_base"]) < 0 and max(bucket_of["far_before_base"]) < -2
    assert min(bucket_of["past_end"]) >= D.HIST_NBUCKETS
    assert set(bucket_of["across_bucket"]) == {2, 3}
    assert set(bucket_of["across_end"]) == {D.HIST_NBUCKETS - 1, D.HIST_NBUCKETS}
    assert set(bucket_of["across_base"]) == {-1, 0}
    assert total.sum() > 10


def test_generation_is_deterministic():
    for cls in D.CLASSES + ("mixed", "histogram"):
        again = D._GENERATORS[cls]()
        rows = D.cases(cls)
        assert [c.name for c in again] == [c.name for c in rows] and len({c.name for c in rows}) == len(rows)
        for a, b in zip(again, rows):
            assert a.k == b.k and a.cfg == b.cfg and a.expect == b.expect
            assert a.delta.tobytes() == b.delta.tobytes() and not b.delta.flags.writeable
    assert D.sweep_params() == D.sweep_params()


def test_total_blocks_stay_small():
    total = sum(len(c.delta) for cls in D.CLASSES + ("mixed", "histogram") for c in D.cases(cls))
    assert total < 300_000
