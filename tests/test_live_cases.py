"""CPU: the generators of tests/live_cases.py deliver what they promise, by the oracle alone
(oracle/live_oracle.py).  tests/test_gpu_live_contract.py holds csrc/live.hip to the same rows.

The W = 0 row of long_histories is the slow one (the oracle converts a growing list for every block):
8392 blocks take about three seconds here, so its length stays as the class describes it."""
import numpy as np
import pytest

from tests import live_cases as C


def _kinds(r, kind):
    return [b for b, k in r.events if k == kind]


def _before(r, b):
    return r.states[b - 1][0] if b else "init"


def test_config_sweep_contains_every_listed_value():
    params = C.sweep_params()
    rows = C.cases("config_sweep")
    assert len(params) == len(rows) == C.SWEEP_N
    for col, values in enumerate((C.RATES, C.SWEEP_W, C.SWEEP_K, C.SWEEP_INIT, C.SWEEP_WAIT, C.SWEEP_MIN_DB,
                                  C.SWEEP_MIN_DUR), start=1):
        assert {p[col] for p in params} == set(values)
    assert all(150 <= p[0] <= 700 for p in params)
    for c, (nb, (fs, bs), W, k, tag, wait, min_db, min_dur) in zip(rows, params):
        g = c.cfg
        assert (c.rows.shape, c.fs, c.bs) == ((3, nb), fs, bs) and int(g.proc_block_sec * fs) == bs
        assert C.win_blocks(g) == W and g.threshold_std_factor == k and g.after_tracking_wait_sec == wait
        assert (g.detection_db_over_noise_mean_min, g.detection_dur_min_sec) == (min_db, min_dur)
        assert g.init_detection_wait_sec == C.init_wait(tag, nb, fs, bs)
        ends = _kinds(C.reference(c.name), "init_end")
        if tag == "0":
            assert ends == [0]
        elif tag == "block":
            assert ends == [1]
        elif tag == "file":
            assert ends == [] and C.reference(c.name).final[0] == 0
    refs = [C.reference(c.name) for c in rows]
    assert sum(len(r.meteors) for r in refs) > 500
    assert any(r.final[0] == 2 for r in refs) and any(r.final[0] == 1 for r in refs)


def test_value_ties_hold_exact_ties_whose_neighbours_decide_the_other_way():
    rows = C.cases("value_ties")
    assert {c.cfg.threshold_std_factor for c in rows} == {0.0, 4.0}
    n = dict.fromkeys(("det_tie", "det_above", "det_below", "trk_tie", "trk_above", "trk_below"), 0)
    for c in rows:
        if "closes" in c.expect:
            continue
        r = C.reference(c.name)
        for kind, blocks in c.expect.items():
            step = {"tie": 0, "above": 1, "below": -1}[kind[4:]]
            want = "detection" if kind[:3] == "det" else "tracking"
            for b in blocks:
                assert _before(r, b) == want, (c.name, kind, b)
                assert C.same_floats(r.over[b:b + 1], [C.ulps(r.thr[b], step)]), (c.name, kind, b)
                # strict both ways: a tie changes nothing, one ulp above starts Tracking, one ulp below ends it
                after = {"det_tie": "detection", "det_below": "detection", "det_above": "tracking",
                         "trk_tie": "tracking", "trk_above": "tracking", "trk_below": "detection"}[kind]
                assert r.states[b][0] == after, (c.name, kind, b)
                n[kind] += 1
        if "dyadic" in c.name:
            # fresh or locked, the threshold every probe meets is 2.5 bit for bit
            assert {float(r.thr[b]) for blocks in c.expect.values() for b in blocks} == {2.5}
        assert r.ties >= len(c.expect["det_tie"]) + len(c.expect["trk_tie"])
    assert min(n.values()) >= 8, n
    # rounded rows: the tied thresholds are not dyadic (real rounding in mean + k std)
    r = C.reference("value_ties/rounded-k4")
    assert all(float(r.thr[b]) * 2 ** 20 % 1 for b in C.case("value_ties/rounded-k4").expect["det_tie"])


def test_value_ties_mean_against_min_db_mean():
    emitted = {}
    for c in C.cases("value_ties"):
        if "closes" not in c.expect:
            continue
        r = C.reference(c.name)
        stops = set(r.meteors["stop_block"].tolist())
        assert [b for b, _ in c.expect["closes"]] == _kinds(r, "close")
        for (b, want), h in zip(c.expect["closes"], C.MEAN_TIE_HISTORIES):
            assert (b in stops) == want, (c.name, b)
            emitted.setdefault(c.name.rsplit("-", 1)[1], []).append(want)
            if want:
                m = r.meteors[r.meteors["stop_block"] == b][0]
                assert m["db_mean"] == np.mean(h) and b - m["start_block"] == len(h)
    # mean == 4.0 exactly in three histories; min_db_mean 4.0 takes them, one ulp up drops them
    assert emitted["eq"][:3] == [True] * 3 and emitted["up"][:3] == [False] * 3 and emitted["down"][:3] == [True] * 3
    assert emitted["eq"][3:5] == [True, False] and emitted["up"][3:5] == [True, False]
    assert emitted["down"][3:5] == [True, True]


def test_time_ties_lock_expiry_follows_the_rounding():
    hit = {"gt": 0, "lt": 0, "eq": 0}
    fired = {True: 0, False: 0}
    waits = set()
    for c in C.cases("time_ties"):
        if "lock" not in c.expect:
            continue
        r = C.reference(c.name)
        wait, off = c.cfg.after_tracking_wait_sec, c.expect["offset"]
        waits.add(wait)
        for close, p, rel in c.expect["lock"]:
            assert (close, "close") in r.events and _before(r, p) == "detection"
            until = C.t_start_of(close, c.fs, c.bs) + wait
            locked = until > C.t_end_of(p, c.fs, c.bs)
            assert (r.states[p][0] == "tracking") == locked, (c.name, close, p)
            lock = r.states[close][1]
            assert lock < r.over[p] and C.same_floats(r.thr[p:p + 1], [lock]) == locked
            if not locked:
                assert r.over[p] < r.thr[p]  # below the fresh threshold: the lock alone decides
            if off == 0 and wait > 0.2:
                assert locked == (rel == "gt")
                hit[rel] += 1
                fired[locked] += 1
            else:  # a block off the deciding one: no rounding reaches it
                assert locked == (off < 0)
    assert waits == {0.2, 0.4, 0.6}
    assert fired[True] >= 10 and fired[False] >= 10 and min(hit.values()) >= 10, (hit, fired)


def test_time_ties_duration_and_init():
    out, exact = {True: 0, False: 0}, 0
    for c in C.cases("time_ties"):
        r = C.reference(c.name)
        if "dur" in c.expect:
            md = c.cfg.detection_dur_min_sec
            stops = dict(zip(r.meteors["stop_block"].tolist(), r.meteors["start_block"].tolist()))
            assert _kinds(r, "trigger") == [s for s, _, _ in c.expect["dur"]]
            assert _kinds(r, "close") == [e for _, e, _ in c.expect["dur"]]
            for s, e, want in c.expect["dur"]:
                dur = C.t_start_of(e, c.fs, c.bs) - C.t_start_of(s, c.fs, c.bs)
                assert (e in stops) == want == bool(dur >= md), (c.name, s)
                if round(md / 0.2) == e - s:  # the tie: exactly min_dur / block_sec blocks
                    assert abs(dur - md) < 1e-12
                    out[want] += 1
        if "dur_exact" in c.expect:  # duration == min_dur bit for bit: emitted
            (m,) = r.meteors
            assert (m["start_block"], m["stop_block"]) == c.expect["dur_exact"]
            assert m["duration"] == c.cfg.detection_dur_min_sec
            exact += 1
        if "init_end" in c.expect:
            assert _kinds(r, "init_end") == [c.expect["init_end"]]
            b = c.expect["burst"]
            assert (r.states[b][0] == "tracking") == (c.expect["init_end"] < b)
    assert out[True] >= 10 and out[False] >= 10 and exact == 4, (out, exact)
    inits = [c.expect["init_end"] for c in C.cases("time_ties") if "init_end" in (c.expect or {})]
    assert sorted(set(inits)) == [7, 8, 41, 42] and len(inits) == 12


def test_edges_carry_their_events():
    rows = C.cases("lane_and_segment_edges")
    seen = {k: set() for k in ("init_end", "trigger", "close", "expiry")}
    for c in rows:
        r = C.reference(c.name)
        for kind in seen:
            for X in (c.expect or {}).get(kind, ()):
                assert (X, kind) in r.events, (c.name, kind, X)
                seen[kind].add(X)
                if kind == "expiry":  # the value planted there is above the lock that has just run out
                    lock = r.states[X - 1][1]
                    assert r.states[X][0] == "detection" and lock < r.over[X] < r.thr[X] and r.thr[X - 1] == lock
    assert seen["init_end"] >= set(C.EDGE_BLOCKS)
    assert seen["trigger"] >= set(C.EDGE_BLOCKS) - {0}
    assert seen["close"] >= set(C.EDGE_BLOCKS) - {0, 1} and seen["expiry"] >= set(C.EDGE_BLOCKS) - {0, 1}
    assert [c.rows.shape[1] for c in rows if "/mixed-" in c.name] == list(C.EDGE_MIXED_NB)
    assert len({C.cfg_key(c) for c in rows if "/mixed-" in c.name}) == 1
    # a run still open at the end emits nothing; a close on the last block does
    r = C.reference("lane_and_segment_edges/trigger-g0")
    assert r.final[0] == 2 and r.final[1] == C.EDGE_NB - 2 and r.meteors["stop_block"].max() < C.EDGE_NB - 2
    assert C.reference("lane_and_segment_edges/trigger-g1").final[:2] == (2, C.EDGE_NB - 1)
    r = C.reference("lane_and_segment_edges/close-g1")
    assert r.meteors["stop_block"][-1] == C.EDGE_NB - 1 and r.final[0] == 1
    for edges in (1, 2, 5):
        c = C.case(f"lane_and_segment_edges/run_across-{edges}")
        r = C.reference(c.name)
        a, e = c.expect["run"]
        assert [(m["start_block"], m["stop_block"]) for m in r.meteors] == [(a, e)]
        assert e // 256 - a // 256 == edges
    r = C.reference("lane_and_segment_edges/lock_200s")
    lock = r.states[250][1]
    assert all(s == ("detection", lock, 250 * 0.2 + 200.0) for s in r.states[250:1100])
    assert set(r.thr[251:1100].tolist()) == {lock} and 1100 // 256 - 250 // 256 == 4
    assert [b for b, k in r.events if k == "trigger" and b > 250] == [1100, 1300]
    assert _kinds(C.reference("lane_and_segment_edges/init_300"), "init_end") == [300]


def test_long_histories_have_the_listed_lengths():
    rows = C.cases("long_histories")
    w0 = rows[0]
    assert C.win_blocks(w0.cfg) == 0 and w0.rows.shape[1] == 8192 + 200
    r = C.reference(w0.name)
    assert r.longest == w0.rows.shape[1] - 1 and len(r.meteors) > 3
    assert r.thr[8300] != np.mean(r.over[108:8300]) + 4 * np.std(r.over[108:8300])  # all history, not a window
    lengths = []
    for c in rows[1:]:
        r = C.reference(c.name)
        assert [(m["start_block"], m["stop_block"]) for m in r.meteors] == list(c.expect["runs"]), c.name
        for m in r.meteors:
            a, e = int(m["start_block"]), int(m["stop_block"])
            lengths.append(e - a)
            assert m["db_mean"] == np.mean(r.over[a + 1:e + 1]) and m["db_std"] == np.std(r.over[a + 1:e + 1])
    assert tuple(lengths) == C.LONG_RUNS


def test_nonfinite_rows():
    rows = C.cases("nonfinite")
    nan_thr = odd_meteor = 0
    for c in rows:
        r = C.reference(c.name)
        if c.expect:
            assert not np.isfinite(r.over[c.expect["block"]]), c.name
            assert r.nonfinite == 1
        nan_thr += int(np.isnan(r.thr[1:]).any())
        odd_meteor += sum(1 for m in r.meteors if not all(np.isfinite(m[f]) for f in C.STATS))
    assert nan_thr >= 10 and odd_meteor >= 2
    assert {c.name.split("/")[1].rsplit("-", 1)[0] for c in rows if c.expect} >= set(C.NF_KINDS)
    by = {c.name.split("/")[1]: C.reference(c.name) for c in rows}
    assert np.isnan(by["all_neginf-window"].over[80]) and by["neginf_sig-window"].over[80] == -np.inf
    assert by["neginf_noise-later"].over[203] == np.inf
    # on the trigger block: +inf fires, NaN and -inf do not; inside a history
    assert by["posinf_sig-trigger"].states[200][0] == "tracking"
    assert by["nan_sig-trigger"].states[200][0] == by["neginf_sig-trigger"].states[200][0] == "detection"
    m = by["posinf_sig-later"].meteors
    m = m[m["start_block"] == 200][0]
    assert m["db_max"] == np.inf and m["db_mean"] == np.inf and np.isnan(m["db_std"])
    assert by["nan_sig-first"].states[206][0] == "detection" and 206 not in by["nan_sig-first"].meteors["stop_block"]
    r = by["lock_becomes_nan"]  # Tracking under a NaN lock never ends
    assert r.final[0] == 2 and np.isnan(r.final[2]) and r.final[1] == 120 and np.isnan(r.thr[121:]).all()
    for k in ("k0", "k4"):
        c, r = C.case(f"nonfinite/signed_zeros-{k}"), by[f"signed_zeros-{k}"]
        assert np.signbit(r.over[r.over == 0]).any() and not np.signbit(r.over[r.over == 0]).all()
        sig, n1, n2 = c.rows
        naive = sig - (-0.0 + n1 + n2) / 2.0  # a sum that starts at -0.0, as numpy's pairwise leaf alone does
        assert np.array_equal(naive, r.over) and not C.same_floats(naive, r.over)
        assert any(m["db_max"] == 0 and np.signbit(m["db_max"]) for m in r.meteors)
    m = by["signed_zeros-k4"].meteors[-1]  # a history of one -0.0: np.mean gives +0.0, min and max keep the sign
    assert m["db_mean"] == 0 and not np.signbit(m["db_mean"]) and np.signbit(m["db_min"]) and np.signbit(m["db_max"])
    assert by["signed_zeros-k4"].ties >= 1  # (and 2.0 meets a threshold of exactly 2.0)


def test_capacity_rows_have_their_count():
    rows = C.cases("capacity")
    assert sorted({c.cap for c in rows}) == [0, 1, C.CAP_COUNT - 1, C.CAP_COUNT, C.CAP_COUNT + 1]
    for c in rows:
        assert len(C.reference(c.name).meteors) == c.expect["count"] == C.CAP_COUNT
    assert len(C.groups(rows)) == 5 and len(C.groups(rows, with_cap=False)) == 1


def test_builder_is_the_oracle():
    """_Builder steps the oracle's loop: on its own rows the two give the same thresholds and values"""
    for cfg in (C.config(4000, 800, W=8, k=0.0, wait=0.4), C.config(44100, 4410, W=0, k=4.0, init=1.0, wait=12.0)):
        fs, bs = (4000, 800) if cfg.proc_block_sec == 0.2 else (44100, 4410)
        B = C._Builder(cfg, fs, bs)
        for v in C.random_rows(5, 300)[0]:
            B.push(v)
        with C._quiet():
            _, thr, over = C.L.live_detect_ref(B.rows(), fs, bs, cfg)
        assert C.same_floats(thr, B.thr) and C.same_floats(over, B.over)
        assert C.replay(thr, over, cfg, fs, bs)[-1][:2] == B.state[:2]


def test_replay_and_references_are_consistent():
    for cls in C.CLASSES:
        for c in C.cases(cls):
            r = C.reference(c.name)
            nb = c.rows.shape[1]
            assert r.thr.shape == r.over.shape == (nb,) and len(r.states) == nb
            assert not r.thr.flags.writeable and not c.rows.flags.writeable
            for m in r.meteors:  # the block indices reproduce the oracle's times
                assert C.t_start_of(int(m["start_block"]), c.fs, c.bs) == m["time_start"]
                assert r.states[m["stop_block"] - 1][0] == "tracking" and r.states[m["stop_block"]][0] == "detection"
                assert r.states[m["stop_block"] - 1][3] == m["start_block"]


def test_generation_is_deterministic():
    for cls in C.CLASSES:
        again = C._GENERATORS[cls]()
        rows = C.cases(cls)
        assert [c.name for c in again] == [c.name for c in rows] and len({c.name for c in rows}) == len(rows)
        for a, b in zip(again, rows):
            assert C.cfg_key(a) == C.cfg_key(b) and a.cap == b.cap and a.expect == b.expect
            assert a.rows.tobytes() == b.rows.tobytes()


def test_total_blocks_stay_small():
    assert sum(c.rows.shape[1] for cls in C.CLASSES for c in C.cases(cls)) < 200_000


@pytest.mark.parametrize("cls", C.CLASSES)
def test_summary_line(cls):
    line = C.summary_line(cls)
    assert line.startswith(f"LIVE {cls}: files {len(C.cases(cls))}, blocks ")
