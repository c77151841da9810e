"""The live detector's two device implementations (csrc/live.hip) against the oracle
(oracle/live_oracle.py) over the rows of tests/live_cases.py:

  one-shot   msd_live_detect_dev, the cases of one configuration in one launch (ld = max nb + 3, band
             rows NaN in [nb, ld), every output buffer prefilled with a sentinel), and msd_live_detect;
  session    LiveSession.push_rows under four cut schedules (one push, one block per push, cuts at every
             event block and the block after it, seeded sizes 0 .. 70 with empty pushes) for the cases of
             up to 700 blocks and pushes of 257 blocks for the longer ones; the cases of one
             configuration are the streams of one session, the shorter ones get empty pushes.

Every comparison is bit-exact, any NaN equal to any NaN at the same position (live_cases.same_floats),
so a sign of zero counts: over-noise values, thresholds used, counts, status, every field of every meteor
(the block indices against the replayed states), and the session's carried state after the last push.
No case is skipped: every case of every class goes through each form that applies to it.

Each class prints one line:  LIVE class: files, blocks, meteors, exact ties, longest history, non-finite
blocks.
"""
import ctypes as CT

import numpy as np
import pytest

from meteorgpu import _lib, dsp, live
from tests import live_cases as C

pytestmark = pytest.mark.gpu

SENT = 0xA5           # every byte of every output buffer before a launch
SESSION_MAX_NB = 700  # up to here a case takes the four schedules, above it pushes of CHUNK blocks
CHUNK = 257
SWEEP_PARTS = 5       # config_sweep's 150 configurations are 150 sessions: a fifth of them per test


def _cfg(c):
    return live.ConfigDetection(**{k: getattr(c.cfg, k) for k in C.CFG_FIELDS})


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENT).all())


def _same_meteors(got, want, name):
    assert len(got) == len(want), name
    for f in C.METEOR.names:
        if C.METEOR[f] == np.int64:
            assert got[f].tolist() == want[f].tolist(), (name, f)
        else:
            assert C.same_floats(got[f], want[f]), (name, f, got[f], want[f])


def _first_difference(got, want):
    bad = [b for b in range(len(want)) if not C.same_floats(got[b:b + 1], want[b:b + 1])]
    return (bad[0], got[bad[0]], want[bad[0]]) if bad else None


# ------------------------------------------------------------------ one-shot, batched
def _launch(group):
    """the cases of one configuration and capacity through one msd_live_detect_dev launch"""
    assert C.METEOR == _lib.METEOR_DTYPE
    ctx = dsp.context(0)
    c0, F = group[0], len(group)
    nbs = np.array([c.rows.shape[1] for c in group], np.int64)
    ld = int(nbs.max()) + 3
    cap = ld // 2 + 2 if c0.cap is None else c0.cap
    band = np.full((F, 3, ld), np.nan)
    for f, c in enumerate(group):
        band[f, :, :nbs[f]] = c.rows
    msz = C.METEOR.itemsize
    bufs = [ctx.alloc(n) for n in (F * 3 * ld * 8, F * 8, (F * cap + 1) * msz, F * 8, F * ld * 8, F * ld * 8, F * 4)]
    d_band, d_nb, d_met, d_cnt, d_thr, d_over, d_st = bufs
    for b in (d_met, d_cnt, d_thr, d_over, d_st):
        b.memset(SENT)
    d_band.upload(band)
    d_nb.upload(nbs)
    lc = live.live_cfg(c0.fs, _cfg(c0))
    assert (lc.block_size, lc.avg_win_blocks) == (c0.bs, C.win_blocks(c0.cfg))
    _lib.check(ctx.lib.msd_live_detect_dev(ctx.h, d_band.ptr, d_nb.ptr, F, ld, CT.byref(lc), d_met.ptr, cap,
                                           d_cnt.ptr, d_thr.ptr, d_over.ptr, d_st.ptr))
    counts = d_cnt.download(np.empty(F, np.int64))
    status = d_st.download(np.empty(F, np.int32))
    thr = d_thr.download(np.empty((F, ld)))
    over = d_over.download(np.empty((F, ld)))
    met = d_met.download(np.empty(F * cap + 1, C.METEOR))
    for b in bufs:
        b.free()
    for f, c in enumerate(group):
        r, nb = C.reference(c.name), int(nbs[f])
        assert _first_difference(over[f, :nb], r.over) is None, (c.name, "over", _first_difference(over[f, :nb], r.over))
        assert _first_difference(thr[f, :nb], r.thr) is None, (c.name, "thr", _first_difference(thr[f, :nb], r.thr))
        assert _untouched(over[f, nb:]) and _untouched(thr[f, nb:]), c.name  # nothing past nb is written
        n = len(r.meteors)
        assert counts[f] == n, (c.name, counts[f], n)  # the whole count, also past the capacity
        assert status[f] == (3 if n > cap else 0), (c.name, status[f])
        keep = min(n, cap)
        _same_meteors(met[f * cap:f * cap + keep], r.meteors[:keep], c.name)
        assert _untouched(met[f * cap + keep:(f + 1) * cap]), c.name  # nothing past min(count, cap)
    assert _untouched(met[F * cap:])


@pytest.mark.parametrize("cls", C.CLASSES)
def test_one_shot_batched(cls):
    rows = C.cases(cls)
    done = 0
    for group in C.groups(rows):
        _launch(group)
        done += len(group)
    assert done == len(rows)
    if cls == "capacity":
        assert sorted({g[0].cap for g in C.groups(rows)}) == [0, 1, C.CAP_COUNT - 1, C.CAP_COUNT, C.CAP_COUNT + 1]
    if cls == "lane_and_segment_edges":  # files of 0 .. 3000 blocks shared one launch
        assert any(sorted(c.rows.shape[1] for c in g) == sorted(C.EDGE_MIXED_NB) for g in C.groups(rows))
    print("\n" + C.summary_line(cls))


# ------------------------------------------------------------------ one-shot, host form
HOST_CASES = [f"lane_and_segment_edges/mixed-{nb}" for nb in (0, 1, 2)] + [c.name for c in C.cases("capacity")]


@pytest.mark.parametrize("name", HOST_CASES)
def test_one_shot_host_form(name):
    """msd_live_detect: MSD_ERR_CAPACITY exactly when the count exceeds cap, *count whole, the first cap
    meteors copied, nothing written past them or past nb"""
    ctx = dsp.context(0)
    c, r = C.case(name), C.reference(name)
    nb = c.rows.shape[1]
    cap = nb // 2 + 2 if c.cap is None else c.cap
    out = np.frombuffer(bytes([SENT]) * ((cap + 2) * C.METEOR.itemsize), C.METEOR).copy()
    thr, over = (np.frombuffer(bytes([SENT]) * ((nb + 2) * 8), np.float64).copy() for _ in range(2))
    count = CT.c_int64(-7)
    lc = live.live_cfg(c.fs, _cfg(c))
    rows = np.ascontiguousarray(c.rows)
    rc = ctx.lib.msd_live_detect(ctx.h, _lib.ptr(rows), nb, CT.byref(lc), _lib.ptr(out), cap, CT.byref(count),
                                 _lib.ptr(thr), _lib.ptr(over))
    n = len(r.meteors)
    assert rc == (_lib.MSD_ERR_CAPACITY if n > cap else _lib.MSD_OK), (name, rc)
    assert count.value == n
    keep = min(n, cap)
    _same_meteors(out[:keep], r.meteors[:keep], name)
    assert _untouched(out[keep:])
    assert C.same_floats(thr[:nb], r.thr) and C.same_floats(over[:nb], r.over)
    assert _untouched(thr[nb:]) and _untouched(over[nb:])


# ------------------------------------------------------------------ session
def _cuts_one(c, r):
    return [0, c.rows.shape[1]]


def _cuts_by_block(c, r):
    return list(range(c.rows.shape[1] + 1))


def _cuts_events(c, r):
    nb = c.rows.shape[1]
    return sorted({0, nb} | {x for b, _ in r.events for x in (b, b + 1) if x <= nb})


def _cuts_random(c, r):
    nb = c.rows.shape[1]
    rng = np.random.default_rng(sum(map(ord, c.name)))
    sizes = rng.integers(0, 71, nb // 20 + 8)
    sizes[::7] = 0
    return [0] + [int(x) for x in np.cumsum(sizes) if x < nb] + [nb]  # repeated cuts: empty pushes


def _cuts_chunk(c, r):
    nb = c.rows.shape[1]
    return list(range(0, nb, CHUNK)) + [nb]


SCHEDULES = {"one_push": _cuts_one, "by_block": _cuts_by_block, "event_cuts": _cuts_events,
             "random_cuts": _cuts_random}


def _session(group, cuts_of):
    """the cases of one configuration as the streams of one session, stream f cut by cuts_of"""
    c0, F = group[0], len(group)
    refs = [C.reference(c.name) for c in group]
    pieces = []
    for c, r in zip(group, refs):
        k = cuts_of(c, r)
        assert k[0] == 0 and k[-1] == c.rows.shape[1] and all(a <= b for a, b in zip(k[:-1], k[1:]))
        pieces.append(list(zip(k[:-1], k[1:])))
    P = max([b - a for p in pieces for a, b in p] + [1])
    nbmax = max(c.rows.shape[1] for c in group)
    pbs = c0.cfg.proc_block_sec
    overs, thrs, mets = ([[] for _ in range(F)] for _ in range(3))
    with live.LiveSession(c0.fs, _cfg(c0), nstreams=F, max_push_sec=(P + 0.5) * pbs,
                          hist_sec=(nbmax + 8) * pbs) as s:
        assert s.P >= P and s.H >= nbmax and (s.B, s.W) == (c0.bs, C.win_blocks(c0.cfg))
        for k in range(max(1, max(len(p) for p in pieces))):
            parts = [c.rows[:, p[k][0]:p[k][1]] if k < len(p) else None for c, p in zip(group, pieces)]
            got = s.push_rows(parts)
            for f in range(F):
                n = parts[f].shape[1] if parts[f] is not None else 0
                assert s.last_over[f].shape == s.last_thresholds[f].shape == (n,)
                overs[f].append(s.last_over[f])
                thrs[f].append(s.last_thresholds[f])
                mets[f] += [(k, m) for m in got[f]]
        raw, status = s.raw_state, list(s.status)
    for f, (c, r) in enumerate(zip(group, refs)):
        over, thr = np.concatenate(overs[f]), np.concatenate(thrs[f])
        assert _first_difference(over, r.over) is None and over.shape == r.over.shape, \
            (c.name, "over", _first_difference(over, r.over))
        assert _first_difference(thr, r.thr) is None, (c.name, "thr", _first_difference(thr, r.thr))
        assert len(mets[f]) == len(r.meteors), c.name
        for field in C.STATS:
            assert C.same_floats([getattr(m, field) for _, m in mets[f]], r.meteors[field]), (c.name, field)
        for (k, _), stop in zip(mets[f], r.meteors["stop_block"]):  # out of the push that holds its closing block
            assert pieces[f][k][0] <= stop < pieces[f][k][1], (c.name, k, stop)
        st = raw[f]
        state, trig, lock, until, t_start = r.final
        assert (st.state, st.status, st.blocks, st.trig, st.meteors) == \
            (state, 0, c.rows.shape[1], trig, len(r.meteors)), c.name
        assert C.same_floats([st.lock, st.until, st.t_start], [lock, until, t_start]), \
            (c.name, (st.lock, st.until, st.t_start), r.final)
        assert status[f] == 0


def _parts(cls):
    return range(SWEEP_PARTS if cls == "config_sweep" else 1)


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("cls,part", [(cls, p) for cls in C.CLASSES for p in _parts(cls)])
def test_session_pushes(cls, part, schedule):
    rows = [c for c in C.cases(cls) if c.rows.shape[1] <= SESSION_MAX_NB]
    groups = C.groups(rows, with_cap=False)
    n = len(_parts(cls))
    for group in groups[part::n]:
        _session(group, SCHEDULES[schedule])
    assert sum(len(g) for p in range(n) for g in groups[p::n]) == len(rows)


@pytest.mark.parametrize("cls", ["lane_and_segment_edges", "long_histories"])
def test_session_long_cases(cls):
    rows = [c for c in C.cases(cls) if c.rows.shape[1] > SESSION_MAX_NB]
    assert rows
    for group in C.groups(rows, with_cap=False):
        _session(group, _cuts_chunk)


def test_every_case_has_its_forms():
    """the split between the schedules and the long pushes leaves no case out"""
    long_classes = {cls for cls in C.CLASSES if any(c.rows.shape[1] > SESSION_MAX_NB for c in C.cases(cls))}
    assert long_classes == {"lane_and_segment_edges", "long_histories"}
