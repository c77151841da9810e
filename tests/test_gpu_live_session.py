"""GPU: the resumable live session (include/msdsp.h, meteorgpu.live.LiveSession).

The defining property: for any split of a stream into pushes, the concatenated per-push outputs
(band dB rows, over-noise values, thresholds used, meteors and their order) are bit-identical to the
one-shot path on the concatenated input, which test_gpu_live.py holds to the oracle.  The reference
answer here is therefore the oracle's one-shot result on the whole stream."""
import ctypes
import math

import numpy as np
import pytest

from oracle import live_oracle as L
from tests.live_cases import replay as _replay

pytestmark = pytest.mark.gpu

STAT_TOL = 1e-9  # test_gpu_live.py's
FS, BS = 4000, 800


@pytest.fixture(scope="module")
def live():
    from meteorgpu import live as LV
    return LV


def _ref_cfg(c):
    return L.ConfigDetectionRef(**{k: getattr(c, k) for k in L.ConfigDetectionRef.__dataclass_fields__})


def _tuples(ms):
    return [(a.time_start, a.time_stop, a.duration, a.db_min, a.db_max, a.db_mean, a.db_std) for a in ms]


def _random_rows(seed, nb=600):
    """the recipe of test_gpu_live.py::test_state_machine_random_rows"""
    rng = np.random.default_rng(seed)
    sig = rng.normal(0, 1, nb)
    for s in rng.integers(50, nb - 10, 12):
        sig[s:s + rng.integers(1, 8)] += rng.uniform(5, 30)
    return np.stack([sig, rng.normal(0, 0.5, nb), rng.normal(0, 0.5, nb)])


def _push_all(sess, rows, cuts):
    """push rows[:, cuts[i]:cuts[i+1]] in turn through a one-stream session: (over, thr, [(push, meteor)],
    [(a, b)] block range of each push)"""
    overs, thrs, mets, ranges = [], [], [], []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        got = sess.push_rows(rows[:, a:b])
        assert sess.last_over[0].shape == (b - a,) and sess.last_thresholds[0].shape == (b - a,)
        assert np.array_equal(sess.last_band_db[0], rows[:, a:b])
        overs.append(sess.last_over[0])
        thrs.append(sess.last_thresholds[0])
        mets += [(k, m) for m in got]
        ranges.append((a, b))
    return np.concatenate(overs), np.concatenate(thrs), mets, ranges


def _check_against(over, thr, mets, ranges, ref):
    rm, rthr, rover = ref
    assert np.array_equal(over, rover, equal_nan=True)
    assert np.array_equal(thr, rthr, equal_nan=True)  # NaN positions included
    assert _tuples([m for _, m in mets]) == _tuples(rm)
    for k, m in mets:  # each meteor comes out of the push that holds its closing block
        close = int(round(m.time_stop * FS / BS))
        assert ranges[k][0] <= close < ranges[k][1], (k, close, ranges[k])


# ------------------------------------------------------------------ 1. row pushes equal one shot
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("kw", [dict(), dict(avg_win_sec=0.1), dict(after_tracking_wait_sec=0.0),
                                dict(detection_db_over_noise_mean_min=4, detection_dur_min_sec=0.4)])
def test_row_pushes_equal_one_shot(live, seed, kw):
    nb = 600
    rows = _random_rows(seed, nb)
    cfg = live.ConfigDetection(**kw)
    ref = L.live_detect_ref(rows, FS, BS, _ref_cfg(cfg))
    states = _replay(ref[1], ref[2], cfg)
    # the blocks where Init ends, one that triggers tracking and one that closes it
    init_end = next(b for b, s in enumerate(states) if s[0] != "init")
    trig = next(b for b, s in enumerate(states) if s[0] == "tracking")
    close = next(b for b in range(trig + 1, nb) if states[b][0] == "detection")
    key_cuts = sorted({0, nb} | {c for b in (init_end, trig, close) for c in (b, b + 1)})
    rng = np.random.default_rng(100 + seed)
    sizes = rng.integers(0, 71, 60)
    sizes[::7] = 0
    rand_cuts = [0] + [int(c) for c in np.cumsum(sizes) if c < nb] + [nb]
    # W = 0 (avg_win_sec 0.1: int(0.1 / 0.2)) keeps all history: hist_blocks >= 600
    with live.LiveSession(FS, cfg, max_push_sec=nb * 0.2, hist_sec=(nb + 8) * 0.2) as sess:
        assert sess.H >= nb and sess.P >= nb
        for cuts in ([0, nb], list(range(nb + 1)), rand_cuts, key_cuts):
            sess.reset()
            over, thr, mets, ranges = _push_all(sess, rows, cuts)
            _check_against(over, thr, mets, ranges, ref)
            assert sess.blocks == [nb] and sess.status == [0]
    assert len(ref[0]) > 0 or kw  # the default configuration finds meteors in every seed


# ------------------------------------------------------------------ 2. carried state, long pushes
@pytest.mark.parametrize("chunk", [1000, 257])
def test_long_pushes_carry_tracking_and_locks(live, chunk):
    """pushes longer than the one-shot path's 256-block segments, entered from a carried Tracking or
    locked Detection state (plateaus of 400 blocks, a 30 s lock after each)"""
    rng = np.random.default_rng(30 + 400)
    nb = 9000
    sig = rng.normal(0, 1, nb)
    for s in (300, 2100, 5050, 7777):
        sig[s:s + 400] += 30
    rows = np.stack([sig, rng.normal(0, 0.5, nb), rng.normal(0, 0.5, nb)])
    cfg = live.ConfigDetection(after_tracking_wait_sec=30.0)
    ref = L.live_detect_ref(rows, FS, BS, _ref_cfg(cfg))
    states = _replay(ref[1], ref[2], cfg)
    cuts = list(range(0, nb, chunk)) + [nb]
    assert any(states[c - 1][0] == "tracking" for c in cuts[1:-1])
    assert any(states[c - 1][0] == "detection" and states[c - 1][2] > c * 0.2 for c in cuts[1:-1]) or chunk == 1000
    with live.LiveSession(FS, cfg, max_push_sec=chunk * 0.2) as sess:
        assert sess.P == chunk
        over, thr, mets, ranges = _push_all(sess, rows, cuts)
    _check_against(over, thr, mets, ranges, ref)
    assert len(mets) >= 1


# ------------------------------------------------------------------ 3. streams are independent
def test_streams_are_independent(live):
    nbs = [600, 431, 517]
    rows = [_random_rows(10 + f, nb) for f, nb in enumerate(nbs)]
    cfg = live.ConfigDetection()
    refs = [L.live_detect_ref(r, FS, BS, _ref_cfg(cfg)) for r in rows]
    rng = np.random.default_rng(5)
    pos = [0, 0, 0]
    overs, thrs, mets = ([[] for _ in range(3)] for _ in range(3))
    with live.LiveSession(FS, cfg, nstreams=3, max_push_sec=80 * 0.2) as sess:
        call = 0
        while any(p < nb for p, nb in zip(pos, nbs)):
            take = [int(rng.integers(0, 81)) for _ in range(3)]
            take[call % 3] = 0  # one stream gets nothing in every call
            parts = [rows[f][:, pos[f]: pos[f] + take[f]] for f in range(3)]
            if call % 5 == 0:
                parts[(call + 1) % 3] = parts[(call + 1) % 3] if parts[(call + 1) % 3].shape[1] else None
            got = sess.push_rows(parts)
            assert len(got) == 3 and got[call % 3] == []
            for f in range(3):
                n = 0 if parts[f] is None else parts[f].shape[1]
                assert sess.last_over[f].shape == (n,)
                overs[f].append(sess.last_over[f])
                thrs[f].append(sess.last_thresholds[f])
                mets[f] += got[f]
                pos[f] += n
            call += 1
        assert sess.blocks == nbs
    for f in range(3):
        assert np.array_equal(np.concatenate(overs[f]), refs[f][2], equal_nan=True)
        assert np.array_equal(np.concatenate(thrs[f]), refs[f][1], equal_nan=True)
        assert _tuples(mets[f]) == _tuples(refs[f][0])
    assert sum(len(r[0]) for r in refs) > 0


# ------------------------------------------------------------------ 4. state getter
def test_state_getter_mid_tracking(live):
    rng = np.random.default_rng(7)
    nb = 300
    sig = rng.normal(0, 1, nb)
    sig[120:180] += 25
    rows = np.stack([sig, rng.normal(0, 0.5, nb), rng.normal(0, 0.5, nb)])
    cfg = live.ConfigDetection()
    _, rthr, rover = L.live_detect_ref(rows, FS, BS, _ref_cfg(cfg))
    states = _replay(rthr, rover, cfg)
    stop = 150  # blocks pushed: the last one is block 149, inside the plateau
    want = states[stop - 1]
    assert want[0] == "tracking" and want[3] == 120
    with live.LiveSession(FS, cfg, max_push_sec=20.0) as sess:
        assert isinstance(sess.state[0], live.StateInitialization)
        sess.push_rows(rows[:, :20])
        assert isinstance(sess.state[0], live.StateInitialization)
        sess.push_rows(rows[:, 20:90])
        st = sess.state[0]
        assert st == live.StateDetection(-1.0, -1.0)
        sess.push_rows(rows[:, 90:stop])
        raw = sess.raw_state[0]
        assert (raw.state, raw.status, raw.blocks, raw.trig) == (2, 0, stop, want[3])
        assert (raw.lock, raw.t_start) == (want[1], want[2])
        assert raw.meteors == 0 and raw.retained == stop - (stop - sess.W) == sess.W
        st = sess.state[0]
        assert isinstance(st, live.StateTracking)
        assert (st.locked_threshold, st.time_start_detection) == (want[1], want[2])
        assert st.history_over_noise_sig_dB == rover[want[3] + 1: stop].tolist()
        assert sess.blocks == [stop]
        # tracking ends: the locked Detection state of the oracle
        sess.push_rows(rows[:, stop:200])
        end = states[199]
        assert end[0] == "detection"
        assert sess.state[0] == live.StateDetection(end[1], end[2])
        assert sess.raw_state[0].meteors == 1


# ------------------------------------------------------------------ 5. history overflow
def test_history_overflow_freezes_one_stream(live):
    """a signal that stays above its lock (a continuous carrier): once the open tracking run no longer
    fits in hist_blocks the stream reports status 4 and is frozen until reset; the other stream goes on"""
    rng = np.random.default_rng(21)
    nb = 400
    sig = rng.normal(0, 1, nb)
    sig[100:300] += 30
    carrier = np.stack([sig, rng.normal(0, 0.5, nb), rng.normal(0, 0.5, nb)])
    other = _random_rows(22, nb)
    cfg = live.ConfigDetection()
    refs = [L.live_detect_ref(r, FS, BS, _ref_cfg(cfg)) for r in (carrier, other)]
    states = _replay(refs[0][1], refs[0][2], cfg)
    step = 10
    with live.LiveSession(FS, cfg, nstreams=2, max_push_sec=step * 0.2, hist_sec=(40 + 8) * 0.2) as sess:
        W, H = sess.W, sess.H
        assert (W, H) == (40, 48)
        # the documented rule: after a push that ends at block e, everything from
        # keep = min(e - W, trig while Tracking) on stays; more than hist_blocks values: status 4
        def kept(e):
            s = states[e - 1]
            keep = max(0, e - W)
            if s[0] == "tracking":
                keep = min(keep, s[3])
            return e - keep
        e_over = next(e for e in range(step, nb + 1, step) if kept(e) > H)
        assert states[e_over - 1][0] == "tracking" and 100 < e_over < 300
        overs, thrs, mets = ([[], []] for _ in range(3))
        for a in range(0, nb, step):
            got = sess.push_rows([carrier[:, a:a + step], other[:, a:a + step]])
            for f in range(2):
                overs[f].append(sess.last_over[f])
                thrs[f].append(sess.last_thresholds[f])
                mets[f] += got[f]
            e = a + step
            if e < e_over:
                assert sess.status == [0, 0]
            elif e == e_over:  # found at the end of this push, whose own outputs are still valid
                assert sess.status == [4, 0] and sess.last_over[0].shape == (step,)
            else:  # frozen: nothing consumed, nothing emitted, 4 again
                assert sess.status == [4, 0] and got[0] == [] and sess.last_over[0].shape == (0,)
                assert sess.last_thresholds[0].shape == (0,)
        assert sess.blocks == [e_over, nb]
        raw = sess.raw_state
        assert (raw[0].status, raw[0].state, raw[0].blocks) == (4, 2, e_over) and raw[1].status == 0
        # the frozen stream's outputs up to the overflow, the other stream's whole run
        assert np.array_equal(np.concatenate(overs[0]), refs[0][2][:e_over], equal_nan=True)
        assert np.array_equal(np.concatenate(thrs[0]), refs[0][1][:e_over], equal_nan=True)
        assert mets[0] == []
        assert np.array_equal(np.concatenate(overs[1]), refs[1][2], equal_nan=True)
        assert np.array_equal(np.concatenate(thrs[1]), refs[1][1], equal_nan=True)
        assert _tuples(mets[1]) == _tuples(refs[1][0]) and len(mets[1]) > 0
        # reset: the stream behaves as a fresh session's (the other stream's state stays)
        sess.reset(0)
        assert sess.status == [0, 0] and sess.blocks == [0, nb]
        assert isinstance(sess.state[0], live.StateInitialization)
        o2, t2, m2 = [], [], []
        for a in range(0, nb, step):
            got = sess.push_rows([other[:, a:a + step], None])
            o2.append(sess.last_over[0])
            t2.append(sess.last_thresholds[0])
            m2 += got[0]
        assert sess.status == [0, 0] and sess.blocks == [nb, nb]
        assert np.array_equal(np.concatenate(o2), refs[1][2], equal_nan=True)
        assert np.array_equal(np.concatenate(t2), refs[1][1], equal_nan=True)
        assert _tuples(m2) == _tuples(refs[1][0])


# ------------------------------------------------------------------ 6. samples end to end
@pytest.fixture(scope="module")
def audio():
    from meteorgpu import synth
    x, _ = synth.synth_real(seed=77, fs=4000, duration_s=90.0, f0=1020.0, sigma=300.0, rate_per_min=10,
                            band_hz=100.0, snr_db=(15, 30), dur_s=(0.4, 2.0))
    return x


def _e2e_cfg(live):
    return live.ConfigDetection(proc_block_sec=0.2, n_fft=4096, detection_db_over_noise_mean_min=1,
                                detection_dur_min_sec=0.5, signal_freq=1020)


def _push_chunks(sess, x):
    sizes = [12345, 1, 799, 800, 801, 0]
    cuts = [0] + list(np.cumsum(sizes)) + [len(x)]
    bands, thrs, overs, mets = [], [], [], []
    carried = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        mets += sess.push(x[a:b])
        n = (carried + (b - a)) // BS
        carried = (carried + (b - a)) % BS
        assert sess.last_band_db[0].shape == (3, n)
        bands.append(sess.last_band_db[0])
        thrs.append(sess.last_thresholds[0])
        overs.append(sess.last_over[0])
    assert sess.raw_state[0].remainder == carried == len(x) % BS
    return np.concatenate(bands, axis=1), np.concatenate(thrs), np.concatenate(overs), mets


def test_samples_end_to_end_int16(live, audio, tmp_path):
    from meteorgpu import wav
    x, cfg = audio, _e2e_cfg(live)
    with live.LiveSession(FS, cfg, max_push_sec=90.0) as sess:
        bdb, thr, over, mets = _push_chunks(sess, x)
        assert sess.blocks == [len(x) // BS] and sess.status == [0]
        margins = (sess.near_tie[0], sess.min_margin[0], sess.decision_bound[0])
    one = live.welch_band_db(x, FS, cfg, sample_scale=1 / 32768)
    assert np.array_equal(bdb, one)
    m1, thr1, over1 = live.live_detect(one, FS, cfg)
    assert np.array_equal(thr, thr1, equal_nan=True) and np.array_equal(over, over1, equal_nan=True)
    assert _tuples(mets) == _tuples(m1)
    ref, _, _ = L.wav_file_process_ref(x.astype(np.float64) / 32768.0, FS, _ref_cfg(cfg))
    assert len(ref) > 0 and len(mets) == len(ref)
    for a, b in zip(mets, ref):
        assert (a.time_start, a.time_stop, a.duration) == (b.time_start, b.time_stop, b.duration)
        for f in ("db_min", "db_max", "db_mean", "db_std"):
            assert math.isclose(getattr(a, f), getattr(b, f), rel_tol=STAT_TOL, abs_tol=STAT_TOL)
    # the cumulative near-tie guard ends at the one-shot values
    p = tmp_path / "live.wav"
    wav.write(p, FS, x)
    got = live.wav_file_process(str(p), cfg, live.ConfigVisualization(enable_ui_plots=False),
                                live.ConfigSpecExport(output_dir=""))
    assert margins == (got.near_tie, got.min_margin, got.decision_bound)
    assert not margins[0] and 0 < margins[2] < 1e-6 and margins[1] > margins[2]


def test_samples_end_to_end_float64(live, audio):
    from meteorgpu import margin as M
    cfg = _e2e_cfg(live)
    x = audio.astype(np.float64) / 32768.0
    with live.LiveSession(FS, cfg, dtype=np.float64, sample_scale=1.0, max_push_sec=90.0) as sess:
        bdb, thr, over, mets = _push_chunks(sess, x)
        margins = (sess.near_tie[0], sess.min_margin[0], sess.decision_bound[0])
    one = live.welch_band_db(x, FS, cfg, sample_scale=1.0)
    assert np.array_equal(bdb, one)
    m1, thr1, over1 = live.live_detect(one, FS, cfg)
    assert np.array_equal(thr, thr1, equal_nan=True) and np.array_equal(over, over1, equal_nan=True)
    assert _tuples(mets) == _tuples(m1) and len(m1) > 0
    span = M.block_span(x, BS, 1.0)[: one.shape[1]]
    assert margins == live.near_tie_check(one, thr1, over1, span, FS, cfg, warn=False)


def test_uint8_samples_and_split_long_push(live, audio):
    """8-bit audio is shifted as the one-shot path shifts it; a push longer than max_push_sec is split"""
    cfg = _e2e_cfg(live)
    x8 = (np.clip(audio[: 20 * FS] // 64, -128, 127) + 128).astype(np.uint8)
    dev, scale = live._device_samples(x8)
    one = live.welch_band_db(dev, FS, cfg, sample_scale=scale)
    with live.LiveSession(FS, cfg, dtype=np.uint8, sample_scale=scale, max_push_sec=3.0) as sess:
        assert sess.P == 15
        sess.push(x8[:1234])
        first = sess.last_band_db[0]
        sess.push(x8[1234:])  # 99 blocks through a session that takes 15 per device push
        assert np.array_equal(np.concatenate([first, sess.last_band_db[0]], axis=1), one)
        assert sess.blocks == [one.shape[1]]
        with pytest.raises(TypeError):
            sess.push(audio[:100])


# ------------------------------------------------------------------ the C-ABI's host forms
def test_host_forms_one_stream_at_a_time(live, audio):
    from meteorgpu import _lib
    from meteorgpu.dsp import context
    cfg = live.ConfigDetection()
    rows = _random_rows(3)
    nb = rows.shape[1]
    rm, rthr, rover = L.live_detect_ref(rows, FS, BS, _ref_cfg(cfg))
    assert len(rm) >= 2
    ctx = context(0)
    lib = ctx.lib
    lc = live.live_cfg(FS, cfg)
    wc, win = live.welch_cfg(FS, cfg, 1 / 32768)
    h = ctypes.c_void_p()
    _lib.check(lib.msd_live_session_create(ctx.h, ctypes.byref(lc), ctypes.byref(wc), _lib.ptr(win), 2, 256, 64,
                                           _lib.MSD_I16, ctypes.byref(h)))
    try:
        out = np.zeros(64, _lib.METEOR_DTYPE)
        thr, over = np.empty(256), np.empty(256)
        cnt, stat, newb = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        got, thrs, overs = [], [], []
        for a in range(0, nb, 250):  # stream 1 only
            part = np.ascontiguousarray(rows[:, a:a + 250])
            _lib.check(lib.msd_live_session_push_rows(h, 1, _lib.ptr(part), part.shape[1], _lib.ptr(out), 64,
                                                      ctypes.byref(cnt), _lib.ptr(thr), _lib.ptr(over),
                                                      ctypes.byref(stat)))
            assert stat.value == 0
            got += [(r["start_block"], r["stop_block"], r["time_start"], r["time_stop"], r["db_mean"])
                    for r in out[: cnt.value]]
            thrs.append(thr[: part.shape[1]].copy())
            overs.append(over[: part.shape[1]].copy())
        assert np.array_equal(np.concatenate(thrs), rthr, equal_nan=True)
        assert np.array_equal(np.concatenate(overs), rover, equal_nan=True)
        assert [(g[2], g[3], g[4]) for g in got] == [(m.time_start, m.time_stop, m.db_mean) for m in rm]
        assert [g[1] for g in got] == [int(round(m.time_stop * FS / BS)) for m in rm]  # global block indices
        st = (_lib.MsdLiveStreamState * 2)()
        _lib.check(lib.msd_live_session_state(h, 0, 2, st))
        assert (st[0].blocks, st[0].state, st[1].blocks, st[1].meteors) == (0, 0, nb, len(rm))
        # more meteors in one push than cap: status 3, MSD_ERR_CAPACITY, the count still whole
        _lib.check(lib.msd_live_session_reset(h, 1))
        part = np.ascontiguousarray(rows[:, :256])
        n256 = sum(1 for m in rm if round(m.time_stop * FS / BS) < 256)
        assert n256 >= 2
        rc = lib.msd_live_session_push_rows(h, 1, _lib.ptr(part), 256, _lib.ptr(out), 1, ctypes.byref(cnt), None,
                                            None, ctypes.byref(stat))
        assert rc == _lib.MSD_ERR_CAPACITY and stat.value == 3 and cnt.value == n256
        assert out[0]["time_start"] == rm[0].time_start
        # samples, stream 0: 3 pushes with remainders
        x = np.ascontiguousarray(audio[: 30 * FS + 123])
        cfg6 = live.ConfigDetection()
        one = live.welch_band_db(x, FS, cfg6, sample_scale=1 / 32768)
        band = np.empty((3, 256))
        parts = []
        for a, b in ((0, 801), (801, 50000), (50000, len(x))):
            seg = np.ascontiguousarray(x[a:b])
            rc = lib.msd_live_session_push_samples(h, 0, _lib.ptr(seg), len(seg), _lib.ptr(out), 64,
                                                   ctypes.byref(cnt), ctypes.byref(newb), _lib.ptr(band), None, None,
                                                   256, ctypes.byref(stat))
            _lib.check(rc)
            parts.append(band[:, : newb.value].copy())
        assert np.array_equal(np.concatenate(parts, axis=1), one)
        _lib.check(lib.msd_live_session_state(h, 0, 2, st))
        assert (st[0].blocks, st[0].remainder) == (one.shape[1], len(x) % BS)
        hist = np.empty(64 + 256)
        n = ctypes.c_int64(0)
        _lib.check(lib.msd_live_session_history(h, 0, _lib.ptr(hist), hist.size, ctypes.byref(n)))
        assert n.value == st[0].retained >= 40
        # argument checks on a real session
        assert lib.msd_live_session_push_rows(h, 2, _lib.ptr(part), 1, _lib.ptr(out), 1, ctypes.byref(cnt), None,
                                              None, None) == _lib.MSD_ERR_INVALID
        assert lib.msd_live_session_push_rows(h, 0, _lib.ptr(part), 257, _lib.ptr(out), 1, ctypes.byref(cnt), None,
                                              None, None) == _lib.MSD_ERR_INVALID
    finally:
        lib.msd_live_session_destroy(h)
