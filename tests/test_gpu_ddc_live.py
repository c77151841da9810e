"""GPU, end to end: the live detector fed from recordings that are not 4 kHz audio (meteorgpu.ddc).

90 s of synthetic 192 kHz int16 I/Q -- noise from meteorgpu.synth, three pings of different lengths at
f_signal, one of them across a push boundary, and a strong carrier 20 kHz away -- go through DdcLiveSession
in 30 s pushes with both audio dtypes; 90 s of 48 kHz int16 audio go through decimate_audio (D = 12).  The
meteors' times are identical to oracle.live_oracle run on the float64 reference's audio and the band dB is
within the project's flat 1e-9 dB.

The condition for that is checked first, on the CPU, from the references alone: the float64 and the
long-double audio give band dB within 1e-10 dB of each other, every decision clears its threshold by
1e-6 dB, and (int16 audio) no long-double value lies within the error bound of a half-integer, so that
rint of the GPU's value is rint of the reference's.
"""
import numpy as np
import pytest

import ddc_ref as R
from meteorgpu import _lib, ddc, live, synth
from oracle import live_oracle as L

pytestmark = pytest.mark.gpu

FS_IQ, F_SIGNAL, GAIN, SECS = 192000, 30000, 16.0, 90
PINGS = [(12.0, 0.6, 120.0), (29.4, 1.5, 90.0), (55.0, 3.0, 150.0)]  # (start s, length s, amplitude)


def _cfgs():
    cfg = live.ConfigDetection()
    return cfg, L.ConfigDetectionRef(**{k: getattr(cfg, k) for k in L.ConfigDetectionRef.__dataclass_fields__})


def _first_decision(nb, fs, cfg):
    B = int(cfg.proc_block_sec * fs)
    return next((b for b in range(nb) if (b * B) / fs >= cfg.init_detection_wait_sec), nb)


def _oracle(audio, scale, rcfg):
    """(meteors, thresholds, over, band dB) of the reference detector on 4 kHz audio"""
    x = audio.astype(np.float64) * scale
    bdb = L.welch_band_db_ref(x, 4000, rcfg)
    mets, thr, over = L.live_detect_ref(bdb, 4000, int(rcfg.proc_block_sec * 4000), rcfg)
    return mets, thr, over, bdb


def _condition(a64, ald, scale, cfg, rcfg):
    """the CPU-side condition on the two references; returns the float64 audio's oracle results"""
    mets, thr, over, bdb = _oracle(a64, scale, rcfg)
    bdb_ld = L.welch_band_db_ref(ald.astype(np.float64) * scale, 4000, rcfg)
    assert np.max(np.abs(bdb - bdb_ld)) <= 1e-10
    first = _first_decision(bdb.shape[1], 4000, cfg)
    ok = np.isfinite(over[first:]) & np.isfinite(thr[first:])
    assert np.min(np.abs(over[first:][ok] - thr[first:][ok])) > 1e-6
    assert len(mets) == len(PINGS)
    return mets, thr, over, bdb


@pytest.fixture(scope="module")
def iq_case():
    i, q, _ = synth.synth_iq(seed=41, fs=FS_IQ, duration_s=SECS, f0=0.0, sigma=300.0, rate_per_min=0.0)
    t = np.arange(len(i)) / FS_IQ
    z = 4000.0 * np.exp(2j * np.pi * (F_SIGNAL + 20000.0) * t)  # the strong carrier 20 kHz away
    for t0, d, amp in PINGS:
        sel = (t >= t0) & (t < t0 + d)
        z[sel] += amp * np.exp(2j * np.pi * F_SIGNAL * t[sel])
    i = np.clip(i + np.rint(z.real), -32768, 32767).astype(np.int16)
    q = np.clip(q + np.rint(z.imag), -32768, 32767).astype(np.int16)
    raw = ddc.interleave(i, q)
    cfg, taps = ddc.weaver(FS_IQ, F_SIGNAL, gain=GAIN)
    val = i.astype(np.float64) + 1j * q.astype(np.float64)
    args = (taps, int(cfg.decim), True, int(cfg.shift_num), int(cfg.shift_den), GAIN)
    a64 = R.ref_f64(val, *args)
    ald = R.ref_ld_long(val, *args)
    S = R.abs_sum(val, taps, int(cfg.decim))
    bound = _lib.ddc_chain(cfg) * R.U * GAIN * S
    return raw, a64, ald, bound


@pytest.mark.parametrize("audio_dtype", [np.float64, np.int16])
def test_iq_through_ddc_live_session(iq_case, audio_dtype):
    raw, a64, ald, bound = iq_case
    cfg, rcfg = _cfgs()
    scale = 1.0 / 32768.0
    if audio_dtype == np.int16:
        # rint of the reference: the same integer from both references, none near a half-integer
        frac = np.abs((ald - np.floor(ald)).astype(np.float64) - 0.5)
        assert np.all(frac > bound) and np.all(np.abs(ald) < 32767)
        ref_audio = np.rint(ald).astype(np.int16)
        assert np.array_equal(ref_audio, np.rint(a64).astype(np.int16))
        mets, thr, over, bdb = _condition(ref_audio, ref_audio, scale, cfg, rcfg)
    else:
        ref_audio = a64
        mets, thr, over, bdb = _condition(a64, ald, scale, cfg, rcfg)
    push = 30 * FS_IQ
    got, bands, audio = [], [], []
    with ddc.DdcLiveSession(FS_IQ, cfg, f_signal=F_SIGNAL, gain=GAIN, audio_dtype=audio_dtype, sample_scale=scale,
                            max_push_sec=31.0) as s:
        for a in range(0, len(raw) // 2, push):
            got += s.push(raw[2 * a: 2 * (a + push)])
            bands.append(s.session.last_band_db[0])
            audio.append(s.last_audio)
        got += s.flush()
        bands.append(s.session.last_band_db[0])
        audio.append(s.last_audio)
        assert s.meteors == got and s.blocks == bdb.shape[1] and not s.near_tie
        assert isinstance(s.state, (live.StateDetection, live.StateTracking, live.StateInitialization))
    audio = np.concatenate(audio)
    assert audio.dtype == np.dtype(audio_dtype) and len(audio) == len(ref_audio)
    if audio_dtype == np.int16:
        assert np.array_equal(audio, ref_audio)
    else:
        assert np.all(np.abs(audio.astype(R.LD) - ald).astype(np.float64) <= bound)
    # the meteors: the oracle's on the reference's audio, times and blocks identical
    assert [(m.time_start, m.time_stop, m.duration) for m in got] == [(m.time_start, m.time_stop, m.duration) for m in mets]
    # (the second ping lies across the first push boundary)
    assert any(m.time_start < 30.0 < m.time_stop for m in got)
    assert np.max(np.abs(np.concatenate(bands, axis=1) - bdb)) <= 1e-9
    # the detector on the GPU's own audio: bit-equal to a LiveSession fed that audio directly
    with live.LiveSession(4000, cfg, dtype=audio_dtype, sample_scale=scale, max_push_sec=100.0) as direct:
        want = direct.push(audio)
        assert want == got
        assert np.array_equal(direct.last_band_db[0], np.concatenate(bands, axis=1))


def test_48k_audio_through_decimate_audio():
    fs = 48000
    x, _ = synth.synth_real(seed=43, fs=fs, duration_s=SECS, f0=1000.0, sigma=300.0, rate_per_min=0.0)
    t = np.arange(len(x)) / fs
    add = np.zeros(len(x))
    for t0, d, amp in PINGS:
        sel = (t >= t0) & (t < t0 + d)
        add[sel] += 2 * amp * np.sin(2 * np.pi * 1000.0 * t[sel])
    x = np.clip(x + np.rint(add), -32768, 32767).astype(np.int16)
    cfg, rcfg = _cfgs()
    dcfg, taps = ddc.lowpass_decimator(fs, gain=4.0)
    assert int(dcfg.decim) == 12
    val = x.astype(np.float64)
    a64 = R.ref_f64(val, taps, 12, gain=4.0)
    ald = R.ref_ld_long(val, taps, 12, gain=4.0)
    scale = 1.0 / 32768.0
    mets, thr, over, bdb = _condition(a64, ald, scale, cfg, rcfg)
    audio = ddc.decimate_audio(x, fs, gain=4.0)
    bound = _lib.ddc_chain(dcfg) * R.U * 4.0 * R.abs_sum(val, taps, 12)
    assert np.all(np.abs(audio.astype(R.LD) - ald).astype(np.float64) <= bound)
    got_bdb = live.welch_band_db(audio, 4000, cfg, sample_scale=scale)
    assert np.max(np.abs(got_bdb - bdb)) <= 1e-9
    got, gthr, _ = live.live_detect(got_bdb, 4000, cfg)
    assert [(m.time_start, m.time_stop) for m in got] == [(m.time_start, m.time_stop) for m in mets]
    # pushed through the session in 30 s grabs as int16 audio: the same meteors
    with ddc.DdcLiveSession(fs, cfg, gain=4.0, audio_dtype=np.float64, sample_scale=scale, max_push_sec=31.0) as s:
        for a in range(0, len(x), 30 * fs):
            s.push(x[a: a + 30 * fs])
        s.flush()
        assert [(m.time_start, m.time_stop) for m in s.meteors] == [(m.time_start, m.time_stop) for m in mets]
