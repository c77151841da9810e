"""GPU, end to end: the live detector fed from recordings whose rate is no integer multiple of 4 kHz
(meteorgpu.resample), after tests/test_gpu_ddc_live.py.

Two recordings of 90 s, int16 audio at 6 kHz (the reference's phase-1 archive rate, ratio 2/3, 25 taps) and
at 44.1 kHz (a sound card, 40/441, 3529 taps), with the noise, seed, pings and gain of
test_48k_audio_through_decimate_audio, go through resample_audio and through ResampleLiveSession in 30 s
pushes with both audio dtypes.  The meteors' times are identical to oracle.live_oracle run on the float64
reference's audio and the band dB is within the project's flat 1e-9 dB.

The condition for that is checked first, on the CPU, from the references alone: the float64 and the
long-double audio give band dB within 1e-10 dB of each other, every decision clears its threshold by
1e-6 dB, the result is exactly three meteors, and (int16 audio) no long-double value lies within the error
bound of a half-integer, so that rint of the GPU's value is rint of the reference's.
"""
import numpy as np
import pytest

import resamp_ref as R
from meteorgpu import _lib, ddc, live, resample, synth
from oracle import live_oracle as L

pytestmark = pytest.mark.gpu

SECS, GAIN, SCALE = 90, 4.0, 1.0 / 32768.0
PINGS = [(12.0, 0.6, 120.0), (29.4, 1.5, 90.0), (55.0, 3.0, 150.0)]  # (start s, length s, amplitude)


def _cfgs():
    cfg = live.ConfigDetection()
    return cfg, L.ConfigDetectionRef(**{k: getattr(cfg, k) for k in L.ConfigDetectionRef.__dataclass_fields__})


def _first_decision(nb, fs, cfg):
    B = int(cfg.proc_block_sec * fs)
    return next((b for b in range(nb) if (b * B) / fs >= cfg.init_detection_wait_sec), nb)


def _oracle(audio, rcfg):
    """(meteors, thresholds, over, band dB) of the reference detector on 4 kHz audio"""
    x = audio.astype(np.float64) * SCALE
    bdb = L.welch_band_db_ref(x, 4000, rcfg)
    mets, thr, over = L.live_detect_ref(bdb, 4000, int(rcfg.proc_block_sec * 4000), rcfg)
    return mets, thr, over, bdb


def _condition(a64, ald, cfg, rcfg):
    """the CPU-side condition on the two references; returns the float64 audio's oracle results"""
    mets, thr, over, bdb = _oracle(a64, rcfg)
    bdb_ld = L.welch_band_db_ref(ald.astype(np.float64) * SCALE, 4000, rcfg)
    assert np.max(np.abs(bdb - bdb_ld)) <= 1e-10
    first = _first_decision(bdb.shape[1], 4000, cfg)
    ok = np.isfinite(over[first:]) & np.isfinite(thr[first:])
    assert np.min(np.abs(over[first:][ok] - thr[first:][ok])) > 1e-6
    assert len(mets) == len(PINGS) == 3
    return mets, thr, over, bdb


def _recording(fs):
    x, _ = synth.synth_real(seed=43, fs=fs, duration_s=SECS, f0=1000.0, sigma=300.0, rate_per_min=0.0)
    t = np.arange(len(x)) / fs
    add = np.zeros(len(x))
    for t0, d, amp in PINGS:
        sel = (t >= t0) & (t < t0 + d)
        add[sel] += 2 * amp * np.sin(2 * np.pi * 1000.0 * t[sel])
    return np.clip(x + np.rint(add), -32768, 32767).astype(np.int16)


_cases = {}


def _case(fs):
    """(recording, config, taps, float64 audio, long-double audio, error bound), computed once per rate"""
    if fs not in _cases:
        x = _recording(fs)
        rcfg, taps = resample.lowpass_resampler(fs, gain=GAIN)
        Lr, Mr = int(rcfg.up), int(rcfg.down)
        assert (Lr, Mr, int(rcfg.ntaps)) == {6000: (2, 3, 25), 44100: (40, 441, 3529)}[fs]
        val = x.astype(np.float64)
        a64 = R.ref_f64(val, taps, Lr, Mr, gain=GAIN)
        ald = R.ref_ld_long(val, taps, Lr, Mr, gain=GAIN)
        bound = _lib.resamp_chain(rcfg) * R.U * GAIN * R.abs_sum(val, taps, Lr, Mr)
        assert len(a64) == len(ald) == len(bound) == SECS * 4000
        _cases[fs] = (x, rcfg, taps, a64, ald, bound)
    return _cases[fs]


def _times(mets):
    return [(m.time_start, m.time_stop) for m in mets]


@pytest.mark.parametrize("fs", [6000, 44100])
def test_recording_through_resample_audio(fs):
    x, rcfg, taps, a64, ald, bound = _case(fs)
    cfg, ocfg = _cfgs()
    mets, thr, over, bdb = _condition(a64, ald, cfg, ocfg)
    audio = resample.resample_audio(x, fs, gain=GAIN)
    assert audio.dtype == np.float64 and len(audio) == len(ald)
    assert np.all(np.abs(audio.astype(R.LD) - ald).astype(np.float64) <= bound)
    got_bdb = live.welch_band_db(audio, 4000, cfg, sample_scale=SCALE)
    assert np.max(np.abs(got_bdb - bdb)) <= 1e-9
    got, _, _ = live.live_detect(got_bdb, 4000, cfg)
    assert _times(got) == _times(mets) and len(got) == 3
    for m, (t0, d, _) in zip(got, PINGS):  # the pings, to the detector's block of 0.2 s
        assert abs(m.time_start - t0) <= 0.4 and abs(m.time_stop - (t0 + d)) <= 0.4


@pytest.mark.parametrize("audio_dtype", [np.float64, np.int16])
@pytest.mark.parametrize("fs", [6000, 44100])
def test_recording_through_resample_live_session(fs, audio_dtype):
    x, rcfg, taps, a64, ald, bound = _case(fs)
    cfg, ocfg = _cfgs()
    if audio_dtype == np.int16:
        # rint of the reference: the same integer from both references, none near a half-integer
        frac = np.abs((ald - np.floor(ald)).astype(np.float64) - 0.5)
        assert np.all(frac > bound) and np.all(np.abs(ald) < 32767)
        ref_audio = np.rint(ald).astype(np.int16)
        assert np.array_equal(ref_audio, np.rint(a64).astype(np.int16))
        mets, thr, over, bdb = _condition(ref_audio, ref_audio, cfg, ocfg)
    else:
        mets, thr, over, bdb = _condition(a64, ald, cfg, ocfg)
    push = 30 * fs
    got, bands, audio = [], [], []
    with resample.ResampleLiveSession(fs, cfg, gain=GAIN, audio_dtype=audio_dtype, sample_scale=SCALE,
                                      max_push_sec=31.0) as s:
        assert isinstance(s, ddc.DdcLiveSession) and (s.fs_in, s.fs_out) == (fs, 4000)
        for a in range(0, len(x), push):
            got += s.push(x[a: a + push])
            bands.append(s.session.last_band_db[0])
            audio.append(s.last_audio)
        got += s.flush()
        bands.append(s.session.last_band_db[0])
        audio.append(s.last_audio)
        assert s.meteors == got and s.blocks == bdb.shape[1] and not s.near_tie
        assert isinstance(s.state, (live.StateDetection, live.StateTracking, live.StateInitialization))
        with pytest.raises(_lib.MsdError):  # flushed: the converter's stream needs a reset
            s.push(x[:10])
    audio = np.concatenate(audio)
    assert audio.dtype == np.dtype(audio_dtype) and len(audio) == SECS * 4000
    if audio_dtype == np.int16:
        assert np.array_equal(audio, ref_audio)
    else:  # the pushes' audio is the one pass's, bit for bit
        assert np.array_equal(audio, resample.resample_audio(x, fs, gain=GAIN))
    assert _times(got) == _times(mets) and len(got) == 3
    assert [m.duration for m in got] == [m.duration for m in mets]
    # (the second ping lies across the first push boundary)
    assert any(m.time_start < 30.0 < m.time_stop for m in got)
    assert np.max(np.abs(np.concatenate(bands, axis=1) - bdb)) <= 1e-9


def test_an_integer_ratio_is_decimate_audio_bit_for_bit():
    x48 = _recording(48000)[: 3 * 48000 + 77]
    for kw in (dict(gain=GAIN), dict(gain=0.5, out_dtype=np.int16), dict(ntaps=41)):
        a, b = resample.resample_audio(x48, 48000, **kw), ddc.decimate_audio(x48, 48000, **kw)
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # and the 6 kHz archive, which decimate_audio turns away
    with pytest.raises(ValueError):
        ddc.decimate_audio(x48[:6000], 6000)
    assert len(resample.resample_audio(x48[:6000], 6000)) == 4000
