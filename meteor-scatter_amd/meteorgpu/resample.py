"""The down-converter at any rational ratio (include/msdsp.h, msd_resamp_*): a polyphase resampler by
up / down on the GPU, so that the live detector (``meteorgpu.live``, built for 4 kHz audio with the carrier
at 1 kHz) also runs on the 6 kHz archive (2/3), on 44.1 kHz sound-card audio (40/441) and on 250 kHz I/Q
(2/125), which ``meteorgpu.ddc`` turns away because it decimates by an integer only.

    audio = resample_audio(x6, 6000)                         # a 6 kHz archive file -> 4 kHz
    audio = iq_to_audio(i, q, 250000, 30000)                 # 250 kHz I/Q, carrier at +30 kHz -> 4 kHz
    cfg, taps = weaver_resampler(192000, 30000, fs_out=4100) # any rate the ratio limits allow
    with ResampleLiveSession(44100, ConfigDetection()) as s:
        for grab in grabs:                                   # int16 audio, any lengths
            meteors = s.push(grab)

numpy only.  All arithmetic is the library's (float64); nothing is resampled on the CPU.  An integer ratio
(up = 1) runs on ``ddc``'s plan with ``ddc``'s design, so its bits are ``ddc.decimate_audio``'s.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _lib, ddc
from .dsp import context

MAX_UP, MAX_DOWN, MAX_TAPS = 256, 1024, 4095


def ratio(fs_in, fs_out) -> tuple[int, int]:
    """(L, M) with fs_out / fs_in = L / M in lowest terms, from exact fractions"""
    r = Fraction(fs_out) / Fraction(fs_in)
    if r <= 0:
        raise ValueError("the sample rates must be positive")
    L, M = r.numerator, r.denominator
    if L > MAX_UP or M > MAX_DOWN:
        raise ValueError(f"fs_out / fs_in = {fs_out} / {fs_in} = {L} / {M}: up is at most {MAX_UP}, down at most {MAX_DOWN}")
    return L, M


def _ntaps(L: int, M: int, ntaps) -> int:
    if ntaps is not None:
        return int(ntaps)
    n = 8 * max(L, M) + 1
    if n > MAX_TAPS:
        raise ValueError(f"the default filter of the ratio {L} / {M} has {n} taps, above {MAX_TAPS}: pass ntaps")
    return n


def _from_ddc(dcfg: _lib.MsdDdcCfg) -> _lib.MsdResampCfg:
    return _lib.MsdResampCfg(dcfg.mode, 1, dcfg.decim, dcfg.ntaps, dcfg.out_dtype, 0, dcfg.shift_num, dcfg.shift_den,
                             dcfg.gain)


def _to_ddc(cfg: _lib.MsdResampCfg) -> _lib.MsdDdcCfg:
    return _lib.MsdDdcCfg(cfg.mode, cfg.down, cfg.ntaps, cfg.out_dtype, cfg.shift_num, cfg.shift_den, cfg.gain)


def lowpass_resampler(fs_in, fs_out=4000, ntaps: int | None = None, gain: float = 1.0, out_dtype=np.float64):
    """(config, taps) of the real resampler from ``fs_in`` to ``fs_out``: L times a low-pass at 0.9 of the
    lower of the two Nyquist frequencies, ``ntaps`` taps (default 8 max(L, M) + 1)."""
    L, M = ratio(fs_in, fs_out)
    if L == 1:
        dcfg, taps = ddc.lowpass_decimator(fs_in, fs_out, ntaps, gain, out_dtype)
        return _from_ddc(dcfg), taps
    ntaps = _ntaps(L, M, ntaps)
    taps = L * ddc.design_lowpass(ntaps, 0.9 / max(L, M))
    cfg = _lib.MsdResampCfg(_lib.DDC_REAL, L, M, ntaps, ddc._out_code(out_dtype), 0, 0, 1, float(gain))
    return cfg, taps


def weaver_resampler(fs_in, f_signal, fs_out=4000, f_tone=1000, ntaps: int | None = None, gain: float = 1.0,
                     out_dtype=np.float64):
    """(config, taps) of the single-sideband down-converter of ``ddc.weaver`` at any ratio: the tuning
    shift = (f_signal - f_tone + fs_out / 4) / fs_in as an exact fraction, L times a low-pass at
    0.9 min(fs_out / 4, fs_in / 2), ``ntaps`` taps (default 8 max(L, M) + 1)."""
    L, M = ratio(fs_in, fs_out)
    if L == 1:
        dcfg, taps = ddc.weaver(fs_in, f_signal, fs_out, f_tone, ntaps, gain, out_dtype)
        return _from_ddc(dcfg), taps
    shift = (Fraction(f_signal) - Fraction(f_tone) + Fraction(fs_out) / 4) / Fraction(fs_in)
    shift -= shift.numerator // shift.denominator  # into [0, 1)
    if shift.denominator > ddc.MAX_Q:
        raise ValueError(f"the tuning shift {shift} has a denominator above 2^24")
    ntaps = _ntaps(L, M, ntaps)
    taps = L * ddc.design_lowpass(ntaps, 0.9 * min(1.0 / (2 * M), 1.0 / L))
    cfg = _lib.MsdResampCfg(_lib.DDC_SSB, L, M, ntaps, ddc._out_code(out_dtype), 0, shift.numerator, shift.denominator,
                            float(gain))
    return cfg, taps


class Resampler(ddc.Ddc):
    """A resampler plan with ``nstreams`` streams: ``ddc.Ddc``'s samples, ``run``, ``push``, ``flush``,
    ``reset`` and ``close`` on an ``msd_resamp`` plan (``up`` = 1: on the ``msd_ddc`` plan of the same
    configuration)."""

    def __init__(self, cfg: _lib.MsdResampCfg, taps, nstreams: int = 1, max_push: int = 1 << 23, device: int = 0):
        self.cfg = cfg
        self.ssb = cfg.mode == _lib.DDC_SSB
        self.up, self.down = int(cfg.up), int(cfg.down)
        if self.up == 1:
            self.plan = _lib.DdcPlan(context(device), _to_ddc(cfg), taps, nstreams, max_push)
        else:
            self.plan = _lib.ResampPlan(context(device), cfg, taps, nstreams, max_push)
        self.max_push = int(max_push)


def resample_audio(x, fs, fs_out=4000, ntaps: int | None = None, gain: float = 1.0, out_dtype=np.float64,
                   device: int = 0) -> np.ndarray:
    """fs_out audio of int16 or float32 audio at ``fs`` (low-pass, resample by fs_out / fs)"""
    cfg, taps = lowpass_resampler(fs, fs_out, ntaps, gain, out_dtype)
    with Resampler(cfg, taps, nstreams=0, max_push=0, device=device) as r:
        return r.run(x)


def iq_to_audio(i, q, fs, f_signal, fs_out=4000, f_tone=1000, ntaps: int | None = None, gain: float = 1.0,
                out_dtype=np.float64, device: int = 0) -> np.ndarray:
    """fs_out audio of an I/Q recording (int16 or float32 I and Q at ``fs``) in which the carrier at
    ``f_signal`` is a tone at ``f_tone``"""
    cfg, taps = weaver_resampler(fs, f_signal, fs_out, f_tone, ntaps, gain, out_dtype)
    with Resampler(cfg, taps, nstreams=0, max_push=0, device=device) as r:
        return r.run(ddc.interleave(i, q))


class ResampleLiveSession(ddc.DdcLiveSession):
    """``ddc.DdcLiveSession`` at any ratio: the same arguments, attributes, ``push`` / ``flush`` / ``reset``
    and feed into the ``live.LiveSession``; the converter (``self.ddc``) is a ``Resampler`` stream."""

    def __init__(self, fs_in, config_detection, f_signal=None, fs_out=4000, f_tone=1000, ntaps: int | None = None,
                 gain: float = 1.0, audio_dtype=np.int16, sample_scale: float = 1.0 / 32768.0, max_push_sec: float = 60.0,
                 device: int = 0, **session_kw):
        from . import live
        self.audio_dtype = np.dtype(audio_dtype)
        if f_signal is None:
            cfg, taps = lowpass_resampler(fs_in, fs_out, ntaps, gain, self.audio_dtype)
        else:
            cfg, taps = weaver_resampler(fs_in, f_signal, fs_out, f_tone, ntaps, gain, self.audio_dtype)
        self.fs_in, self.fs_out = fs_in, fs_out
        self.ddc = Resampler(cfg, taps, nstreams=1, max_push=int(np.ceil(max_push_sec * float(fs_in))), device=device)
        self.session = live.LiveSession(fs_out, config_detection, nstreams=1, dtype=self.audio_dtype,
                                        sample_scale=sample_scale, max_push_sec=max_push_sec, device=device,
                                        **session_kw)
        self.meteors = []
        self.last_audio = np.zeros(0, self.audio_dtype)
