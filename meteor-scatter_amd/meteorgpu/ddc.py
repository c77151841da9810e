"""The receiver's last stage on the GPU (include/msdsp.h, msd_ddc_*): tune, low-pass, decimate and take
the single-sideband audio, so that the live detector (``meteorgpu.live``, built for 4 kHz audio with the
carrier at 1 kHz) runs on what is recorded: 48 kHz audio or wide-band I/Q.

    cfg, taps = weaver(192000, f_signal=30000)           # 192 kHz I/Q, carrier at +30 kHz -> 4 kHz audio
    audio = iq_to_audio(i, q, 192000, 30000)             # the carrier is a 1 kHz tone in it
    audio = decimate_audio(x48, 48000)                   # 48 kHz audio -> 4 kHz
    with DdcLiveSession(192000, ConfigDetection(), f_signal=30000) as s:
        for grab in grabs:                               # interleaved int16 I/Q, any lengths
            meteors = s.push(grab)

numpy only.  All arithmetic is the library's (float64); nothing is resampled on the CPU.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _lib
from .dsp import context

MAX_Q = 1 << 24


def design_lowpass(ntaps: int, cutoff: float) -> np.ndarray:
    """The Hamming-windowed sinc of ``scipy.signal.firwin(ntaps, cutoff)``: ``cutoff`` in units of the
    Nyquist frequency, unit gain at 0 Hz."""
    ntaps = int(ntaps)
    if ntaps < 1 or not 0.0 < cutoff < 1.0:
        raise ValueError("design_lowpass: ntaps >= 1 and 0 < cutoff < 1")
    m = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = cutoff * np.sinc(cutoff * m)
    if ntaps > 1:
        h = h * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(ntaps) / (ntaps - 1)))
    return h / np.sum(h)


def _decim(fs_in, fs_out) -> int:
    r = Fraction(fs_in) / Fraction(fs_out)
    if r.denominator != 1 or not 1 <= r <= 1024:
        raise ValueError(f"fs_in / fs_out = {fs_in} / {fs_out} must be an integer in 1 .. 1024")
    return int(r)


def _out_code(out_dtype) -> int:
    dt = np.dtype(out_dtype)
    if dt == np.float64:
        return _lib.MSD_F64
    if dt == np.int16:
        return _lib.MSD_I16
    raise TypeError("the down-converter's output is float64 or int16")


def weaver(fs_in, f_signal, fs_out=4000, f_tone=1000, ntaps: int | None = None, gain: float = 1.0,
           out_dtype=np.float64):
    """(config, taps) of the single-sideband down-converter that turns a carrier at ``f_signal`` Hz of I/Q
    sampled at ``fs_in`` into a real tone at ``f_tone`` Hz of audio sampled at ``fs_out``: the tuning
    shift = (f_signal - f_tone + fs_out / 4) / fs_in as an exact fraction, a low-pass at 0.9 fs_out / 4 of
    ``ntaps`` taps (default 8 D + 1).  Raises unless fs_in / fs_out is an integer and the shift is a
    fraction with a denominator of at most 2^24."""
    D = _decim(fs_in, fs_out)
    shift = (Fraction(f_signal) - Fraction(f_tone) + Fraction(fs_out) / 4) / Fraction(fs_in)
    shift -= shift.numerator // shift.denominator  # into [0, 1)
    if shift.denominator > MAX_Q:
        raise ValueError(f"the tuning shift {shift} has a denominator above 2^24")
    ntaps = 8 * D + 1 if ntaps is None else int(ntaps)
    taps = design_lowpass(ntaps, min(0.9 * (float(fs_out) / 4.0) / (float(fs_in) / 2.0), 0.999))
    cfg = _lib.MsdDdcCfg(_lib.DDC_SSB, D, ntaps, _out_code(out_dtype), shift.numerator, shift.denominator, float(gain))
    return cfg, taps


def lowpass_decimator(fs_in, fs_out=4000, ntaps: int | None = None, gain: float = 1.0, out_dtype=np.float64):
    """(config, taps) of the real decimator from ``fs_in`` to ``fs_out``: a low-pass at 0.9 of the output's
    Nyquist frequency, ``ntaps`` taps (default 8 D + 1)."""
    D = _decim(fs_in, fs_out)
    ntaps = 8 * D + 1 if ntaps is None else int(ntaps)
    taps = design_lowpass(ntaps, min(0.9 * float(fs_out) / float(fs_in), 0.999))
    cfg = _lib.MsdDdcCfg(_lib.DDC_REAL, D, ntaps, _out_code(out_dtype), 0, 1, float(gain))
    return cfg, taps


def interleave(i, q) -> np.ndarray:
    """int16 or float32 I and Q as the interleaved samples the library takes"""
    i, q = np.asarray(i), np.asarray(q)
    if i.shape != q.shape or i.ndim != 1:
        raise ValueError("I and Q must be 1-D arrays of one length")
    dt = np.int16 if i.dtype == np.int16 and q.dtype == np.int16 else np.float32
    out = np.empty(2 * i.shape[0], dt)
    out[0::2] = i
    out[1::2] = q
    return out


class Ddc:
    """A down-converter plan with ``nstreams`` streams.  Samples: REAL plans take 1-D int16 or float32;
    SSB plans take interleaved I/Q (1-D int16 or float32 of even length, or an [n][2] array) or complex64.
    ``run`` is one batch row; ``push`` / ``flush`` / ``reset`` drive a stream whose history stays on the
    GPU: pushes of any lengths followed by ``flush`` give ``run`` over the concatenation bit for bit."""

    def __init__(self, cfg: _lib.MsdDdcCfg, taps, nstreams: int = 1, max_push: int = 1 << 23, device: int = 0):
        self.cfg = cfg
        self.ssb = cfg.mode == _lib.DDC_SSB
        self.plan = _lib.DdcPlan(context(device), cfg, taps, nstreams, max_push)
        self.max_push = int(max_push)
        self.decim = int(cfg.decim)

    def _samples(self, x):
        """(contiguous array, dtype code, samples)"""
        x = np.asarray(x)
        if self.ssb:
            if x.dtype == np.complex64:
                x = np.ascontiguousarray(x).view(np.float32)
            x = np.ascontiguousarray(x).reshape(-1)
            if x.shape[0] % 2:
                raise ValueError("interleaved I/Q needs an even number of values")
            if x.dtype == np.int16:
                return x, _lib.MSD_CI16, x.shape[0] // 2
            if x.dtype == np.float32:
                return x, _lib.MSD_CF32, x.shape[0] // 2
            raise TypeError(f"I/Q samples are int16, float32 or complex64, got {x.dtype}")
        x = np.ascontiguousarray(x)
        if x.ndim != 1:
            raise ValueError("real samples must be 1-D")
        if x.dtype == np.int16:
            return x, _lib.MSD_I16, x.shape[0]
        if x.dtype == np.float32:
            return x, _lib.MSD_F32, x.shape[0]
        raise TypeError(f"real samples are int16 or float32, got {x.dtype}")

    def run(self, x, pos0: int = 0) -> np.ndarray:
        x, code, n = self._samples(x)
        return self.plan.run(x, code, n, pos0)

    def push(self, x, stream: int = 0) -> np.ndarray:
        x, code, n = self._samples(x)
        w = 2 if self.ssb else 1
        out = [self.plan.push(stream, x[w * a: w * min(n, a + self.max_push)], code, min(n, a + self.max_push) - a)
               for a in range(0, max(n, 1), self.max_push)]
        return out[0] if len(out) == 1 else np.concatenate(out)

    def flush(self, stream: int = 0) -> np.ndarray:
        return self.plan.flush(stream)

    def reset(self, stream: int | None = None, pos0: int = 0):
        self.plan.reset(-1 if stream is None else int(stream), pos0)

    def close(self):
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def iq_to_audio(i, q, fs, f_signal, fs_out=4000, f_tone=1000, ntaps: int | None = None, gain: float = 1.0,
                out_dtype=np.float64, device: int = 0) -> np.ndarray:
    """fs_out audio of an I/Q recording (int16 or float32 I and Q at ``fs``) in which the carrier at
    ``f_signal`` is a tone at ``f_tone``"""
    cfg, taps = weaver(fs, f_signal, fs_out, f_tone, ntaps, gain, out_dtype)
    with Ddc(cfg, taps, nstreams=0, max_push=0, device=device) as d:
        return d.run(interleave(i, q))


def decimate_audio(x, fs, fs_out=4000, ntaps: int | None = None, gain: float = 1.0, out_dtype=np.float64,
                   device: int = 0) -> np.ndarray:
    """fs_out audio of int16 or float32 audio at ``fs`` (low-pass, decimate)"""
    cfg, taps = lowpass_decimator(fs, fs_out, ntaps, gain, out_dtype)
    with Ddc(cfg, taps, nstreams=0, max_push=0, device=device) as d:
        return d.run(x)


class DdcLiveSession:
    """The live detector on a recording that is not 4 kHz audio: each push is down-converted on the GPU
    by a ``Ddc`` stream and the small audio is handed to a ``live.LiveSession`` (through the host: the
    session's near-tie guard needs the samples there anyway).  ``f_signal`` None: real audio at ``fs_in``
    is low-passed and decimated; else interleaved I/Q at ``fs_in`` is tuned to ``f_signal``.
    ``audio_dtype``: int16 (the session's int8 matrix-core Welch path) or float64.  The audio is in the
    input's units times ``gain``; ``sample_scale`` (default 1 / 32768) takes it to the detector's.

    ``push`` returns the meteors closed by it; ``flush`` pushes the converter's last outputs (the stream
    then needs ``reset``).  ``meteors``: all so far.  ``state``, ``blocks``, ``status``, ``near_tie``,
    ``min_margin``, ``decision_bound``: the session's, for its one stream.  ``last_audio``: the audio of
    the last push."""

    def __init__(self, fs_in, config_detection, f_signal=None, fs_out=4000, f_tone=1000, ntaps: int | None = None,
                 gain: float = 1.0, audio_dtype=np.int16, sample_scale: float = 1.0 / 32768.0, max_push_sec: float = 60.0,
                 device: int = 0, **session_kw):
        from . import live
        self.audio_dtype = np.dtype(audio_dtype)
        if f_signal is None:
            cfg, taps = lowpass_decimator(fs_in, fs_out, ntaps, gain, self.audio_dtype)
        else:
            cfg, taps = weaver(fs_in, f_signal, fs_out, f_tone, ntaps, gain, self.audio_dtype)
        self.fs_in, self.fs_out = fs_in, fs_out
        self.ddc = Ddc(cfg, taps, nstreams=1, max_push=int(np.ceil(max_push_sec * float(fs_in))), device=device)
        self.session = live.LiveSession(fs_out, config_detection, nstreams=1, dtype=self.audio_dtype,
                                        sample_scale=sample_scale, max_push_sec=max_push_sec, device=device,
                                        **session_kw)
        self.meteors = []
        self.last_audio = np.zeros(0, self.audio_dtype)

    def _feed(self, audio):
        self.last_audio = audio
        found = self.session.push(audio)
        self.meteors.extend(found)
        return found

    def push(self, x):
        return self._feed(self.ddc.push(x))

    def flush(self):
        return self._feed(self.ddc.flush())

    def reset(self):
        self.ddc.reset()
        self.session.reset()
        self.meteors = []
        self.last_audio = np.zeros(0, self.audio_dtype)

    state = property(lambda self: self.session.state[0])
    blocks = property(lambda self: self.session.blocks[0])
    status = property(lambda self: self.session.status[0])
    near_tie = property(lambda self: self.session.near_tie[0])
    min_margin = property(lambda self: self.session.min_margin[0])
    decision_bound = property(lambda self: self.session.decision_bound[0])

    def close(self):
        self.session.close()
        self.ddc.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
