"""Echo measurement: one record per batch detection from the one-sided spectrogram (include/msdsp.h a12,
csrc/echo.hip), and its conversion to physical units.

* ``measure_dev``  -- the device call on ``DeviceBuffer``s (spectrogram, detections and records stay in HBM)
* ``measure``      -- one file from host arrays, float32 or float64 spectrogram
* ``parameters``   -- records (from the GPU or from any restatement) to seconds, Hz and dB, host float64
* ``write_echo_csv`` -- the reference's six detection columns followed by the echo columns

The I/Q (two-sided) spectrogram and the live path are not covered.
"""
from __future__ import annotations

import csv
import ctypes as C

import numpy as np

from . import _lib
from .dsp import context

ECHO_DTYPE = _lib.ECHO_DTYPE
MAX_BAND = _lib.ECHO_MAX_BAND
FLAG_CLIPPED_BEFORE, FLAG_CLIPPED_AFTER, FLAG_NO_EFOLD, FLAG_PEAK_AT_EDGE = 1, 2, 4, 8
PARAM_FIELDS = ("t_peak_s", "peak_db", "snr_db", "f_peak_hz", "f_mean_hz", "drift_hz_per_s", "dur_3db_s", "rise_s",
                "efold_s", "energy", "flags")
PARAM_DTYPE = np.dtype([(n, np.int32 if n == "flags" else np.float64) for n in PARAM_FIELDS])
DETECTION_FIELDS = ("t_start", "t_stop", "dur_s", "dB", "utc_start", "utc_stop")


def echo_cfg(block_size: int, nperseg: int, hop: int, band_bins, noise_bins=(0, -1), pre_frames: int = 0,
             post_frames: int = 0) -> _lib.MsdEchoCfg:
    return _lib.MsdEchoCfg(int(block_size), int(nperseg), int(hop), int(band_bins[0]), int(band_bins[1]),
                           int(noise_bins[0]), int(noise_bins[1]), int(pre_frames), int(post_frames))


def measure_dev(ctx: _lib.Context, spec: _lib.DeviceBuffer, spec_dtype, nfiles: int, K: int,
                frames: _lib.DeviceBuffer, ld: int, dets: _lib.DeviceBuffer, cap: int, counts: _lib.DeviceBuffer,
                cfg: _lib.MsdEchoCfg, out: _lib.DeviceBuffer) -> None:
    """Enqueue msd_echo_measure_dev / _f64_dev on ``ctx``: spec [nfiles][K][ld] of ``spec_dtype``, frames and
    counts int64 [nfiles], dets / out [nfiles][cap]."""
    dt = np.dtype(spec_dtype)
    if dt not in (np.float32, np.float64):
        raise TypeError("the spectrogram must be float32 or float64")
    fn = ctx.lib.msd_echo_measure_f64_dev if dt == np.float64 else ctx.lib.msd_echo_measure_dev
    _lib.check(fn(ctx.h, spec.ptr, int(nfiles), int(K), frames.ptr, int(ld), dets.ptr, int(cap), counts.ptr,
                  C.byref(cfg), out.ptr))


def _dets(dets) -> np.ndarray:
    d = np.asarray(dets)
    if d.dtype == _lib.DET_DTYPE:
        return np.ascontiguousarray(d)
    d = np.asarray(dets, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(d.shape[0], _lib.DET_DTYPE)
    out["start"], out["stop"] = d[:, 0], d[:, 1]
    return out


def measure(spec, dets, *, block_size: int, nperseg: int, hop: int, band_bins, noise_bins=(0, -1),
            pre_frames: int = 0, post_frames: int = 0, frames: int | None = None, device: int = 0) -> np.ndarray:
    """One file on the GPU: ``spec`` [K][ld] float32 or float64 (columns at or past ``frames``, default all of
    them, are not read), ``dets`` the file's detections in blocks (DET_DTYPE, or rows of (start, stop)).
    Returns the records, ECHO_DTYPE [len(dets)]."""
    spec = np.asarray(spec)
    if spec.ndim != 2 or spec.dtype not in (np.float32, np.float64):
        raise TypeError("spec must be a float32 or float64 array [K][frames]")
    spec = np.ascontiguousarray(spec)
    d = _dets(dets)
    K, ld = spec.shape
    T = ld if frames is None else int(frames)
    cfg = echo_cfg(block_size, nperseg, hop, band_bins, noise_bins, pre_frames, post_frames)
    out = np.zeros(d.shape[0], ECHO_DTYPE)
    ctx = context(device)
    fn = ctx.lib.msd_echo_measure_f64 if spec.dtype == np.float64 else ctx.lib.msd_echo_measure
    _lib.check(fn(ctx.h, _lib.ptr(spec), int(K), T, int(ld), _lib.ptr(d), int(d.shape[0]), C.byref(cfg),
                  _lib.ptr(out)))
    return out


def parameters(raw, fs: float, nfft: int, hop: int, nperseg: int, band_bins, noise_bins=(0, -1)) -> np.ndarray:
    """Records to physical units (PARAM_DTYPE), all in host float64 from the record's fields:
    t_peak_s the centre of the peak frame; peak_db = 10 log10(p_peak); snr_db = the peak's power per band row
    over the span's noise power per frame and noise row, in dB (NaN without a noise band or with zero noise);
    f_peak_hz = (k_peak + d_peak) fs / nfft; f_mean_hz the power-weighted mean of the per-frame peak
    frequency; drift_hz_per_s its power-weighted least-squares slope (NaN when the span does not determine
    one); dur_3db_s the extent of the frames within 3 dB of the peak, first to last inclusive; rise_s from the
    first of them to the peak; efold_s from the peak to the first frame at or below 1/e of it (NaN when the
    span ends first, flag bit 2); energy = e_sig."""
    raw = np.asarray(raw, dtype=ECHO_DTYPE)
    fs, nfft, hop, nperseg = float(fs), int(nfft), int(hop), int(nperseg)
    k_lo = int(band_bins[0])
    nk = int(band_bins[1]) - k_lo + 1
    nn = max(0, int(noise_bins[1]) - int(noise_bins[0]) + 1)
    out = np.zeros(raw.shape[0], PARAM_DTYPE)
    hz, sec = fs / nfft, hop / fs
    with np.errstate(divide="ignore", invalid="ignore"):
        p, es = raw["p_peak"], raw["e_sig"]
        n = (raw["t1"] - raw["t0"]).astype(np.float64)
        out["t_peak_s"] = (nperseg / 2 + raw["t_peak"].astype(np.float64) * hop) / fs
        out["peak_db"] = 10.0 * np.log10(p)
        noise = raw["e_noise"] / (n * nn) if nn else np.full(raw.shape[0], np.nan)
        out["snr_db"] = np.where(noise > 0, 10.0 * np.log10((p / nk) / noise), np.nan)
        empty = raw["t1"] <= raw["t0"]
        out["f_peak_hz"] = np.where(empty, np.nan, (raw["k_peak"] + raw["d_peak"]) * hz)
        out["f_mean_hz"] = (k_lo + raw["w_r"] / es) * hz
        den = es * raw["w_uu"] - raw["w_u"] * raw["w_u"]
        slope = (es * raw["w_ur"] - raw["w_u"] * raw["w_r"]) / den  # bins per frame
        out["drift_hz_per_s"] = np.where(den > 0, slope * hz / sec, np.nan)
        out["dur_3db_s"] = np.where(empty, np.nan, (raw["t_half_last"] - raw["t_half_first"] + 1) * sec)
        out["rise_s"] = np.where(empty, np.nan, (raw["t_peak"] - raw["t_half_first"]) * sec)
        no_fold = empty | ((raw["flags"] & FLAG_NO_EFOLD) != 0)
        out["efold_s"] = np.where(no_fold, np.nan, (raw["t_efold"] - raw["t_peak"]) * sec)
    out["energy"] = es
    out["flags"] = raw["flags"]
    return out


def write_echo_csv(detections, echoes, path) -> None:
    """The reference's detection columns (dsp.write_csv: t_start, t_stop, dur_s, dB, utc_start, utc_stop)
    followed by PARAM_FIELDS, one row per detection; ``echoes`` is ``parameters()``'s output."""
    echoes = np.asarray(echoes, dtype=PARAM_DTYPE)
    if len(detections) != echoes.shape[0]:
        raise ValueError("one echo record per detection")
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(DETECTION_FIELDS) + list(PARAM_FIELDS))
        w.writeheader()
        for det, e in zip(detections, echoes):
            row = {"t_start": det.t_start, "t_stop": det.t_stop, "dur_s": det.dur_s, "dB": det.dB,
                   "utc_start": det.utc_start.isoformat() if det.utc_start else None,
                   "utc_stop": det.utc_stop.isoformat() if det.utc_stop else None}
            row.update({n: (int(e[n]) if n == "flags" else repr(float(e[n]))) for n in PARAM_FIELDS})
            w.writerow(row)
