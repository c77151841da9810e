"""Legacy pipeline pieces: the spectrogram and noise floor of
meteor_detect_class/prime_detection.py:65-91, on the GPU.

``specgram`` mirrors ``matplotlib.mlab.specgram`` (what ``plt.specgram`` computes) for a
real 1-D signal: symmetric Hann (``window_hanning``), no detrend, one-sided PSD with the
DC / Nyquist rows undoubled, ``/Fs/sum(w**2)``, zero padding to NFFT for a signal shorter than
NFFT — on libmsdsp's float64 STFT (``stft_any.hip``), the precision mlab computes in
(mlab.py:299-356); agreement with mlab is at the 1e-12 level (tested).
``noise_floor`` adds the band power over the noise band's rows and all frames
(``np.sum(Pxx[noise_band])``, a device reduction) and the reference's colour floor
``vmin = 10*log10(band_power/bandwidth) / (40/23) + C_MS_SPEC_CUT_FACTOR``.

``detect_and_cluster_bursts_spec`` adds the stage that follows in the reference
(meteor_detect_class/detector_and_classification.py:7-91): points on the 800-1200 Hz spectrogram,
``DBSCAN(eps=30, min_samples=5)``, a box per cluster and the critical rule (extent along time >= 5 px), the
``Anzahl`` / ``Kritisch`` columns of the hourly CSV.  DBSCAN, the boxes and the critical rule are the
reference's exactly (``meteorgpu.cluster``, csrc/cluster.hip).  The points are not: the reference takes ORB
corners of the rendered JPEG, which cannot be reproduced (JPEG and ORB are not bit-stable); here they are the
spectrogram cells above the colour floor ``vmin`` -- the non-background pixels of that image -- on its pixel
grid.  Counts therefore still differ from the reference's.

Out of scope: the JPEG rendering and ORB themselves.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .dsp import context, hanning_sym

C_MS_SPEC_CUT_FACTOR = 12  # prime_detection.py:22


def _freqs_times(n: int, NFFT: int, Fs: float, noverlap: int):
    """mlab._spectral_helper's frequency and time axes (onesided, even or odd pad_to = NFFT)."""
    num = NFFT // 2 + 1 if NFFT % 2 == 0 else (NFFT + 1) // 2
    freqs = np.fft.fftfreq(NFFT, 1 / Fs)[:num]
    if not NFFT % 2:
        freqs[-1] *= -1  # "get the last value correctly, it is negative otherwise"
    t = np.arange(NFFT / 2, n - NFFT / 2 + 1, NFFT - noverlap) / Fs
    return freqs, t


class SpecgramPlan:
    """mlab.specgram(x, NFFT, Fs, noverlap) for signals of one length, resident on the device."""

    def __init__(self, n: int, NFFT: int = 256, Fs: float = 2, noverlap: int = 128, dtype=np.int16,
                 device: int = 0):
        NFFT = int(NFFT)
        if NFFT < 16 or NFFT > 16384 or NFFT & (NFFT - 1):
            raise NotImplementedError("NFFT must be a power of two in [16, 16384]")
        if not 0 <= noverlap < NFFT:
            raise ValueError("noverlap must be less than NFFT")
        self.ctx = context(device)
        self.n, self.NFFT, self.Fs, self.noverlap = int(n), NFFT, float(Fs), int(noverlap)
        self.dtype = np.dtype(dtype)
        # mlab._spectral_helper: a signal shorter than NFFT is zero-padded to NFFT (one frame)
        self.n_dev = max(self.n, NFFT)
        w = hanning_sym(NFFT)                   # window_hanning(np.ones(NFFT)) = np.hanning(NFFT)
        scale = 1.0 / (Fs * (w ** 2).sum())     # result /= Fs; result /= (window**2).sum()
        self.plan = _lib.StftPlan(self.ctx, NFFT, NFFT - noverlap, w, scale, nfft=NFFT, precision=np.float64)
        self.plan.set_detrend(False)            # mlab default detrend_none
        self.K = NFFT // 2 + 1
        self.T = self.plan.frames(self.n_dev)
        self.ld = max(32, (self.T + 31) // 32 * 32)
        self.freqs, self.t = _freqs_times(self.n_dev, NFFT, Fs, noverlap)
        es = self.dtype.itemsize
        self.d_x = self.ctx.alloc((self.n_dev + 7) // 8 * 8 * es)
        self.d_x.memset(0)
        self.d_off = self.ctx.alloc(8)
        self.d_len = self.ctx.alloc(8)
        self.d_off.upload(np.zeros(1, np.int64))
        self.d_len.upload(np.array([self.n_dev], np.int64))
        self.d_spec = self.ctx.alloc(self.K * self.ld * 8)
        self.d_sum = self.ctx.alloc(8)

    def run(self, x: np.ndarray):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.shape != (self.n,):
            raise ValueError("signal length differs from the plan's")
        self.d_x.upload(x)  # the zero tail up to NFFT (short signals) was set at construction
        self.plan.run_dev(self.d_x, self.dtype, self.d_off, self.d_len, 1, self.T, self.d_spec, self.ld)

    def spectrogram(self) -> np.ndarray:
        out = np.empty((self.K, self.ld), np.float64)
        self.d_spec.download(out)
        return out[:, : self.T]

    def band_power(self, lo_hz: float, hi_hz: float) -> tuple[float, int]:
        """(np.sum(Pxx[(freqs >= lo) & (freqs <= hi)]), number of bins) on the device."""
        idx = np.nonzero((self.freqs >= lo_hz) & (self.freqs <= hi_hz))[0]
        if idx.size == 0:
            return 0.0, 0
        assert idx[-1] - idx[0] + 1 == idx.size
        _lib.check(self.ctx.lib.msd_spec_band_sum_f64_dev(self.ctx.h, self.d_spec.ptr, 1, self.K, self.T, self.ld,
                                                          int(idx[0]), int(idx[-1]), self.d_sum.ptr))
        s = np.empty(1, np.float64)
        self.d_sum.download(s)
        return float(s[0]), int(idx.size)


def specgram(x, NFFT=None, Fs=None, noverlap=None, device: int = 0):
    """matplotlib.mlab.specgram(x, NFFT, Fs, noverlap) defaults (window_hanning, detrend_none,
    one-sided psd, scale_by_freq): returns (spec float64 [NFFT//2+1, T], freqs, t)."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise NotImplementedError("only 1-D real signals are implemented")
    NFFT = 256 if NFFT is None else int(NFFT)
    Fs = 2 if Fs is None else Fs
    noverlap = 128 if noverlap is None else int(noverlap)
    dt = x.dtype if x.dtype in (np.int16, np.int32, np.uint8, np.float32, np.float64) else np.float64
    p = SpecgramPlan(len(x), NFFT, Fs, noverlap, dtype=dt, device=device)
    p.run(x.astype(dt, copy=False))
    return p.spectrogram(), p.freqs, p.t


def noise_floor(x, fs, NFFT=2048, lower_freq=250, upper_freq=800, cut_factor=C_MS_SPEC_CUT_FACTOR, device: int = 0):
    """prime_detection.py:65-91 without the figure: returns (Pxx, freqs, bins, vmin,
    power_density_db_hz) for ``plt.specgram(x, Fs=fs, NFFT=NFFT, noverlap=NFFT // 2)``."""
    x = np.asarray(x)
    dt = x.dtype if x.dtype in (np.int16, np.int32, np.uint8, np.float32, np.float64) else np.float64
    p = SpecgramPlan(len(x), NFFT, fs, NFFT // 2, dtype=dt, device=device)
    p.run(x.astype(dt, copy=False))
    band_power, nbins = p.band_power(lower_freq, upper_freq)
    delta_f = fs / NFFT
    bandwidth = nbins * delta_f
    with np.errstate(divide="ignore", invalid="ignore"):
        pddb = 10 * np.log10(band_power / bandwidth)
    factor = 40 / 23
    vmin = pddb / factor + cut_factor
    return p.spectrogram(), p.freqs, p.t, float(vmin), float(pddb)


# ------------------------------------------------------------------ §8(f) legacy drop-in shim
def detect_and_cluster_bursts_audio(segment, fs, freq_band=(950.0, 1050.0), noise_band=(650.0, 750.0),
                                    n_fft=1024, block_duration_sec=0.1, threshold_std_factor=4.0,
                                    critical_min_dur_s=0.5, device: int = 0):
    """Audio-fed stand-in for ``detect_and_cluster_bursts(image_path, ...)``
    (meteor_detect_class/detector_and_classification.py:7-91) with its return shape
    ``(bursts, unique_labels, burst_positions, critical_bursts, non_critical_bursts)``, so the
    hourly loop of prime_detection.py:208-252 runs unchanged.  Bursts are the GPU block
    detector's detections on the segment (adaptive threshold, main.py:450-522); a burst is
    critical when it lasts >= 0.5 s, the duration rule of detector_and_classification.py:50
    (``duration >= 5`` pixels ≈ 0.5 s).  The counts are not those of the reference's ORB /
    DBSCAN image clustering (a different algorithm); only the interface and the hourly CSV
    format are compatible."""
    from .dsp import process_samples
    x = np.asarray(segment)
    if x.ndim == 2:
        x = x[:, 0]  # prime_detection.py:70 uses iq_segment[:, 0]
    res = process_samples(x, fs, block_duration_sec, freq_band, noise_band, n_fft, threshold_std_factor,
                          flag_adaptive_threshold=True, device=device)
    bursts = list(res.detections)
    labels = set(range(len(bursts)))
    positions = [(d.t_start, d.t_stop) for d in bursts]
    critical = [i for i, d in enumerate(bursts) if d.dur_s >= critical_min_dur_s]
    non_critical = [i for i, d in enumerate(bursts) if d.dur_s < critical_min_dur_s]
    return bursts, labels, positions, critical, non_critical


# The reference figure's pixel grid.  prime_detection.py:67-71 takes 2048-point frames at hop 1024 of a 30 s,
# 5 kHz grab: (150000 - 2048) // 1024 + 1 = 145 frames; :101 crops to 800-1200 Hz, bins 328 .. 491 of the 5000 / 2048
# Hz grid: 164 bins; :105 saves that axes area alone (axis off, tight, no padding), and
# detector_and_classification.py:76-81 puts the ticks of the saved image at 0 .. 495 and 0 .. 365: 496 x 366 px.
SPEC_IMAGE_PX = (496, 366)
SPEC_IMAGE_CELLS = (145, 164)
SPEC_SX = SPEC_IMAGE_PX[0] / SPEC_IMAGE_CELLS[0]  # px per frame
SPEC_SY = SPEC_IMAGE_PX[1] / SPEC_IMAGE_CELLS[1]  # px per bin
SPEC_BAND_HZ = (800.0, 1200.0)                    # prime_detection.py:101


class _SpecBatch:
    """The float64 specgrams of up to ``cap`` equal-length segments, resident on the device (SpecgramPlan's
    plan over several files)."""

    def __init__(self, n: int, cap: int, NFFT: int, fs: float, dtype, device: int):
        self.one = SpecgramPlan(n, NFFT, fs, NFFT // 2, dtype=dtype, device=device)
        p = self.one
        self.ctx, self.cap = p.ctx, int(cap)
        self.stride = (p.n_dev + 7) // 8 * 8
        es = p.dtype.itemsize
        self.d_x = self.ctx.alloc(self.cap * self.stride * es)
        self.d_x.memset(0)
        self.d_off, self.d_len = self.ctx.alloc(8 * self.cap), self.ctx.alloc(8 * self.cap)
        self.d_off.upload(np.arange(self.cap, dtype=np.int64) * self.stride)
        self.d_len.upload(np.full(self.cap, p.n_dev, np.int64))
        self.d_spec = self.ctx.alloc(self.cap * p.K * p.ld * 8)
        self.d_sum = self.ctx.alloc(8 * self.cap)

    def run(self, segs):
        """specgrams of ``segs`` (<= cap arrays of the plan's length) into d_spec"""
        p = self.one
        x = np.zeros((len(segs), self.stride), p.dtype)
        for i, sgm in enumerate(segs):
            x[i, : p.n] = sgm
        self.d_x.upload(x)
        p.plan.run_dev(self.d_x, p.dtype, self.d_off, self.d_len, len(segs), p.T, self.d_spec, p.ld)

    def band_power(self, nseg: int, lo_hz: float, hi_hz: float):
        p = self.one
        idx = np.nonzero((p.freqs >= lo_hz) & (p.freqs <= hi_hz))[0]
        if idx.size == 0:
            return np.zeros(nseg), 0
        _lib.check(self.ctx.lib.msd_spec_band_sum_f64_dev(self.ctx.h, self.d_spec.ptr, nseg, p.K, p.T, p.ld,
                                                          int(idx[0]), int(idx[-1]), self.d_sum.ptr))
        s = np.empty(nseg, np.float64)
        self.d_sum.download(s)
        return s, int(idx.size)


def _mono(segment):
    x = np.asarray(segment)
    if x.ndim == 2:
        x = x[:, 0]  # prime_detection.py:70 uses iq_segment[:, 0]
    dt = x.dtype if x.dtype in (np.int16, np.int32, np.uint8, np.float32, np.float64) else np.float64
    return x.astype(dt, copy=False)


def detect_and_cluster_bursts_spec_batch(segments, fs, eps=30, min_samples=5, critical_min_extent=5.0,
                                         band_hz=SPEC_BAND_HZ, NFFT=2048, lower_freq=250, upper_freq=800,
                                         cut_factor=C_MS_SPEC_CUT_FACTOR, sx=None, sy=None, max_points=500,
                                         batch: int = 120, device: int = 0, details: bool = False):
    """``detect_and_cluster_bursts_spec`` over a list of equal-length segments (an hour is 120 grabs, a day
    2 880), ``batch`` of them per launch: one 5-tuple per segment, in order.  ``details=True`` returns
    (tuples, info) with info[i] = dict(vmin, thr, ncand, points, labels)."""
    from . import cluster
    segs = [_mono(s) for s in segments]
    if not segs:
        return ([], []) if details else []
    n, dt = len(segs[0]), segs[0].dtype
    if any(len(s) != n or s.dtype != dt for s in segs):
        raise ValueError("the segments of a batch must have one length and one dtype")
    sb = _SpecBatch(n, min(int(batch), len(segs)), NFFT, fs, dt, device)
    p, ctx = sb.one, sb.ctx
    rows = np.nonzero((p.freqs >= band_hz[0]) & (p.freqs <= band_hz[1]))[0]
    if rows.size == 0:
        raise ValueError("band_hz selects no bin")
    k_lo, k_hi = int(rows[0]), int(rows[-1])
    sx = SPEC_SX if sx is None else float(sx)
    sy = SPEC_SY if sy is None else float(sy)
    out, info = [], []
    for b0 in range(0, len(segs), sb.cap):
        part = segs[b0: b0 + sb.cap]
        nseg = len(part)
        sb.run(part)
        band_power, nbins = sb.band_power(nseg, lower_freq, upper_freq)
        with np.errstate(divide="ignore", invalid="ignore"):
            pddb = 10 * np.log10(band_power / (nbins * (fs / NFFT)))  # prime_detection.py:77-84
            vmin = pddb / (40 / 23) + cut_factor                       # :85-91
            thr = 10.0 ** (vmin / 10)  # the image shows 10 log10(Pxx) against vmin (:88, :96-97)
        bufs = cluster.peaks_dev(ctx, sb.d_spec, nseg, p.K, p.T, p.ld, k_lo, k_hi, thr, sx, sy, max_points)
        try:
            res = cluster.cluster_dev(ctx, bufs[0], bufs[2], nseg, max_points, eps, min_samples, critical_min_extent)
            pk = cluster.download_peaks(*bufs, nseg, max_points) if details else None
        finally:
            for d in bufs:
                d.free()
        for i in range(nseg):
            positions = [tuple(float(v) for v in b) for b in res.boxes[i]]
            labels = set(int(v) for v in res.labels[i])
            # (bursts, unique_labels, burst_positions, critical_bursts, non_critical_bursts), :91
            out.append((positions, labels, positions, [int(c) for c in res.critical[i]],
                        [int(c) for c in res.non_critical[i]]))
            if details:
                info.append(dict(vmin=float(vmin[i]), thr=float(thr[i]), ncand=int(pk.ncand[i]), points=pk.points[i],
                                 cells=pk.cells[i], labels=res.labels[i], k_lo=k_lo, k_hi=k_hi, frames=p.T))
    return (out, info) if details else out


def detect_and_cluster_bursts_spec(segment, fs, eps=30, min_samples=5, **kw):
    """Spectrogram-fed ``detect_and_cluster_bursts(image_path, eps=30, min_samples=5)``
    (meteor_detect_class/detector_and_classification.py:7-91) with its return shape
    ``(bursts, unique_labels, burst_positions, critical_bursts, non_critical_bursts)``: the float64 specgram
    and ``vmin`` of ``noise_floor`` (the spectrogram stays on the device) -> the cells of the 800-1200 Hz
    window above ``vmin``, at most 500 (ORB's nfeatures), on the reference image's pixel grid (``SPEC_SX``,
    ``SPEC_SY``) -> DBSCAN, boxes and the critical rule on the device.  ``burst_positions`` (and ``bursts``)
    are the clusters' boxes ``(x_min, y_min, x_max, y_max)`` in those pixels, x along time, y along
    frequency upwards from ``band_hz[0]`` (the image's rows run downwards; DBSCAN and the extent rule do not
    depend on the flip); ``unique_labels`` is ``set(labels)``, -1 included when there is noise, as :38.
    Clustering, boxes and the critical rule are the reference's; the points are above-floor cells, not ORB
    corners, so the counts still differ from the reference's."""
    r = detect_and_cluster_bursts_spec_batch([segment], fs, eps, min_samples, **kw)
    return (r[0][0], r[1][0]) if kw.get("details") else r[0]


HOURLY_COLUMNS = ("Timestamp", "Anzahl", "Kritisch")  # prime_detection.py:138


def append_hourly_row(file_name, start_time, n_critical: int, n_non_critical: int) -> None:
    """prime_detection.py:229-245: append ``start_time;total;critical`` to the day's
    ``;``-separated CSV (header ``Timestamp;Anzahl;Kritisch``, created if missing — :139-146)."""
    import os
    new = not os.path.exists(file_name)
    with open(file_name, "a", newline="") as fh:
        if new:
            fh.write(";".join(HOURLY_COLUMNS) + "\n")
        fh.write(f"{start_time.strftime('%Y-%m-%d %H:%M:%S')};{n_critical + n_non_critical};{n_critical}\n")
