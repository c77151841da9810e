"""Drop-in for the reference's phase-2 live detector, dsp/src/live/backend/processor.py
(``wav_file_process``) with the dataclasses of dsp/src/live/backend/aggregates.py.

The per-block Welch PSD band powers (a8, processor.py:206 and :349-369) and the state
machine (a9, processor.py:391-507) run on the GPU through libmsdsp
(``msd_welch_bands*``, ``msd_live_detect*``); there is no CPU fallback.  The per-meteor
waterfall export (``ConfigSpecExport.output_dir``, processor.py:295-343) draws per-block Welch
PSD rows computed on the GPU (``msd_welch_psd``: only the rows the image shows, plus the
full rows of the initialisation blocks that set its colour range).  The live UI animation
(``enable_ui_plots``, an interactive matplotlib window) is not part of the drop-in: asking for
it raises ``NotImplementedError``.

Lower-level pieces: ``welch_band_db`` (band dB rows of one signal), ``welch_spectrum`` (every block's
whole-band PSD row and its dB mean, by a pruned FFT), ``live_detect`` (the
state machine over band dB rows), ``LiveBatch`` (many recordings resident in HBM),
``LiveSession`` (the detector fed in chunks as the audio arrives, state kept on the GPU).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib, margin, wav
from .dsp import context, hann_periodic


# ------------------------------------------------------------------ aggregates.py:4-74
@dataclass
class State:
    pass


@dataclass
class StateInitialization(State):
    history_channel_dB: list = field(default_factory=list)


@dataclass
class StateDetection(State):
    locked_threshold: float = -1.0
    use_locked_threshold_until_secs: float = -1.0


@dataclass
class StateTracking(State):
    locked_threshold: float
    time_start_detection: float
    history_over_noise_sig_dB: list


@dataclass
class Config:
    pass


@dataclass
class ConfigDetection(Config):
    proc_block_sec: float = 0.2
    n_fft: int = 4096
    signal_freq: int = 1000
    channel_width: int = 100
    noise_channel_offset: int = 300
    avg_win_sec: float = 8
    init_detection_wait_sec: float = 8 * 1.0
    after_tracking_wait_sec: float = 8 * 1.5
    threshold_std_factor: float = 4
    detection_db_over_noise_mean_min: float = -1
    detection_dur_min_sec: float = -1


@dataclass
class ConfigVisualization(Config):
    enable_ui_plots: bool = True
    realtime_factor: float = 16
    flag_realtime_animation: bool = True
    max_range_sec: int = 60
    limit_freq_offset_wf2_and_export: int = 100
    wf_offset_vmin: int = 20
    wf_offset_vmax: int = 20
    enable_debug_logs: bool = False


@dataclass
class ConfigSpecExport(Config):
    output_dir: str = ""
    time_before_meteor_sec: int = 3
    time_after_meteor_sec: int = 3


@dataclass
class DetectedMeteor:
    time_start: float
    time_stop: float
    duration: float
    db_min: float
    db_max: float
    db_mean: float
    db_std: float


class LiveMeteors(list):
    """``wav_file_process``'s meteors, with the near-tie guard's verdict (margin.py, live part):
    ``near_tie`` is True when a detector decision lies within the over-noise error bound of its
    threshold (a meteor boundary may then differ from the scipy reference; otherwise none can),
    ``min_margin`` = min |db2 - thr| over the decisions, ``decision_bound`` the bound."""
    near_tie: bool = False
    min_margin: float = float("inf")
    decision_bound: float = 0.0


# ------------------------------------------------------------------ configuration
def band_edges(cfg: ConfigDetection):
    """processor.py:32-45: [start, stop] in Hz of the signal band and the two noise bands."""
    half = cfg.channel_width / 2
    ms = (cfg.signal_freq - half, cfg.signal_freq + half)
    n1 = ((cfg.signal_freq - cfg.noise_channel_offset) - half, (cfg.signal_freq - cfg.noise_channel_offset) + half)
    n2 = ((cfg.signal_freq + cfg.noise_channel_offset) - half, (cfg.signal_freq + cfg.noise_channel_offset) + half)
    return ms, n1, n2


def _mask_bins(nfft: int, fs, lo: float, hi: float) -> tuple[int, int]:
    """Inclusive bin range of (freqs >= lo) & (freqs <= hi) over scipy's welch frequencies
    (sp_fft.rfftfreq(nfft, 1/fs)); (0, -1) when empty."""
    freqs = np.fft.rfftfreq(nfft, 1 / fs)
    idx = np.nonzero((freqs >= lo) & (freqs <= hi))[0]
    if idx.size == 0:
        return 0, -1
    assert idx[-1] - idx[0] + 1 == idx.size
    return int(idx[0]), int(idx[-1])


def welch_cfg(fs, cfg: ConfigDetection, sample_scale: float = 1.0):
    """scipy.signal.welch(block, fs, nfft=n_fft) defaults (window 'hann', nperseg 256 capped at
    the block length, noverlap nperseg//2) → (msd_welch_cfg, window)."""
    bs = int(cfg.proc_block_sec * fs)
    if bs < 1:
        raise ValueError("proc_block_sec * fs must give at least one sample per block")
    nperseg = 256 if bs >= 256 else bs
    noverlap = nperseg // 2
    nfft = int(cfg.n_fft)
    if nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")  # scipy's message
    win = hann_periodic(nperseg)
    wc = win.astype(np.complex128)
    scale = np.real(1.0 / (fs * (wc * wc).sum()))  # scipy: win cast to the complex out dtype
    c = _lib.MsdWelchCfg()
    c.block_size, c.nperseg, c.noverlap, c.nfft = bs, nperseg, noverlap, nfft
    c.sample_scale = float(sample_scale)
    c.scale = float(scale)
    c.nbands = 3
    for j, (lo, hi) in enumerate(band_edges(cfg)):
        c.band_lo[j], c.band_hi[j] = _mask_bins(nfft, fs, lo, hi)
    return c, win


def live_cfg(fs, cfg: ConfigDetection) -> _lib.MsdLiveCfg:
    c = _lib.MsdLiveCfg()
    c.block_size = int(cfg.proc_block_sec * fs)
    c.avg_win_blocks = int(cfg.avg_win_sec / cfg.proc_block_sec)  # processor.py:58
    c.fs = float(fs)
    c.k_std = float(cfg.threshold_std_factor)
    c.init_wait_sec = float(cfg.init_detection_wait_sec)
    c.after_tracking_wait_sec = float(cfg.after_tracking_wait_sec)
    c.min_db_mean = float(cfg.detection_db_over_noise_mean_min)
    c.min_dur_sec = float(cfg.detection_dur_min_sec)
    return c


def _device_samples(data: np.ndarray):
    """Samples as the kernels take them + the factor that turns them into soundfile's float64
    (PCM16 / 32768, PCM32 and 24-bit-in-int32 / 2^31, 8-bit (x - 128) / 128)."""
    if data.dtype == np.int16:
        return data, 1.0 / 32768.0
    if data.dtype == np.int32:
        return data, 1.0 / 2147483648.0
    if data.dtype == np.uint8:
        return data.astype(np.int16) - 128, 1.0 / 128.0
    if data.dtype in (np.float32, np.float64):
        return data, 1.0
    raise TypeError(f"unsupported sample dtype {data.dtype}")


# ------------------------------------------------------------------ a8 / a9 entry points
def welch_band_db(x: np.ndarray, fs, config_detection: ConfigDetection, sample_scale: float = 1.0,
                  device: int = 0) -> np.ndarray:
    """Per-block (signal, noise 1, noise 2) dB, float64 [3][nb] (processor.py:206, :349-369)."""
    c, win = welch_cfg(fs, config_detection, sample_scale)
    plan = _lib.WelchPlan(context(device), c, win)
    try:
        return plan.run(np.ascontiguousarray(x))
    finally:
        plan.close()


def welch_spectrum(x: np.ndarray, fs, config_detection: ConfigDetection, sample_scale: float = 1.0, device: int = 0):
    """Per-block whole-band Welch PSD by the pruned FFT (csrc/welch_fft.hip): (psd [nb][n_fft/2 + 1],
    db_mean [nb]) -- processor.py:206's ``block_psd`` of every block and :448's
    ``np.mean(10 * np.log10(block_psd))``, float64."""
    c, win = welch_cfg(fs, config_detection, sample_scale)
    plan = _lib.WelchPlan(context(device), c, win)
    try:
        return plan.spectrum(np.ascontiguousarray(x))
    finally:
        plan.close()


def live_detect(band_db: np.ndarray, fs, config_detection: ConfigDetection, device: int = 0):
    """The state machine (processor.py:391-507): (list[DetectedMeteor], thresholds, over_noise)."""
    rows, thr, over = _lib.live_detect(context(device), band_db, live_cfg(fs, config_detection))
    mets = [DetectedMeteor(float(r["time_start"]), float(r["time_stop"]), float(r["duration"]), float(r["db_min"]),
                           float(r["db_max"]), float(r["db_mean"]), float(r["db_std"])) for r in rows]
    return mets, thr, over


def _first_decision_block(nb: int, fs, cfg: ConfigDetection) -> int:
    """the block at which Init ends (processor.py:452-455: block start >= the wait)"""
    bs = int(cfg.proc_block_sec * fs)
    for b in range(nb):
        if (b * bs) / fs >= cfg.init_detection_wait_sec:
            return b
    return nb


def near_tie_check(band_db: np.ndarray, thr: np.ndarray, over: np.ndarray, span: np.ndarray, fs,
                   cfg: ConfigDetection, what: str = "", warn: bool = True, absmax=None):
    """(near_tie, min_margin, bound) of one recording from the device's band dB rows, the
    thresholds used and the over-noise values (live_detect), and each block's sample span
    (margin.block_span); ``absmax`` (margin.block_absmax) for int16 samples, which may take the
    int8 path (csrc/welch_i8.hip); a NearTieWarning when near."""
    c, win = welch_cfg(fs, cfg)
    bands = [(int(c.band_lo[j]), int(c.band_hi[j])) for j in range(3)]
    err = margin.live_over_error(band_db, block_size=int(c.block_size), nperseg=int(c.nperseg),
                                 noverlap=int(c.noverlap), nfft=int(c.nfft), window=win, span=span, bands=bands,
                                 scale=float(c.scale), absmax=absmax)
    W = int(cfg.avg_win_sec / cfg.proc_block_sec)
    return margin.live_decision_check(over, thr, err, k_std=cfg.threshold_std_factor, W=W,
                                      first_block=_first_decision_block(len(over), fs, cfg), what=what, warn=warn)


def wav_file_process(wav_file_path: str,
                     config_detection: ConfigDetection,
                     config_visualization: ConfigVisualization,
                     config_spec_export: ConfigSpecExport,
                     wav_file_start_sec: float = 0,
                     wav_file_stop_sec: float = -1,
                     *,
                     required_sample_rate=4000,
                     device: int = 0):
    """GPU drop-in for processor.py:14-543 (same arguments, asserts and printed results).
    Returns the detected meteors as a ``LiveMeteors`` list (the reference returns None and only
    prints them) carrying the near-tie guard's verdict; a NearTieWarning when a decision lies
    within the error bound of the scipy reference."""
    assert os.path.exists(wav_file_path), f"File not found: {wav_file_path}"
    if config_spec_export.output_dir != "":
        assert os.path.exists(config_spec_export.output_dir), \
            f"Output Directory not found: {config_spec_export.output_dir}"
    if config_visualization.enable_ui_plots:
        raise NotImplementedError("the live UI animation (enable_ui_plots) is not part of the GPU drop-in; "
                                  "set enable_ui_plots=False (the spectrogram export, output_dir, is)")
    file_sample_rate, data = wav.read(wav_file_path)
    if required_sample_rate is not None:
        assert file_sample_rate == required_sample_rate, f"Invalid Sample Rate: {file_sample_rate}"
    start = int(wav_file_start_sec * file_sample_rate)
    if wav_file_stop_sec != -1:
        data = data[start:int(wav_file_stop_sec * file_sample_rate)]
    else:
        data = data[start:]
    if data.ndim > 1:
        print("WARNING: Multichannel file detected. Using first channel only.")
        data = data[:, 0]
    _print_config(config_detection, config_visualization)
    x, sample_scale = _device_samples(np.ascontiguousarray(data))
    block_size = int(config_detection.proc_block_sec * file_sample_rate)
    print()
    print("###############")
    print("Prepare Wav")
    print("###############")
    print("File Samplerate: ", file_sample_rate)
    print("File Blockgröße: ", block_size)
    print("File Dauer: ", len(x) / file_sample_rate)
    print()
    print("###############")
    print("Process Loop")
    print("###############")
    bdb = welch_band_db(x, file_sample_rate, config_detection, sample_scale, device)
    found, thr, over = live_detect(bdb, file_sample_rate, config_detection, device)
    meteors = LiveMeteors(found)
    span = margin.block_span(x, block_size, sample_scale)[: bdb.shape[1]]
    absmax = margin.block_absmax(x, block_size, sample_scale)[: bdb.shape[1]] if x.dtype == np.int16 else None
    meteors.near_tie, meteors.min_margin, meteors.decision_bound = near_tie_check(
        bdb, thr, over, span, file_sample_rate, config_detection, what=f"{wav_file_path}: ", absmax=absmax)
    for i, m in enumerate(meteors):
        print("Detected Meteor:", m, "Now Detected Meteors:", i + 1)
    not_exported = list(meteors)
    if config_spec_export.output_dir != "":
        _, not_exported = export_meteor_specs(x, sample_scale, file_sample_rate, bdb.shape[1], meteors,
                                              config_detection, config_visualization, config_spec_export, device)
    if len(not_exported) != 0:  # processor.py:539-543
        print("Detected Meteors not exported: ", len(not_exported))
        for t in not_exported:
            print(t)
    return meteors


def _print_config(cd: ConfigDetection, cv: ConfigVisualization):
    """processor.py:25-59: the band edges and window sizes it prints before processing."""
    (ms0, ms1), (n10, n11), (n20, n21) = band_edges(cd)
    print()
    print("###############")
    print("Init Config")
    print("###############")
    print("Freq MS Min: ", ms0)
    print("Freq MS Max: ", ms1)
    print("Freq Noise 1 Min: ", n10)
    print("Freq Noise 1 Max: ", n11)
    print("Freq Noise 2 Min: ", n20)
    print("Freq Noise 2 Max: ", n21)
    print("Waterfall Win Size: ", int(cv.max_range_sec / cd.proc_block_sec))
    print("Avg Win Size: ", int(cd.avg_win_sec / cd.proc_block_sec))


def block_psd_rows(x: np.ndarray, sample_scale: float, fs, cfg: ConfigDetection, b0: int, b1: int, k0: int, k1: int,
                   device: int = 0) -> np.ndarray:
    """Welch PSD of blocks [b0, b1), bins [k0, k1], float64 [b1-b0][k1-k0+1]: the rows of
    processor.py:206's ``welch(block, fs, nfft=n_fft)`` the waterfall image needs (GPU)."""
    c, win = welch_cfg(fs, cfg, sample_scale)
    c.nbands = 1
    c.band_lo[0], c.band_hi[0] = int(k0), int(k1)
    bs = int(c.block_size)
    plan = _lib.WelchPlan(context(device), c, win)
    try:
        return plan.psd(np.ascontiguousarray(x[b0 * bs: b1 * bs]), k1 - k0 + 1)
    finally:
        plan.close()


def export_meteor_specs(x: np.ndarray, sample_scale: float, fs, nb: int, meteors, cd: ConfigDetection,
                        cv: ConfigVisualization, ce: ConfigSpecExport, device: int = 0):
    """processor.py:295-343: each meteor is exported at the first block after the one that closed
    it whose waterfall window (the block-end times of the last max_range_sec / proc_block_sec
    blocks) contains [start - time_before, stop + time_after]; the image is that window's
    PSD rows in dB (imshow, colour range = the mean PSD dB of the initialisation blocks -
    wf_offset_vmin .. + wf_offset_vmax), cropped to those times and to signal_freq +-
    limit_freq_offset_wf2_and_export, saved as output_dir + spec_{start:.2f}_{stop:.2f}.jpg.
    Only the rows inside the crop (one more on each side) are computed: imshow with the
    matching sub-extent draws the same picture.  Returns (paths, meteors never exported)."""
    import matplotlib.pyplot as plt
    bs = int(cd.proc_block_sec * fs)
    W = int(cv.max_range_sec / cd.proc_block_sec)  # processor.py:57
    nfft = int(cd.n_fft)
    K = nfft // 2 + 1
    freqs = np.fft.rfftfreq(nfft, 1 / fs)
    end = lambda b: (b * bs + bs) / fs  # noqa: E731  block_end_elapsed_sec
    start_of = lambda b: (b * bs) / fs  # noqa: E731
    # the block that ends the initialisation (processor.py:452-455) and the colour range
    b_init = next((b for b in range(nb) if start_of(b) >= cd.init_detection_wait_sec), None)
    mean_init = None
    if b_init is not None:
        full = block_psd_rows(x, sample_scale, fs, cd, 0, b_init + 1, 0, K - 1, device)
        with np.errstate(divide="ignore"):
            mean_init = np.mean([np.mean(10 * np.log10(r)) for r in full])
    lo_f = cd.signal_freq - cv.limit_freq_offset_wf2_and_export
    hi_f = cd.signal_freq + cv.limit_freq_offset_wf2_and_export
    h = (freqs[-1] - freqs[0]) / K  # imshow row height of the full image
    k0 = max(0, int(np.floor((lo_f - freqs[0]) / h)) - 1)
    k1 = min(K - 1, int(np.ceil((hi_f - freqs[0]) / h)) + 1)
    ms0, ms1 = band_edges(cd)[0]
    paths, pending = [], []
    for m in meteors:
        c = int(round(m.time_stop * fs / bs))  # the block that closed the meteor
        t_sim0 = m.time_start - ce.time_before_meteor_sec
        t_sim1 = m.time_stop + ce.time_after_meteor_sec
        exp_b = None
        for b in range(c + 1, nb):
            w0 = end(max(0, b - W + 1))
            if w0 > t_sim0:
                break  # the window start only moves later
            if w0 <= t_sim0 <= end(b) and w0 <= t_sim1 <= end(b):
                exp_b = b
                break
        if exp_b is None:
            pending.append(m)
            continue
        b0 = max(0, exp_b - W + 1)
        with np.errstate(divide="ignore"):
            rows = 10 * np.log10(block_psd_rows(x, sample_scale, fs, cd, b0, exp_b + 1, k0, k1, device))
        vmin = vmax = None
        if mean_init is not None and b_init is not None and exp_b > b_init:
            vmin, vmax = mean_init - cv.wf_offset_vmin, mean_init + cv.wf_offset_vmax
        fig = plt.figure(figsize=(10, 5))
        plt.imshow(rows.T, aspect="auto", cmap="viridis", origin="lower",
                   extent=[end(b0), end(exp_b), freqs[0] + k0 * h, freqs[0] + (k1 + 1) * h], vmin=vmin, vmax=vmax)
        plt.xlim(t_sim0, t_sim1)
        plt.ylim(lo_f, hi_f)
        plt.xlabel("Time [s]")
        plt.ylabel("Frequency [Hz]")
        plt.title(f"Detection {m.time_start:.2f}-{m.time_stop:.2f}sec (d={m.duration:.2f}sec)\n"
                  + f"Min={m.db_min:.2f}dB, Max={m.db_max:.2f}dB, Mean={m.db_mean:.2f}dB, Std={m.db_std:.2f}dB")
        plt.axvline(m.time_start, color="grey", linestyle="--")
        plt.axvline(m.time_stop, color="grey", linestyle="--")
        plt.axhline(ms0, color="grey", linestyle="--")
        plt.axhline(ms1, color="grey", linestyle="--")
        path = ce.output_dir + f"spec_{m.time_start:.2f}_{m.time_stop:.2f}.jpg"
        plt.savefig(path, bbox_inches="tight", pad_inches=0)
        plt.close(fig)
        paths.append(path)
    return paths, pending


# ------------------------------------------------------------------ batch (device-resident)
class LiveBatch:
    """Many equal-format recordings resident in HBM: one Welch launch + one detector launch.

    HBM: x [nfiles][n_pad] samples, band_db [nfiles][3][ld], over / thr [nfiles][ld],
    meteors [nfiles][cap]."""

    def __init__(self, ctx: _lib.Context, nfiles: int, n_per_file: int, fs, cfg: ConfigDetection,
                 dtype=np.int16, sample_scale: float = 1.0 / 32768.0, cap: int = 1024):
        self.ctx, self.nfiles, self.n, self.fs = ctx, int(nfiles), int(n_per_file), fs
        self.dtype = np.dtype(dtype)
        wc, win = welch_cfg(fs, cfg, sample_scale)
        self.plan = _lib.WelchPlan(ctx, wc, win)
        self.lcfg = live_cfg(fs, cfg)
        self.nb = self.plan.blocks(self.n)
        self.ld = max(1, self.nb)
        self.cap = int(cap)
        es = self.dtype.itemsize
        self.n_pad = (self.n + 7) // 8 * 8
        F = self.nfiles
        self.d_x = ctx.alloc(F * self.n_pad * es)
        self.d_off = ctx.alloc(F * 8)
        self.d_len = ctx.alloc(F * 8)
        self.d_nb = ctx.alloc(F * 8)
        self.d_off.upload(np.arange(F, dtype=np.int64) * self.n_pad)
        self.d_len.upload(np.full(F, self.n, np.int64))
        self.d_nb.upload(np.full(F, self.nb, np.int64))
        self.d_band = ctx.alloc(F * 3 * self.ld * 8)
        self.d_over = ctx.alloc(F * self.ld * 8)
        self.d_thr = ctx.alloc(F * self.ld * 8)
        self.d_met = ctx.alloc(F * self.cap * _lib.METEOR_DTYPE.itemsize)
        self.d_counts = ctx.alloc(F * 8)
        self.d_status = ctx.alloc(F * 4)
        self.cfg = cfg
        self.sample_scale = float(sample_scale)
        self.span = np.zeros((F, self.nb))  # per-block sample span, for the near-tie guard
        # per-block max |x| of int16 recordings (the int8 path's error term, margin.live_over_error)
        self.absmax = np.zeros((F, self.nb)) if self.dtype == np.int16 else None
        self.near_tie = np.zeros(F, bool)
        self.min_margins = np.full(F, np.inf)
        self.decision_bounds = np.zeros(F)

    def close(self):
        """free the batch's device buffers and plan (the context stays)"""
        if getattr(self, "plan", None) is None:
            return
        self.ctx.synchronize()
        for b in (self.d_x, self.d_off, self.d_len, self.d_nb, self.d_band, self.d_over, self.d_thr, self.d_met,
                  self.d_counts, self.d_status):
            b.free()
        self.plan.close()
        self.plan = None

    def upload_file(self, i: int, x: np.ndarray):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.shape != (self.n,):
            raise ValueError("file length differs from the batch's")
        self.span[i] = margin.block_span(x, int(self.lcfg.block_size), self.sample_scale)[: self.nb]
        if self.absmax is not None:
            self.absmax[i] = margin.block_absmax(x, int(self.lcfg.block_size), self.sample_scale)[: self.nb]
        self.d_x.upload(x, byte_offset=i * self.n_pad * self.dtype.itemsize)

    def run(self):
        lib, h = self.ctx.lib, self.ctx.h
        self.plan.run_dev(self.d_x, self.dtype, self.d_off, self.d_len, self.nfiles, self.nb, self.d_band, self.ld)
        _lib.check(lib.msd_live_detect_dev(h, self.d_band.ptr, self.d_nb.ptr, self.nfiles, self.ld, self.lcfg,
                                           self.d_met.ptr, self.cap, self.d_counts.ptr, self.d_thr.ptr,
                                           self.d_over.ptr, self.d_status.ptr))

    def band_db(self) -> np.ndarray:
        out = np.empty((self.nfiles, 3, self.ld), np.float64)
        self.d_band.download(out)
        return out[:, :, : self.nb]

    def meteors(self):
        counts = np.empty(self.nfiles, np.int64)
        self.d_counts.download(counts)
        rows = np.empty((self.nfiles, self.cap), _lib.METEOR_DTYPE)
        self.d_met.download(rows)
        return [rows[i, : min(counts[i], self.cap)] for i in range(self.nfiles)], counts

    def thresholds(self) -> np.ndarray:
        out = np.empty((self.nfiles, self.ld), np.float64)
        self.d_thr.download(out)
        return out[:, : self.nb]

    def over_noise(self) -> np.ndarray:
        out = np.empty((self.nfiles, self.ld), np.float64)
        self.d_over.download(out)
        return out[:, : self.nb]

    def check_near_ties(self, warn: bool = True) -> np.ndarray:
        """The near-tie guard per recording (``near_tie_check``): sets ``near_tie``,
        ``min_margins`` and ``decision_bounds``; one NearTieWarning naming the flagged files."""
        bdb, thr, over = self.band_db(), self.thresholds(), self.over_noise()
        for i in range(self.nfiles):
            self.near_tie[i], self.min_margins[i], self.decision_bounds[i] = near_tie_check(
                bdb[i], thr[i], over[i], self.span[i], self.fs, self.cfg, warn=False,
                absmax=None if self.absmax is None else self.absmax[i])
        if warn and self.near_tie.any():
            import warnings
            idx = np.nonzero(self.near_tie)[0]
            warnings.warn(margin.NearTieWarning(
                f"{idx.size} file(s) {idx.tolist()[:10]} have a decision within the over-noise error bound of "
                f"their threshold: a meteor boundary may differ from the scipy reference"), stacklevel=2)
        return self.near_tie


# ------------------------------------------------------------------ live session (resumable)
class LiveSession:
    """The live detector fed as the audio arrives (include/msdsp.h, live session): ``nstreams``
    independent streams, each pushed in chunks of any length -- the reference station's 30 s grabs
    (meteor_detect_class/prime_detection.py:148-163), single blocks, empty pushes.  The state
    machine, the over-noise history and the samples that do not fill a block stay on the GPU
    between pushes, so the concatenated per-push results are bit-identical to ``welch_band_db``
    + ``live_detect`` over the concatenated stream: no 8 s blind spell per grab, no lock dropped
    and no meteor cut at a grab boundary.  Times are those of the stream (block b starts at
    b * block_size / fs).

    ``dtype`` / ``sample_scale``: the samples' format and the factor to soundfile's float64, as
    ``_device_samples`` gives them (uint8 audio is pushed as uint8 and shifted here, scale 1/128).
    ``max_push_sec``: the longest chunk one device push takes (longer ``push`` calls are split).
    ``hist_sec``: the over-noise history the GPU can keep per stream, 8 bytes per block per
    stream; it has to cover ``avg_win_sec`` and the longest tracking run.  None: ``avg_win_sec``
    + 15 minutes (36 KB per stream at 0.2 s blocks).  A stream that outgrows it (a continuous
    carrier; ``avg_win_sec`` so short that the window is 0 blocks = all history) gets status 4
    and is frozen until ``reset``; the other streams carry on.

    Per stream (lists indexed by stream): ``blocks``, ``status`` (0, 3 = more meteors in one push
    than the buffer holds, 4 = history overflow), ``state`` (a ``StateInitialization`` /
    ``StateDetection`` / ``StateTracking``), and the cumulative near-tie guard ``near_tie``,
    ``min_margin``, ``decision_bound`` (margin.py, live part; sample pushes only), which at the end
    of a stream equal ``wav_file_process``'s.  ``last_band_db`` / ``last_thresholds`` /
    ``last_over``: the new blocks of the last push, per stream."""

    HIST_ALLOWANCE_SEC = 900.0

    def __init__(self, fs, config_detection: ConfigDetection, nstreams: int = 1, dtype=np.int16,
                 sample_scale: float = 1.0 / 32768.0, max_push_sec: float = 60.0, hist_sec: float | None = None,
                 device: int = 0, warn: bool = True):
        self.fs, self.cfg, self.F = fs, config_detection, int(nstreams)
        self.in_dtype = np.dtype(dtype)
        self.dev_dtype = np.dtype(np.int16) if self.in_dtype == np.uint8 else self.in_dtype
        self.sample_scale = float(sample_scale)
        self.warn = warn
        self.ctx = context(device)
        self.wcfg, self.win = welch_cfg(fs, config_detection, self.sample_scale)
        self.lcfg = live_cfg(fs, config_detection)
        self.B = int(self.lcfg.block_size)
        self.W = int(self.lcfg.avg_win_blocks)
        bsec = config_detection.proc_block_sec
        self.P = max(1, int(np.ceil(max_push_sec / bsec - 1e-9)))
        if hist_sec is None:
            hist_sec = config_detection.avg_win_sec + self.HIST_ALLOWANCE_SEC
        self.H = max(self.W, int(np.ceil(hist_sec / bsec - 1e-9)))
        self.cap = self.P // 2 + 2  # a meteor takes a trigger and a closing block
        lib, C = self.ctx.lib, _lib.C
        h = C.c_void_p()
        _lib.check(lib.msd_live_session_create(self.ctx.h, C.byref(self.lcfg), C.byref(self.wcfg), _lib.ptr(self.win),
                                               self.F, self.P, self.H, _lib.dtype_code(self.dev_dtype), C.byref(h)))
        self.h = h
        F, P = self.F, self.P
        a = self.ctx.alloc
        self.d_x = a(F * P * self.B * self.dev_dtype.itemsize)
        self.d_off, self.d_len, self.d_counts, self.d_newb = a(F * 8), a(F * 8), a(F * 8), a(F * 8)
        self.d_status = a(F * 4)
        self.d_met = a(F * self.cap * _lib.METEOR_DTYPE.itemsize)
        self.d_band, self.d_thr, self.d_over = a(F * 3 * P * 8), a(F * P * 8), a(F * P * 8)
        self._first = self._first_decision_block()
        self._init_host()

    # ---- host-side bookkeeping (the near-tie guard's running values, the remainder's copy)
    def _init_host(self, stream=None):
        idx = range(self.F) if stream is None else [stream]
        if stream is None:
            self.status = [0] * self.F
            self.near_tie = [False] * self.F
            self.min_margin = [float("inf")] * self.F
            self.decision_bound = [0.0] * self.F
            self._rem = [None] * self.F
            self._blocks = [0] * self.F
            self._big = [0.0] * self.F
            self._emax = [0.0] * self.F
            self._guarded = [False] * self.F
            self.last_band_db = [np.zeros((3, 0))] * self.F
            self.last_thresholds = [np.zeros(0)] * self.F
            self.last_over = [np.zeros(0)] * self.F
        for f in idx:
            self.status[f], self.near_tie[f], self.min_margin[f], self.decision_bound[f] = 0, False, float("inf"), 0.0
            self._rem[f] = np.zeros(0, self.dev_dtype)
            self._blocks[f], self._big[f], self._emax[f], self._guarded[f] = 0, 0.0, 0.0, False
            self.last_band_db[f], self.last_thresholds[f], self.last_over[f] = np.zeros((3, 0)), np.zeros(0), np.zeros(0)

    def _first_decision_block(self) -> int:
        """the first block that can leave Init (processor.py:452-455), as ``_first_decision_block``"""
        wait = self.cfg.init_detection_wait_sec
        b = max(0, int(np.ceil(wait * self.fs / self.B)) - 2)
        while (b * self.B) / self.fs < wait:
            b += 1
        return b

    def _samples(self, x) -> np.ndarray:
        if x is None:
            return np.zeros(0, self.dev_dtype)
        x = np.ascontiguousarray(x)
        if x.ndim != 1:
            raise ValueError("a stream's samples must be 1-D")
        if x.size and x.dtype != self.in_dtype:
            raise TypeError(f"the session takes {self.in_dtype} samples, got {x.dtype}")
        if self.in_dtype == np.uint8:
            return x.astype(np.int16) - 128  # as _device_samples
        return x.astype(self.dev_dtype, copy=False)

    def _meteors(self, rows):
        return [DetectedMeteor(float(r["time_start"]), float(r["time_stop"]), float(r["duration"]),
                               float(r["db_min"]), float(r["db_max"]), float(r["db_mean"]), float(r["db_std"]))
                for r in rows]

    def _collect(self, found, bands, thrs, overs, with_band: bool, newb=None):
        """download one device push's results and add them to the per-stream accumulators (newb: the
        new blocks per stream where the caller knows them, else the device's count)"""
        F, P = self.F, self.P
        counts, stat = np.empty(F, np.int64), np.empty(F, np.int32)
        self.d_counts.download(counts)
        if newb is None:
            newb = np.empty(F, np.int64)
            self.d_newb.download(newb)
        self.d_status.download(stat)
        thr, over = np.empty((F, P)), np.empty((F, P))
        self.d_thr.download(thr)
        self.d_over.download(over)
        band = np.empty((F, 3, P))
        if with_band:
            self.d_band.download(band)
        rows = np.empty((F, self.cap), _lib.METEOR_DTYPE)
        if (counts > 0).any():
            self.d_met.download(rows)
        for f in range(F):
            n = int(newb[f])
            self.status[f] = int(stat[f])
            if int(stat[f]) == _lib.LIVE_STATUS_CAPACITY:
                raise _lib.MsdError(_lib.MSD_ERR_CAPACITY, f"live session: stream {f} closed {int(counts[f])} meteors "
                                                            f"in one push, the buffer holds {self.cap}")
            found[f].extend(self._meteors(rows[f, : min(int(counts[f]), self.cap)]))
            thrs[f].append(thr[f, :n].copy())
            overs[f].append(over[f, :n].copy())
            if with_band:
                bands[f].append(band[f, :, :n].copy())
        return newb

    def _guard(self, f: int, chunk: np.ndarray, bdb: np.ndarray, thr: np.ndarray, over: np.ndarray):
        """the near-tie guard over a push's new blocks of stream f (``chunk``: their samples, the
        carried remainder first): running min margin and maxima, the bound from the maxima so far"""
        n = bdb.shape[1]
        if n:
            c = self.wcfg
            bands = [(int(c.band_lo[j]), int(c.band_hi[j])) for j in range(3)]
            span = margin.block_span(chunk, self.B, self.sample_scale)[:n]
            absmax = margin.block_absmax(chunk, self.B, self.sample_scale)[:n] if self.dev_dtype == np.int16 else None
            err = margin.live_over_error(bdb, block_size=self.B, nperseg=int(c.nperseg), noverlap=int(c.noverlap),
                                         nfft=int(c.nfft), window=self.win, span=span, bands=bands,
                                         scale=float(c.scale), absmax=absmax)
            b0 = self._blocks[f]
            sel = slice(max(0, self._first - b0), None)
            o, t = over[sel], thr[sel]
            ok = np.isfinite(o) & np.isfinite(t)
            if ok.any():
                self.min_margin[f] = min(self.min_margin[f], float(np.min(np.abs(o[ok] - t[ok]))))
            fin = over[np.isfinite(over)]
            if fin.size:
                self._big[f] = max(self._big[f], float(np.max(np.abs(fin))))
            self._emax[f] = float(np.maximum(self._emax[f], np.max(err)))
            self._guarded[f] = True
        if self._guarded[f]:
            k = self.cfg.threshold_std_factor
            self.decision_bound[f] = (2.0 + abs(float(k))) * self._emax[f] * (1.0 + 1e-6) \
                + 8.0 * (self.W + 8) * margin.U * self._big[f]
            m = self.min_margin[f]
            near = bool(np.isfinite(m)) and m <= self.decision_bound[f]
            if near and not self.near_tie[f] and self.warn:
                import warnings
                warnings.warn(margin.NearTieWarning(
                    f"stream {f}: decision margin {m:.3e} dB is within the over-noise error bound "
                    f"{self.decision_bound[f]:.3e} dB: a meteor boundary may differ from the scipy reference"),
                    stacklevel=4)
            self.near_tie[f] = self.near_tie[f] or near

    def _finish(self, single, found, bands, thrs, overs):
        for f in range(self.F):
            self.last_thresholds[f] = np.concatenate(thrs[f]) if thrs[f] else np.zeros(0)
            self.last_over[f] = np.concatenate(overs[f]) if overs[f] else np.zeros(0)
            self.last_band_db[f] = np.concatenate(bands[f], axis=1) if bands[f] else np.zeros((3, 0))
        return found[0] if single else found

    def _streams(self, x, ndim1):
        """(single, list of per-stream inputs): one array for a one-stream session, or a sequence"""
        single = isinstance(x, np.ndarray) and x.ndim == ndim1
        xs = [x] if single else list(x)
        if len(xs) != self.F:
            raise ValueError(f"the session has {self.F} stream(s), got {len(xs)} input(s)")
        return single, xs

    # ---- pushes
    def push(self, x):
        """New samples: a 1-D array (one-stream session) or a sequence with one entry per stream
        (arrays of any lengths, empty or None for nothing new).  Returns the ``DetectedMeteor``s
        closed by this push: a list, or one list per stream."""
        lib, C = self.ctx.lib, _lib.C
        single, xs = self._streams(x, 1)
        xs = [self._samples(v) for v in xs]
        F, B, P = self.F, self.B, self.P
        found, bands, thrs, overs = ([[] for _ in range(F)] for _ in range(4))
        step = P * B
        pos = 0
        longest = max(len(v) for v in xs)
        while True:
            parts = [v[pos: pos + step] for v in xs]
            lens = np.array([len(p) for p in parts], np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            if lens.sum():
                self.d_x.upload(np.concatenate(parts))
            self.d_off.upload(offs)
            self.d_len.upload(lens)
            _lib.check(lib.msd_live_session_push_samples_dev(
                self.h, self.d_x.ptr, self.d_off.ptr, self.d_len.ptr, int(lens.max()), self.d_met.ptr, self.cap,
                self.d_counts.ptr, self.d_newb.ptr, self.d_band.ptr, self.d_thr.ptr, self.d_over.ptr, P,
                self.d_status.ptr))
            frozen = [st == _lib.LIVE_STATUS_OVERFLOW for st in self.status]
            newb = self._collect(found, bands, thrs, overs, True)
            for f in range(F):
                if frozen[f]:
                    continue  # its remainder stays as it is
                chunk = np.concatenate([self._rem[f], parts[f]])
                n = int(newb[f])
                self._guard(f, chunk, bands[f][-1], thrs[f][-1], overs[f][-1])
                self._rem[f] = chunk[n * B:]
                self._blocks[f] += n
            pos += step
            if pos >= longest:
                break
        return self._finish(single, found, bands, thrs, overs)

    def push_rows(self, band_db):
        """New band-dB rows [3][nb] (signal, noise 1, noise 2): one array, or a sequence with one
        entry per stream (None or [3][0] for nothing new).  Returns as ``push`` (no near-tie
        guard: it needs the samples)."""
        lib = self.ctx.lib
        single, xs = self._streams(band_db, 2)
        rows = []
        for v in xs:
            v = np.zeros((3, 0)) if v is None else np.ascontiguousarray(v, dtype=np.float64)
            if v.ndim != 2 or v.shape[0] != 3:
                raise ValueError("band_db must be [3][nb] (signal, noise 1, noise 2)")
            rows.append(v)
        F, P = self.F, self.P
        found, bands, thrs, overs = ([[] for _ in range(F)] for _ in range(4))
        longest = max(v.shape[1] for v in rows)
        pos = 0
        while True:
            parts = [v[:, pos: pos + P] for v in rows]
            nbs = np.array([p.shape[1] for p in parts], np.int64)
            buf = np.zeros((F, 3, P))
            for f, p in enumerate(parts):
                buf[f, :, : p.shape[1]] = p
            self.d_band.upload(buf)
            self.d_len.upload(nbs)
            _lib.check(lib.msd_live_session_push_rows_dev(self.h, self.d_band.ptr, self.d_len.ptr, int(nbs.max()), P,
                                                          self.d_met.ptr, self.cap, self.d_counts.ptr, self.d_thr.ptr,
                                                          self.d_over.ptr, self.d_status.ptr))
            frozen = np.array([st == _lib.LIVE_STATUS_OVERFLOW for st in self.status])
            newb = np.where(frozen, 0, nbs)
            self._collect(found, bands, thrs, overs, False, newb=newb)
            for f in range(F):
                bands[f].append(parts[f][:, : int(newb[f])])
            pos += P
            if pos >= longest:
                break
        return self._finish(single, found, bands, thrs, overs)

    # ---- state
    def _states(self):
        st = (_lib.MsdLiveStreamState * self.F)()
        _lib.check(self.ctx.lib.msd_live_session_state(self.h, 0, self.F, st))
        return list(st)

    @property
    def blocks(self):
        return [int(s.blocks) for s in self._states()]

    @property
    def raw_state(self):
        """the device's msd_live_stream_state per stream (state, status, blocks, trig, lock, until,
        t_start, meteors, retained, remainder)"""
        return self._states()

    @property
    def state(self):
        """per stream, the reference's state object (aggregates.py:4-24)"""
        out = []
        for f, s in enumerate(self._states()):
            if s.state == 0:
                out.append(StateInitialization())
            elif s.state == 1:
                out.append(StateDetection(float(s.lock), float(s.until)))
            else:
                h = self.history(f)
                first = int(s.blocks - s.retained)  # the global block of h[0]
                out.append(StateTracking(float(s.lock), float(s.t_start), h[int(s.trig) + 1 - first:].tolist()))
        return out

    def history(self, stream: int = 0) -> np.ndarray:
        """the over-noise values the GPU retains for a stream (those of its last ``retained`` blocks)"""
        C = _lib.C
        out = np.empty(self.H + self.P, np.float64)
        n = C.c_int64(0)
        _lib.check(self.ctx.lib.msd_live_session_history(self.h, int(stream), _lib.ptr(out), out.size, C.byref(n)))
        return out[: n.value].copy()

    def reset(self, stream: int | None = None):
        """one stream, or all: back to Init at block 0, empty history and remainder, status 0"""
        _lib.check(self.ctx.lib.msd_live_session_reset(self.h, -1 if stream is None else int(stream)))
        self._init_host(None if stream is None else int(stream))

    def close(self):
        if getattr(self, "h", None) is None:
            return
        if self.ctx.h:
            self.ctx.lib.msd_live_session_destroy(self.h)
            for b in (self.d_x, self.d_off, self.d_len, self.d_counts, self.d_newb, self.d_status, self.d_met,
                      self.d_band, self.d_thr, self.d_over):
                b.free()
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def welch_psd(x, fs, nperseg=256, noverlap=None, nfft=None, sample_scale: float = 1.0, device: int = 0):
    """scipy.signal.welch(x, fs, window='hann', nperseg, noverlap, nfft, scaling='density') over a
    whole 1-D signal on the GPU (float64 arithmetic): returns (f, Pxx[nfft//2 + 1]).  As scipy
    does, nperseg is capped at len(x)."""
    x = np.ascontiguousarray(x)
    n = x.shape[0]
    if n == 0:
        return np.empty(0), np.empty(0)
    nperseg = min(int(nperseg), n)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    nfft = nperseg if nfft is None else int(nfft)
    if nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    win = hann_periodic(nperseg)
    wc = win.astype(np.complex128)
    c = _lib.MsdWelchCfg()
    c.block_size, c.nperseg, c.noverlap, c.nfft = n, nperseg, noverlap, nfft
    c.sample_scale = float(sample_scale)
    c.scale = float(np.real(1.0 / (fs * (wc * wc).sum())))
    c.nbands = 1
    c.band_lo[0], c.band_hi[0] = 0, nfft // 2
    plan = _lib.WelchPlan(context(device), c, win)
    try:
        P = plan.psd(x if x.dtype != np.uint8 else x.astype(np.int16) - 128, nfft // 2 + 1)[0]
    finally:
        plan.close()
    return np.fft.rfftfreq(nfft, 1 / fs), P
