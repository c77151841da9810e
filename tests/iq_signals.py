"""Signal classes that stress the C5 I/Q certificate (helper, not a test module).

The suite's other I/Q inputs are white noise of sigma ~1000 plus in-band pings.  A norm-wise error
bound (include/msdsp.h, msd_iq_band_delta_bound_dev: the per-bin error scales with the FRAME's
energy) is exercised where the band energy is far below the frame energy, where an energy is zero
or below the 1e-12 floor, and where the delta equals its threshold.  Each class here is one such
input: seeded, fs = 192 kHz, amplitudes in int16 units; ``cn(sigma)`` is complex Gaussian noise
of total standard deviation sigma.  float32 variants keep the int16 scale unless the table says
``/32768``.

``make(name, kind)`` returns a ``Signal`` (samples, bands, whether it carries pings);
``oracle(name, kind)`` the float64 reference of it (spectrogram, delta, detections), cached per
process; ``model_ed`` evaluates the documented fp32 bound in numpy.
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass

import numpy as np

FS, N, HOP = 192000, 4096, 1024
BAND, NOISE = (950.0, 1050.0), (-3050.0, -2950.0)
KW = dict(threshold_estimation_window_sec=2, threshold_freeze_after_detection_sec=1,
          threshold_fixed_init_duration_sec=1)
U32 = 2.0 ** -24


def _chain_constant():
    """IQ_CHAIN as csrc/stream.hip defines it: the premise and the ed formula are checked with the
    constant the kernel uses, so narrowing it there fails them"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "meteor-scatter_amd", "csrc",
                       "stream.hip")
    with open(src) as f:
        m = re.search(r"constexpr double IQ_CHAIN = ([0-9.eE+-]+);", f.read())
    return float(m.group(1))


IQ_CHAIN = _chain_constant()


@dataclass
class Signal:
    name: str
    kind: str            # "int16" or "float32"
    i: np.ndarray
    q: np.ndarray
    band: tuple
    noise: tuple
    pings: bool          # built to produce detections

    @property
    def z(self):
        return self.i.astype(np.float64) + 1j * self.q.astype(np.float64)


def cn(rng, n, sigma):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (sigma / np.sqrt(2.0))


def add_pings(rng, z, amp, f0=1000.0, count=4, avoid=()):
    """`count` (3..6) tone bursts of 0.3 s at f0, none in the first second, none starting inside an
    `avoid` interval (seconds); as test_gpu_certify._iq_f32 places them, at a fixed count"""
    n = len(z)
    seconds = n / FS
    t = np.arange(n) / FS
    placed = 0
    while placed < count:
        t0 = float(rng.uniform(1.2, seconds - 0.5))
        if any(a - 0.4 <= t0 <= b + 0.1 for a, b in avoid):
            continue
        a, b = int(t0 * FS), min(n, int((t0 + 0.3) * FS))
        z[a:b] += amp * np.exp(2j * np.pi * f0 * t[a:b])
        placed += 1
    return z


def _out(z, kind, scale=1.0):
    if kind == "int16":
        return (np.clip(np.rint(z.real), -32768, 32767).astype(np.int16),
                np.clip(np.rint(z.imag), -32768, 32767).astype(np.int16))
    return (z.real * scale).astype(np.float32), (z.imag * scale).astype(np.float32)


def _n(seconds):
    return int(FS * seconds)


# ------------------------------------------------------------------------------- the classes
def white(kind, seconds=5.0, seed=101):
    rng = np.random.default_rng(seed)
    z = add_pings(rng, cn(rng, _n(seconds), 1000.0), 300.0)
    return _out(z, kind)


def carrier_far(kind, seconds=4.0, seed=102, sigma=30.0):
    """a full-scale line 39 kHz from the bands over quiet noise: band energy ~90 dB (sigma 2: ~115 dB)
    below the frame's"""
    rng = np.random.default_rng(seed)
    n = _n(seconds)
    z = 30000.0 * np.exp(2j * np.pi * 40011.0 * np.arange(n) / FS) + cn(rng, n, sigma)
    z = add_pings(rng, z, 0.3 * sigma)
    return _out(z, kind, 1.0 / 32768.0)


def carrier_far_quiet(kind, seconds=4.0, seed=103):
    return carrier_far(kind, seconds, seed, sigma=2.0)


def carrier_near(kind, seconds=4.0, seed=104):
    """an off-bin line 1 kHz above the signal band: its Hann skirts reach the band"""
    rng = np.random.default_rng(seed)
    n = _n(seconds)
    z = 20000.0 * np.exp(2j * np.pi * 2011.0 * np.arange(n) / FS) + cn(rng, n, 3.0)
    return _out(z, kind)


def lowpass(kind, seconds=4.0, seed=105):
    """loud noise through a 255-tap 500 Hz low-pass (gain 8) plus cn(1): the signal band on the
    filter's edge, the noise band in its stop band"""
    from scipy.signal import firwin, lfilter
    rng = np.random.default_rng(seed)
    n = _n(seconds)
    h = firwin(255, 500.0, fs=FS)
    z = 8.0 * lfilter(h, 1.0, cn(rng, n + 255, 20000.0))[255:] + cn(rng, n, 1.0)
    return _out(z, kind)


DROPOUT_GAP = (2.0 + 777 / FS, 2.5 + 777 / FS)  # seconds; not on a frame border


def dropout(kind, seconds=5.0, seed=106):
    """white with 0.5 s of exact zeros: frames wholly and partly inside the gap"""
    rng = np.random.default_rng(seed)
    z = add_pings(rng, cn(rng, _n(seconds), 1000.0), 300.0, avoid=(DROPOUT_GAP,))
    z[int(DROPOUT_GAP[0] * FS): int(DROPOUT_GAP[1] * FS)] = 0.0
    return _out(z, kind)


def zeros(kind, seconds=4.0, seed=0):
    n = _n(seconds)
    dt = np.int16 if kind == "int16" else np.float32
    return np.zeros(n, dt), np.zeros(n, dt)


def dc_only(kind, seconds=4.0, seed=0):
    n = _n(seconds)
    if kind == "int16":
        return np.full(n, 12345, np.int16), np.full(n, -321, np.int16)
    return np.full(n, 0.6, np.float32), np.full(n, 0.3, np.float32)


def tiny(kind, seconds=4.0, seed=109):
    rng = np.random.default_rng(seed)
    z = cn(rng, _n(seconds), 0.8)
    return _out(np.clip(np.rint(z.real), -1, 1) + 1j * np.clip(np.rint(z.imag), -1, 1), kind)


def tiny_f32(kind, seconds=4.0, seed=110):
    """every band energy below the 1e-12 floor of 10 log10(E + 1e-12)"""
    rng = np.random.default_rng(seed)
    return _out(cn(rng, _n(seconds), 1e-6), "float32")


def impulses(kind, seconds=4.0, seed=111, sigma=0.0):
    rng = np.random.default_rng(seed)
    n = _n(seconds)
    z = cn(rng, n, sigma) if sigma else np.zeros(n, np.complex128)
    z[::1000] += 32767.0 * (1 + 1j)
    return _out(z, kind)


def impulses_noise(kind, seconds=4.0, seed=112):
    return impulses(kind, seconds, seed, sigma=1.0)


def clipped(kind, seconds=4.0, seed=113):
    rng = np.random.default_rng(seed)
    return _out(cn(rng, _n(seconds), 60000.0), kind)


def step(kind, seconds=4.0, seed=114):
    """cn(3), 3000 times louder from the middle on: the last quiet frame's norm is 70 dB below its
    neighbour's, so a bound that takes a frame's norm from a group of frames is void there"""
    rng = np.random.default_rng(seed)
    n = _n(seconds)
    z = cn(rng, n, 3.0)
    z[n // 2:] *= 3000.0
    return _out(z, kind)


def dc_band_2_4(kind, seconds=4.0, seed=115):
    rng = np.random.default_rng(seed)
    n = _n(seconds)
    return _out(30000.0 * (1 - 0.5j) + cn(rng, n, 3.0), kind)


NYQ_BAND, NYQ_NOISE = (95800.0, 96000.0), (-96000.0, -95900.0)


def nyquist(kind, seconds=5.0, seed=116):
    """white, with both bands at the ends of the spectrogram row (bins 2044..2047 and -2048..-2046);
    the pings sit in that signal band (bin 2045)"""
    rng = np.random.default_rng(seed)
    z = add_pings(rng, cn(rng, _n(seconds), 1000.0), 300.0, f0=2045 * FS / N)
    return _out(z, kind)


def levels(n, kind, hop, seed, frames=3):
    """the `step` idea for the energy partials: cn(1) times a level drawn log-uniformly from
    1 .. 10^4 that changes every `frames` hops, so neighbouring frames' energies differ by orders of
    magnitude and a partial stored for the wrong frame shows"""
    rng = np.random.default_rng(seed)
    z = cn(rng, n, 1.0)
    seg = frames * hop
    lv = 10.0 ** rng.uniform(0.0, 4.0, n // seg + 1)
    z *= np.repeat(lv, seg)[:n]
    return _out(z, kind, 1.0 / 32768.0)


#        name: (generator, dtypes, band, noise, pings)
CLASSES = {
    "white": (white, ("int16", "float32"), BAND, NOISE, True),
    "carrier_far": (carrier_far, ("int16", "float32"), BAND, NOISE, True),
    "carrier_far_quiet": (carrier_far_quiet, ("int16",), BAND, NOISE, True),
    "carrier_near": (carrier_near, ("int16",), BAND, NOISE, False),
    "lowpass": (lowpass, ("int16",), BAND, NOISE, False),
    "dropout": (dropout, ("int16", "float32"), BAND, NOISE, True),
    "zeros": (zeros, ("int16", "float32"), BAND, NOISE, False),
    "dc_only": (dc_only, ("int16", "float32"), BAND, NOISE, False),
    "tiny": (tiny, ("int16",), BAND, NOISE, False),
    "tiny_f32": (tiny_f32, ("float32",), BAND, NOISE, False),
    "impulses": (impulses, ("int16",), BAND, NOISE, False),
    "impulses_noise": (impulses_noise, ("int16",), BAND, NOISE, False),
    "clipped": (clipped, ("int16",), BAND, NOISE, False),
    "step": (step, ("int16",), BAND, NOISE, False),
    "dc_band_2_4": (dc_band_2_4, ("int16",), (90.0, 190.0), NOISE, False),
    "nyquist": (nyquist, ("int16", "float32"), NYQ_BAND, NYQ_NOISE, True),
}
CASES = [(name, kind) for name, c in CLASSES.items() for kind in c[1]]
CASE_IDS = [f"{n}-{k}" for n, k in CASES]
# the fp32 bound is finite on every frame in the model (and required so of the kernel: test_gpu_certify_stress.py)
ALL_FINITE = ("white", "dropout", "tiny", "impulses", "impulses_noise", "clipped", "step", "dc_band_2_4",
              "nyquist", "zeros", "dc_only", "tiny_f32")
# ... and a few 1e-3 dB there
TIGHT = ("white", "dropout", "tiny", "impulses", "impulses_noise", "clipped", "step", "dc_band_2_4", "nyquist")


@functools.lru_cache(maxsize=None)
def make(name, kind) -> Signal:
    gen, kinds, band, noise, pings = CLASSES[name]
    assert kind in kinds, (name, kind)
    i, q = gen(kind)
    i.setflags(write=False)
    q.setflags(write=False)
    return Signal(name, kind, i, q, band, noise, pings)


@dataclass
class Oracle:
    S: np.ndarray        # float64 [N][T], scipy's spectrogram of complex128 input
    delta: np.ndarray
    band_db: np.ndarray
    noise_db: np.ndarray
    thr: np.ndarray      # adaptive thresholds per frame
    dets: list
    dets_global: list | None = None


@functools.lru_cache(maxsize=None)
def oracle(name, kind) -> Oracle:
    """the float64 reference of a class, computed once per process and left unchanged"""
    from oracle import dsp_oracle as O
    from oracle import iq_oracle as Q
    sg = make(name, kind)
    _, _, S = Q.spectrogram_iq_ref(sg.i, sg.q, FS, N, N - HOP)
    b, nz, d = Q.band_delta_iq_ref(S, FS, N, sg.band, sg.noise)
    bs = HOP / FS
    dets, thr = O.get_detections_adaptive_ref(d, 4.0, bs, KW["threshold_estimation_window_sec"], 3,
                                              KW["threshold_freeze_after_detection_sec"],
                                              KW["threshold_fixed_init_duration_sec"], None)
    for a in (S, d, b, nz):
        a.setflags(write=False)
    return Oracle(S, d, b, nz, np.asarray(thr, np.float64), dets)


def bins(band):
    """signed inclusive bin range of a band in Hz (meteorgpu.iq.iq_band_bins, restated)"""
    f = np.fft.fftfreq(N, 1 / FS)
    k = np.fft.fftfreq(N, 1.0 / N).round().astype(np.int64)
    sel = (f >= band[0]) & (f <= band[1])
    return (int(k[sel].min()), int(k[sel].max())) if sel.any() else (0, -1)


def band_rows(lo, hi):
    """row indices (FFT order) of the signed bins lo..hi, ascending signed order"""
    return np.arange(lo, hi + 1) % N


def band_db_bound(E, n, d):
    """csrc/stream.hip band_db_bound, vectorised over frames (float64)"""
    E, d = np.asarray(E, np.float64), np.asarray(d, np.float64)
    if n <= 0:
        return np.zeros_like(d)
    dE = 2.0 * d * np.sqrt(n * E) + 3.0 * n * d * d + (n + 4.0) * U32 * E
    den = E + 1e-12 - dE
    with np.errstate(divide="ignore", invalid="ignore"):
        b = 4.342944819032518 * dE / den * (1.0 + 1e-12)
    return np.where(den > 0.0, b, np.inf)


def near_dc(lo, hi):
    return hi >= lo and lo <= 1 and hi >= -1


def ed_formula(Stot, Eb, En, band_bins, noise_bins, chain=IQ_CHAIN):
    """the documented fp32 delta bound (csrc/stream.hip above IQ_CHAIN) from a frame's total power
    Stot (before the factor 1.001) and its two band energies; arrays over frames"""
    Stot = np.asarray(Stot, np.float64)
    A = np.sqrt(Stot * 1.001)
    d = chain * U32 * A + (4.0 * np.log2(N) + 11.0) * 2.0 ** -53 * np.sqrt(float(N)) * A
    b = (band_db_bound(Eb, band_bins[1] - band_bins[0] + 1, d)
         + band_db_bound(En, noise_bins[1] - noise_bins[0] + 1, d))
    if near_dc(*band_bins) or near_dc(*noise_bins):
        b = np.full_like(b, np.inf)
    b = np.where(Stot >= 0.0, b, np.inf)
    return b + 1e-12


def model_ed(S, band, noise):
    """ed_formula evaluated on a reference spectrogram S [N][T]; band, noise in Hz"""
    bb, nb = bins(band), bins(noise)
    Eb = S[band_rows(*bb)].sum(axis=0)
    En = S[band_rows(*nb)].sum(axis=0)
    return ed_formula(S.sum(axis=0), Eb, En, bb, nb)
