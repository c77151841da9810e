"""Inputs, references and bars of the I/Q spectrogram at any frame length (helper, not a test module).

``tests/iq_signals.py`` is fixed at C5's 4096 / 4096 / 1024; everything here is parametrised by
``(fs, nperseg, nfft, hop)``.  Seeded generators of the input classes, scipy's float64 reference of
them, a float32 numpy pipeline as the yardstick of "another float32 implementation", the time-domain
frame energy, and the bars the GPU modules assert -- evaluated in numpy, so that
``tests/test_iq_any_signals.py`` can show without a GPU that the references stay inside them and that
they bite.

Per-bin bar (amplitude domain, no bin excluded), chain from ``msd_cstft_chain``:

    |sqrt S - sqrt R| <= chain * u * sqrt(1.001 * sum_k R) + 3 u sqrt R,      u = 2^-24

``chain_recount`` restates the documented per-pass table of ``csrc/cstft_chain.h`` in Python.
"""
from __future__ import annotations

import functools
import math

import numpy as np

FS = 48000.0
U32 = 2.0 ** -24
FRAME_TOL = 1e-5      # per frame, max |S - R| / max |R|: the north-star tolerance
RMS_FACTOR = 4.0      # "another implementation's constant" 

# (nperseg, nfft, hop, also float32): the GPU list
SHAPES = [
    (16, 16, 4, False),        # the minimum
    (17, 32, 5, False),        # odd everything
    (32, 32, 32, True),        # no overlap
    (64, 64, 1, False),
    (128, 128, 32, False),
    (256, 256, 64, False),
    (512, 512, 128, False),
    (1024, 1024, 256, True),
    (1000, 1024, 250, True),   # zero padding
    (2048, 2048, 512, True),
    (2048, 2048, 1096, False),  # a hop that is no multiple of anything
    (4096, 4096, 1024, False),  # under OPT_GENERIC_CSTFT
    (4000, 4096, 1000, False),  # goes generic without the option
    (8192, 8192, 2048, True),   # the LDS limit
    (3, 8192, 3, False),
]
FRAMES = 24  # frames per stream of the signal classes (20-60)


def cases():
    """(nperseg, nfft, hop, kind) of every GPU case"""
    out = []
    for nperseg, nfft, hop, f32 in SHAPES:
        out.append((nperseg, nfft, hop, "int16"))
        if f32:
            out.append((nperseg, nfft, hop, "float32"))
    return out


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]}"


# ------------------------------------------------------------------------------- the chain
def chain_recount(nperseg: int, nfft: int) -> float:
    """The documented count (csrc/cstft_chain.h): 3 for detrend, window and its rounding; per pass the
    longest path -- radix 2: 1 add, radix 4: 2, radix 8: 3 adds and a twiddle multiply, radix 16: 4 adds and a
    twiddle multiply -- a twiddle multiply being 2 sqrt 2 (complex multiply with FMA) + sqrt 2 (rounded
    twiddle); one twiddle multiply between two passes; rounded up.  nfft = 2^L runs one radix-2^(L mod 4)
    pass (if L mod 4) and L // 4 radix-16 passes.  4096 / 4096 is cstft4096_kernel's 37."""
    if nperseg == 4096 and nfft == 4096:
        return 37.0
    L = nfft.bit_length() - 1
    assert nfft == 1 << L and 4 <= L <= 13
    tw = 3.0 * math.sqrt(2.0)
    first = {0: 0.0, 1: 1.0, 2: 2.0, 3: 3.0 + tw}[L % 4]
    passes = L // 4 + (1 if L % 4 else 0)
    return float(math.ceil(3.0 + first + (4.0 + tw) * (L // 4) + tw * (passes - 1)))


# ------------------------------------------------------------------------------- references
def window(nperseg: int):
    """scipy's periodic Hann as float32 (it casts the window to complex64 for complex64 input)"""
    from scipy.signal import get_window
    return get_window("hann", nperseg).astype(np.float32)


def scale_of(fs: float, nperseg: int) -> float:
    w = window(nperseg).astype(np.complex64)
    return float(np.real(1.0 / (fs * (w * w).sum())))


def n_samples(nperseg: int, hop: int, frames: int = FRAMES) -> int:
    return (frames - 1) * hop + nperseg


def frames_of(n: int, nperseg: int, hop: int) -> int:
    return (n - nperseg) // hop + 1 if n >= nperseg else 0


def reference(z, fs, nperseg, nfft, hop) -> np.ndarray:
    """scipy's float64 two-sided spectrogram of complex128 z, frame-major [T][nfft]"""
    from scipy.signal import spectrogram
    z = np.asarray(z, np.complex128)
    if len(z) < nperseg:
        return np.zeros((0, nfft))
    _, _, S = spectrogram(z, fs, "hann", nperseg, nperseg - hop, nfft, detrend="constant", return_onesided=False,
                          scaling="density", mode="psd")
    return np.ascontiguousarray(S.T)


def reference_frames(fr, fs, nperseg, nfft) -> np.ndarray:
    """the same for single frames given as rows [K][nperseg] -> [K][nfft]"""
    from scipy.signal import spectrogram
    _, _, S = spectrogram(np.asarray(fr, np.complex128), fs, "hann", nperseg, 0, nfft, detrend="constant",
                          return_onesided=False, scaling="density", mode="psd", axis=-1)
    return np.ascontiguousarray(S[..., 0])


def _frames(z, nperseg, hop):
    T = frames_of(len(z), nperseg, hop)
    idx = np.arange(T)[:, None] * hop + np.arange(nperseg)[None, :]
    return z[idx]


def yardstick(z, fs, nperseg, nfft, hop, detrend_after_padding: bool = False) -> np.ndarray:
    """a float32 numpy pipeline: float64-mean detrend, float32 window product, scipy.fft.fft on complex64,
    |X|^2 (float32) -> [T][nfft].  detrend_after_padding: the implementation slip -- the mean taken over
    the zero-padded nfft points and subtracted from all of them"""
    import scipy.fft
    fr = _frames(np.asarray(z, np.complex128), nperseg, hop)
    w = (window(nperseg).astype(np.float64) * math.sqrt(scale_of(fs, nperseg))).astype(np.float32)
    if detrend_after_padding:
        pad = np.zeros((fr.shape[0], nfft), np.complex128)
        pad[:, :nperseg] = fr
        pad -= pad.mean(axis=1, keepdims=True)
        wp = np.zeros(nfft, np.float32)
        wp[:nperseg] = w
        v = pad.astype(np.complex64) * wp
    else:
        v = (fr - fr.mean(axis=1, keepdims=True)).astype(np.complex64) * w
    X = scipy.fft.fft(v.astype(np.complex64), n=nfft, axis=1)
    assert X.dtype == np.complex64
    return (X.real * X.real + X.imag * X.imag).astype(np.float32)


def energy_ref(z, fs, nperseg, nfft, hop) -> np.ndarray:
    """each frame's total power from the time domain (Parseval): nfft sum |(z - mean) w|^2 / (fs sum w^2)"""
    fr = _frames(np.asarray(z, np.complex128), nperseg, hop)
    w = window(nperseg).astype(np.float64)
    v = (fr - fr.mean(axis=1, keepdims=True)) * w
    return nfft * (np.abs(v) ** 2).sum(axis=1) / (fs * (w * w).sum())


# ------------------------------------------------------------------------------- the bars
def frame_err(S, R) -> np.ndarray:
    """per frame max |S - R| / max |R| (0 where both vanish, inf where only R does)"""
    S, R = np.asarray(S, np.float64), np.asarray(R, np.float64)
    num, den = np.abs(S - R).max(axis=1), np.abs(R).max(axis=1)
    out = np.zeros(len(R))
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    return out


def bin_ratio(S, R, chain) -> np.ndarray:
    """|sqrt S - sqrt R| over the per-bin bound, [T][nfft]; where the bound is 0 (an exactly zero reference
    frame): 0 if S is 0 too, else inf"""
    S, R = np.asarray(S, np.float64), np.asarray(R, np.float64)
    bound = chain * U32 * np.sqrt(1.001 * R.sum(axis=1, keepdims=True)) + 3.0 * U32 * np.sqrt(R)
    err = np.abs(np.sqrt(S) - np.sqrt(R))
    out = np.zeros_like(err)
    nz = bound > 0
    out[nz] = err[nz] / bound[nz]
    out[~nz & (err > 0)] = np.inf
    return out


def amp_rms(S, R) -> np.ndarray:
    """per frame rms over the bins of |sqrt S - sqrt R|"""
    d = np.sqrt(np.asarray(S, np.float64)) - np.sqrt(np.asarray(R, np.float64))
    return np.sqrt((d * d).mean(axis=1))


def energy_ok(partials_sum, e_ref):
    """the two energy bars per frame: 1.001 sum_i etot >= S_ref and sum_i etot <= 1.001 S_ref"""
    p, e = np.asarray(partials_sum, np.float64), np.asarray(e_ref, np.float64)
    return (1.001 * p >= e) & (p <= 1.001 * e)


def model_ed(R, nfft, chain, blo, bhi, nlo, nhi):
    """the documented delta bound (csrc/stream.hip above IQ_CHAIN) from the float64 reference spectrogram
    [T][nfft]: per frame, with the frame energy S = sum_k R (x 1.001)"""
    R = np.asarray(R, np.float64)
    A = np.sqrt(R.sum(axis=1) * 1.001)
    d = chain * U32 * A + (4.0 * math.log2(nfft) + 11.0) * 2.0 ** -53 * math.sqrt(nfft) * A

    def band(lo, hi):
        n = hi - lo + 1
        if n <= 0:
            return np.zeros(len(R))
        E = R[:, np.arange(lo, hi + 1) % nfft].sum(axis=1)
        dE = 2.0 * d * np.sqrt(n * E) + 3.0 * n * d * d + (n + 4.0) * U32 * E
        den = E + 1e-12 - dE
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, 4.342944819032518 * dE / den * (1.0 + 1e-12), np.inf)

    return band(blo, bhi) + band(nlo, nhi) + 1e-12


# ------------------------------------------------------------------------------- the inputs
def _to(z, kind):
    if kind == "int16":
        return (np.clip(np.rint(z.real), -32768, 32767).astype(np.int16),
                np.clip(np.rint(z.imag), -32768, 32767).astype(np.int16))
    return z.real.astype(np.float32), z.imag.astype(np.float32)


def tone_bins(nfft):
    if nfft <= 64:
        return list(range(nfft))
    return [0, 1, 2, nfft // 4, nfft // 2 - 1, nfft // 2, nfft // 2 + 1, nfft - 2, nfft - 1]


NOISE_LIKE = ("white", "dc_noise")


def classes(kind):
    base = ["white", "tone80", "tones", "impulses", "constant", "dc_noise", "silence", "levels"]
    return base + (["f32_dc"] if kind == "float32" else [])


def signal(name, nperseg, nfft, hop, kind, frames=FRAMES):
    """(I, Q) of class `name`, seeded by the class and the shape; int16 counts (float32 keeps that scale
    unless the class says otherwise)"""
    seed = [sorted(classes("float32")).index(name), nperseg, nfft, hop, 1 if kind == "int16" else 2]
    rng = np.random.default_rng(seed)
    n = n_samples(nperseg, hop, frames)
    t = np.arange(n)
    amp = 16384.0 if kind == "int16" else 1.0
    if name == "white":        # full-scale complex noise
        z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 8000.0
    elif name == "tone80":     # a -80 dB tone beside a 30000-count carrier
        kc, kt = nfft // 8 + 1, nfft // 8 + 3
        z = 30000.0 * np.exp(2j * np.pi * kc * t / nfft) + 3.0 * np.exp(2j * np.pi * kt * t / nfft)
    elif name == "tones":      # a unit tone on each listed bin in turn, one per stretch of samples
        bins = tone_bins(nfft)
        which = np.minimum(t * len(bins) // n, len(bins) - 1)
        z = amp * np.exp(2j * np.pi * np.asarray(bins)[which] * t / nfft)
    elif name == "impulses":   # samples 0 and nperseg - 1: the later frames are silence
        z = np.zeros(n, np.complex128)
        z[0] += 20000.0 - 10000.0j
        z[nperseg - 1] += -15000.0 + 5000.0j
    elif name == "constant":
        z = np.full(n, 1234.0 - 4321.0j) if kind == "int16" else np.full(n, np.float32(0.6) + 1j * np.float32(-0.3))
    elif name == "dc_noise":   # a near-full-scale offset under 3 counts of noise
        z = (-32000.0 + 3.0 * rng.standard_normal(n)) + 1j * 32000.0
    elif name == "silence":
        z = np.zeros(n, np.complex128)
    elif name == "levels":     # the level changes by up to 1e4 every 3 hops
        lv = 10.0 ** rng.uniform(0.0, 4.0, size=n // (3 * hop) + 1)
        z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * lv[t // (3 * hop)]
    elif name == "f32_dc":     # float32 0.6 + 1e-4 randn
        assert kind == "float32"
        z = (0.6 + 1e-4 * rng.standard_normal(n)) + 1j * (0.6 + 1e-4 * rng.standard_normal(n))
    else:
        raise KeyError(name)
    return _to(z, kind)


def as_complex(i, q):
    return i.astype(np.float64) + 1j * q.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case_data(nperseg, nfft, hop, kind, name):
    """(i, q, R) of one class at one shape: the reference computed once per process"""
    i, q = signal(name, nperseg, nfft, hop, kind)
    R = reference(as_complex(i, q), FS, nperseg, nfft, hop)
    R.setflags(write=False)
    return i, q, R
