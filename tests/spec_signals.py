"""Inputs, references and metrics for the real-input spectrogram kernels (helper, not a test module).

The suite's older spectrogram tests measure max_k |S - R| / max_k |R| per frame (<= 1e-5) on white
noise plus a tone: every bin within 20-30 dB of the peak, so nothing below -50 dB of a frame's
strongest bin is seen.  Here: a per-bin bound in the amplitude domain, the counterpart for
stft1024_kernel, stft_psd_kernel<M> and stft_any_kernel of the model that csrc/stream.hip states
above IQ_CHAIN for cstft4096_kernel, on inputs with 80 dB of dynamic range, full-scale noise, every
bin in turn, impulses, the two undoubled bins, a large DC offset and a constant.

    |sqrt S[k,t] - sqrt R[k,t]| <= sqrt(c_k) chain u sqrt(1.001 sum_k R[k,t]) + 3 u sqrt R[k,t]
    c_k = 1 for k = 0 and k = nfft/2, else 2;  u = 2^-24 (float32 plans), 2^-53 (float64 plans)

sum_k R over the one-sided doubled spectrum is scale ||X||_2^2 over the two-sided one, so this is
|X^_k - X_k| <= chain u sum |v_n| <= chain u ||X||_2 unchanged (sum |v| <= sqrt(N) ||v||_2 and
Parseval); the second term carries |x|^2 + |y|^2, the scale and its float rounding.  No bin is left
out: the kernels claim an exact detrend at any offset.

`chain` is counted from each kernel's code by stream.hip's rules -- the longest rounding chain from a
sample to a bin: add 1; complex multiply with FMA 2 sqrt 2 (2.83); a rounded twiddle sqrt 2 (1.41)
more, 4.24 together; a multiply by an exact power of two or by -i 0; detrend, window and its rounding
3 -- and rounded up to an integer (second-order terms).  Never fitted to a measured error.

* stft_any_kernel (csrc/stft_any.hip), M = nfft / 2, L = log2 M: detrend and window 3; one radix-2
  pass when L is odd (1 add); L // 2 radix-4 passes (2 adds each, the -i free); a twiddle multiply
  in front of every pass but the first (4.24); the real split: e / o one add (the 0.5 exact), the
  post twiddle 4.24, e + W o one add (6.24).
      chain = 3 + (L & 1) + 2 (L // 2) + 4.24 (passes - 1) + 6.24
  M = 8: 16.5 -> 17;  M = 512: 35.2 -> 36;  M = 2048: 41.5 -> 42;  M = 8192: 47.7 -> 48.
* stft_psd_kernel<M> (csrc/stft.hip): L // 3 radix-8 passes, then a radix-2 or radix-4 pass for
  L % 3.  Dft<8>: first add 1, W8 as (x + y) s: an add, a multiply and s rounded (3), Dft<4> 2: 6.
      chain = 3 + 6 (L // 3) + (L % 3) + 4.24 (passes - 1) + 6.24
  M = 128: 30.7 -> 31;  M = 256: 31.7 -> 32;  M = 512: 35.7 -> 36;  M = 1024: 41.0 -> 41.
* stft1024_kernel (csrc/stft1024.hip, csrc/fft_butterfly.h after the FMA fold): x - mean 1 (float
  samples; exact for integer ones), the window 1, its product with sqrt(scale / 2) in the table 1,
  dft8_windowed's d w product 1 and FMA 1 (that is the first DFT8 stage): 5; dft8_tail: u1 1,
  u1 + u3 1, the closing FMA 1 and its rounded s 1: 4 (the even half: dft4, 2); passes 2 and 3:
  twiddle 4.24, first stage 1, tail 4; the split 6.24 (e, o without the 0.5; W o; e + t); the
  mean's fractional part on bins 0, 1: one FMA more.
      chain = 5 + 4 + 2 (4.24 + 5) + 6.24 + 1 = 34.7 -> 35.

`rms_err` is the statistical check for noise-like input: a frame's rms amplitude error over its
2-norm, to be held against the same figure of `ref32_cpu`, a float32 pipeline on the CPU with another
FFT (pocketfft in single precision), never against the kernel's own.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.fft
from scipy.signal import get_window
from scipy.signal import spectrogram as sp_spec

FS = 48000
U32, U64 = 2.0 ** -24, 2.0 ** -53
CMUL, TWID = 2.0 * math.sqrt(2.0), math.sqrt(2.0)  # complex multiply with FMA; a rounded twiddle, on top
SPLIT = 1.0 + (CMUL + TWID) + 1.0                  # the real split: e / o, the post twiddle, e + W o
RMS_FACTOR = 4.0
LD_OK = np.finfo(np.longdouble).eps <= 2.0 ** -60  # the float64 plans' reference needs a wider type
LD_REASON = "np.longdouble is no wider than 2^-60 here: no reference above float64 for the float64 plans"


def _log2(v):
    lg = int(v).bit_length() - 1
    assert 1 << lg == v, v
    return lg


def chain_any(nfft):
    """stft_any_kernel's chain (module docstring)"""
    L = _log2(nfft // 2)
    passes = (L & 1) + L // 2
    return math.ceil(3 + (L & 1) + 2 * (L // 2) + (CMUL + TWID) * (passes - 1) + SPLIT)


def chain_tiled(nfft):
    """stft_psd_kernel<nfft / 2>'s chain (module docstring)"""
    L = _log2(nfft // 2)
    passes = L // 3 + (1 if L % 3 else 0)
    return math.ceil(3 + 6 * (L // 3) + (L % 3) + (CMUL + TWID) * (passes - 1) + SPLIT)


CHAIN_STFT1024 = math.ceil(5 + 4 + 2 * ((CMUL + TWID) + 1 + 4) + SPLIT + 1)  # 35
CHAIN_TILED = {n: chain_tiled(n) for n in (256, 512, 1024, 2048)}            # 31, 32, 36, 41
CHAIN_ANY = {n: chain_any(n) for n in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)}


# --------------------------------------------------------------------------------- signals
CLASSES = ("carrier_weak", "fullscale_noise", "staircase", "impulses", "nyquist_dc", "square", "dc_quiet", "const",
           "f32_dc", "f64_dc")
NOISE_LIKE = ("carrier_weak", "fullscale_noise")


def carrier_bin(N):
    return N // 8


def weak_bin(N):
    """N/8 + N/4 + 3, or where that leaves the one-sided range (N < 32) N/8 + N/4: off the carrier's
    three bins either way"""
    k = N // 8 + N // 4 + 3
    return k if k < N // 2 else N // 8 + N // 4


def staircase_bins(N, seed=0):
    K = N // 2
    if N <= 128:
        return np.arange(K + 1)
    rng = np.random.default_rng(1000 + N + seed)
    mid = rng.choice(np.arange(6, K - 5), size=53, replace=False)
    return np.concatenate([np.arange(6), mid, np.arange(K - 5, K + 1)])


def length(N, hop, frames):
    return N + hop * (frames - 1)


@functools.lru_cache(maxsize=None)
def samples(cls, N, n):
    """class `cls` for segment length N as float64 in int16 units (f32_dc, f64_dc: in float units), n samples
    (staircase and impulses have their own length); read-only"""
    rng = np.random.default_rng([CLASSES.index(cls), N, n])
    i = np.arange(n, dtype=np.float64)
    if cls == "carrier_weak":
        x = 30000.0 * np.cos(2 * np.pi * carrier_bin(N) * i / N) + 3.0 * np.cos(2 * np.pi * weak_bin(N) * i / N)
        x = np.round(x + rng.uniform(-0.5, 0.5, n))
    elif cls == "fullscale_noise":
        x = rng.integers(-32768, 32768, n).astype(np.float64)
    elif cls == "staircase":
        bins = staircase_bins(N)
        m = np.arange(N, dtype=np.float64)
        x = np.concatenate([np.round(8000.0 * np.cos(2 * np.pi * k * m / N + rng.uniform(0, 2 * np.pi)))
                            for k in bins])
    elif cls == "impulses":
        x = np.zeros(6 * N)
        pos = rng.choice(6 * N, size=24, replace=False)
        x[pos[:12]] = 32767.0
        x[pos[12:]] = -32768.0
    elif cls == "nyquist_dc":
        x = 20000.0 * (1.0 - 2.0 * (np.arange(n) & 1)) + 5000.0
    elif cls == "square":
        x = np.where((np.arange(n) % 14) < 7, 32767.0, -32768.0)
    elif cls == "dc_quiet":
        x = np.round(-32000.0 + 3.0 * rng.standard_normal(n))
    elif cls == "const":
        x = np.full(n, -32768.0)
    elif cls in ("f32_dc", "f64_dc"):
        x = 0.6 + 1e-4 * rng.standard_normal(n)
    else:
        raise KeyError(cls)
    x.setflags(write=False)
    return x


def cast(x, dtype, cls=None):
    """as the suite's other tests cast int16-unit samples; f32_dc and f64_dc are float already (the
    other classes' float samples are int16 / 32768: their sums are exact in any float arithmetic, these
    classes' are not)"""
    dt = np.dtype(dtype)
    if cls in ("f32_dc", "f64_dc"):
        assert dt == (np.float32 if cls == "f32_dc" else np.float64)
        return x.astype(dt)
    if dt == np.int16:
        return x.astype(np.int16)
    if dt == np.float32:
        return (x / 32768.0).astype(np.float32)
    if dt == np.uint8:
        return ((x.astype(np.int32) >> 8) + 128).astype(np.uint8)
    if dt == np.int32:
        return x.astype(np.int32) << 8
    if dt == np.float64:
        return x / 32768.0
    raise TypeError(dt)


def signal(cls, N, hop, frames, dtype):
    """the cast samples of a class: `frames` frames at (N, hop), or the class's own length"""
    return cast(samples(cls, N, length(N, hop, frames)), dtype, cls)


# ------------------------------------------------------------------------------ references
def _frames(x, N, hop):
    T = (len(x) - N) // hop + 1
    return np.lib.stride_tricks.sliding_window_view(x, N)[::hop][:T]


def ref64(x, fs, nperseg, noverlap, nfft):
    """scipy's spectrogram of the samples in float64: the truth for float32 plans"""
    return sp_spec(np.asarray(x).astype(np.float64), fs=fs, window="hann", nperseg=nperseg, noverlap=noverlap,
                   nfft=nfft, scaling="density", mode="psd")[2]


def ref32_cpu(x, fs, nperseg, noverlap, nfft):
    """a float32 pipeline on the CPU with another FFT: frames, detrend in float64 rounded to float32,
    the float32 Hann, scipy.fft.rfft in single precision, |X|^2 scale in float32 with the interior
    bins doubled.  The yardstick of the statistical check, never the truth."""
    fr = _frames(np.asarray(x).astype(np.float64), nperseg, nperseg - noverlap)
    w = get_window("hann", nperseg).astype(np.float32)
    v = (fr - fr.mean(axis=1, keepdims=True)).astype(np.float32) * w
    X = scipy.fft.rfft(v, n=nfft, axis=1)
    assert X.dtype == np.complex64, X.dtype
    scale = np.float32(1.0 / (fs * float((w.astype(np.float64) ** 2).sum())))
    P = (X.real * X.real + X.imag * X.imag) * scale
    P[:, 1:nfft // 2] *= np.float32(2.0)
    assert P.dtype == np.float32
    return np.ascontiguousarray(P.T)


def ref_ld(x, fs, nperseg, noverlap, nfft):
    """the same explicit pipeline in np.longdouble with the float64 window values: the truth for
    float64 plans (needs LD_OK)"""
    ld = np.longdouble
    fr = _frames(np.asarray(x).astype(ld), nperseg, nperseg - noverlap)
    w = get_window("hann", nperseg).astype(np.float64).astype(ld)
    v = (fr - fr.sum(axis=1, keepdims=True) / ld(nperseg)) * w
    X = scipy.fft.rfft(v, n=nfft, axis=1)
    assert X.dtype == np.result_type(ld, np.complex64), X.dtype
    P = (X.real * X.real + X.imag * X.imag) * (ld(1.0) / (ld(fs) * (w * w).sum()))
    P[:, 1:nfft // 2] *= ld(2.0)
    return np.ascontiguousarray(P.T)


# --------------------------------------------------------------------------------- metrics
def _wide(S, R):
    t = np.longdouble if np.asarray(R).dtype == np.longdouble else np.float64
    return np.asarray(S).astype(t), np.asarray(R).astype(t)


def bound_ratio(S, R, chain, u):
    """the largest ratio, over every bin of every frame, of |sqrt S - sqrt R| to the per-bin bound
    (module docstring); S, R [nfft/2 + 1][T].  A frame whose reference is all zero must be all zero:
    +inf otherwise.  Returns (ratio, (bin, frame))."""
    S, R = _wide(S, R)
    assert S.shape == R.shape and S.ndim == 2
    if not (np.all(np.isfinite(S)) and np.all(S >= 0)):
        return np.inf, (0, 0)
    K = R.shape[0]
    ck = np.full((K, 1), 2.0, R.dtype)
    ck[0] = ck[K - 1] = 1.0
    rhs = np.sqrt(ck) * (chain * u) * np.sqrt(R.dtype.type(1.001) * R.sum(axis=0))[None, :] + 3 * u * np.sqrt(R)
    lhs = np.abs(np.sqrt(S) - np.sqrt(R))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(rhs > 0, lhs / rhs, np.where(lhs > 0, np.inf, 0.0))
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), (int(at[0]), int(at[1]))


def rms_err(S, R):
    """per frame: sqrt(mean_k (sqrt S - sqrt R)^2) / sqrt(sum_k R); 0 for a frame without power"""
    S, R = _wide(S, R)
    tot = R.sum(axis=0)
    e = np.sqrt(np.mean((np.sqrt(S) - np.sqrt(R)) ** 2, axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot > 0, e / np.sqrt(tot), 0.0).astype(np.float64)


def normwise(S, R):
    """the older bar: max_k |S - R| / max_k |R| per frame, maximised over frames"""
    S, R = _wide(S, R)
    return float((np.abs(S - R).max(axis=0) / np.maximum(np.abs(R).max(axis=0), 1e-300)).max())
