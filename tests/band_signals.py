"""Inputs, references, yardsticks and chains for the float64 band-power kernels (helper, not a test
module): block_delta2_kernel and block_delta_kernel (csrc/block_delta.hip) and welch_bands_kernel
(csrc/live.hip).

The older GPU tests hold these kernels to a flat 1e-9 dB of numpy's pocketfft on noise plus a tone
near 1 kHz: bin angles around pi/3 ... pi/2, where a Goertzel recurrence is at its best.  Here every
block and band is held to meteorgpu/margin.py's own per-bin error model

    |X^_k - X_k| <= chain u S,   S = sum_j |x_j w_j| of that block,   u = 2^-53

against an exact (long double, exactly reduced angles) DFT, at the bins where the model grows as
L_seg^2 (0, 1, K-2, K-1), and -- because the model is 10-100 times loose -- to RMS_FACTOR times the
error of a textbook float64 CPU yardstick with the kernel's segmentation on noise-like input.

Chains (the longest chain of roundings from a sample to a bin, in units of u S):

* block_delta2_kernel: margin._goertzel_chain(SPL, bins, nfft), 3 SPL G + 24, with SPL the lane's
  segment (16 ... 256 by L, msd_block_plan_create), not ceil(L / 16): a lane runs all SPL steps.
* welch_bands_kernel: margin._goertzel_chain(nperseg, bin, nfft) + 2: the detrend's subtraction and
  the window product (the sample scale is a power of two here, the PSD scale and the doubling act on
  the result and sit in the 4 u sqrt P term).  The mean itself is not exact: numpy's pairwise sum
  (8 interleaved partials over a 128-leaf: 16 adds, 3 to combine, one level per doubling above 128,
  the remainder) and the division, MEAN_CHAIN(n) u mean|x|; a mean off by d moves bin k by
  d |W_k|, W the window's transform, so that term is  MEAN_CHAIN u mean|x| |W_k|.
* block_delta_kernel (by the rules of tests/spec_signals.py: add 1, complex multiply 2.83, rounded
  twiddle 1.41): the window product 1; the lane's start twiddle from the table 1.41; SPL - 1 rotation
  steps by the rounded step, 4.24 each; v c 1; the lane's running sum, SPL adds; the wave sum, 6 adds;
  hypot and its square 3 (of |X| <= S):
      chain = 1 + 1.41 + 4.24 (SPL - 1) + 1 + SPL + 6 + 3,   SPL = 8, 16, 32, 64 by L
  SPL 8: 50.1 -> 51;  16: 92.0 -> 93;  32: 175.9 -> 176;  64: 343.6 -> 344.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from meteorgpu import margin as M
from spec_signals import CMUL, LD_OK, LD_REASON, RMS_FACTOR, TWID  # noqa: F401  (re-exported)

LD = np.longdouble
PI_LD = np.longdouble("3.14159265358979323846264338327950288")  # np.pi is the float64 value
U = 2.0 ** -53
FS = 4000.0
I16, F32, U8, I32, F64 = np.int16, np.float32, np.uint8, np.int32, np.float64
ALL_DTYPES = (I16, F32, U8, I32, F64)
NBLK = 33


# ------------------------------------------------------------------------------ kernel shapes
def spl_of(L):
    """block_delta2_kernel's samples per lane (msd_block_plan_create)"""
    return 16 if L <= 256 else 32 if L <= 512 else 64 if L <= 1024 else 128 if L <= 2048 else 256


def generic_spl(L):
    """block_delta_kernel's samples per lane (launch_bd_t)"""
    return 8 if L <= 512 else 16 if L <= 1024 else 32 if L <= 2048 else 64


def chain_goertzel16(L, bins, nfft):
    return M._goertzel_chain(spl_of(L), bins, nfft)


def chain_generic(L):
    """block_delta_kernel's chain (module docstring)"""
    spl = generic_spl(L)
    return math.ceil(1 + TWID + (CMUL + TWID) * (spl - 1) + 1 + spl + 6 + 3)


def mean_chain(n):
    """roundings of np.mean over n samples, relative to mean |x| (module docstring)"""
    return 16 + 3 + max(0, math.ceil(math.log2(max(1.0, n / 128.0)))) + 1 + 1


def block_window(B, L, rect=False):
    return np.ones(L) if rect else np.hanning(B)[:L]


# ------------------------------------------------------------------------------ exact DFT
@functools.lru_cache(maxsize=8)
def _trig_ld(nfft):
    a = 2 * PI_LD * np.arange(nfft, dtype=LD) / LD(nfft)
    return np.cos(a), np.sin(a)


def dft_ld(v, bins, nfft):
    """sum_n v[:, n] e^{-2 pi i k n / nfft} for k in bins, in long double with the angle reduced
    exactly (2 pi ((k n) mod nfft) / nfft); v [rows][L] long double -> (re, im) [rows][len(bins)]"""
    c, s = _trig_ld(int(nfft))
    L = v.shape[1]
    idx = (np.asarray(bins, np.int64)[None, :] * np.arange(L, dtype=np.int64)[:, None]) % int(nfft)
    return v @ c[idx], -(v @ s[idx])


def _blocks(x, B, L):
    nb = len(x) // B
    return np.asarray(x)[: nb * B].reshape(nb, B)[:, :L]


def block_powers_ld(x, B, nfft, w, bins):
    """|X_k|^2 of every block at `bins`, long double [blocks][bins]; w: the L window values used"""
    L = min(B, nfft)
    v = _blocks(x, B, L).astype(LD) * np.asarray(w, np.float64).astype(LD)
    if len(bins) == 0:
        return np.zeros((v.shape[0], 0), LD)
    re, im = dft_ld(v, bins, nfft)
    return re * re + im * im


def band_energy(P):
    """E = sum_k |X_k|^2 + 1e-12 per block (any float type)"""
    return P.sum(axis=1) + P.dtype.type(1e-12)


def db(E):
    return (10 * np.log10(E)).astype(np.float64)


def block_S(x, B, nfft, w):
    """S = sum_j |x_j w_j| of every block"""
    L = min(B, nfft)
    return np.abs(_blocks(x, B, L).astype(np.float64) * w).sum(axis=1)


def block_powers_numpy(x, B, nfft, w, bins):
    """the reference's own numbers: |rfft(block * window, nfft)|^2 at `bins` (pocketfft, float64)"""
    L = min(B, nfft)
    X = np.fft.rfft(_blocks(x, B, L).astype(np.float64) * w, n=nfft, axis=1)
    return np.abs(X[:, list(bins)]) ** 2


# ------------------------------------------------------------------------------ yardsticks
def _goertzel(v, c2, axis_len):
    """s_m = v_m + 2 cos(th) s_{m-1} - s_{m-2} over the last-but-one axis of v [..., m, 1] against
    c2 [bins]; returns (s_{N-1}, s_{N-2})"""
    s1 = np.zeros(v.shape[:-2] + c2.shape)
    s2 = np.zeros_like(s1)
    for m in range(axis_len):
        s0 = v[..., m, :] + c2 * s1 - s2
        s2, s1 = s1, s0
    return s1, s2


def round_twiddle(c, how):
    """c rounded to a float type, or (how an int) to a mantissa `how` bits shorter than float64's"""
    if isinstance(how, int):
        m, e = np.frexp(c)
        return np.ldexp(np.rint(np.ldexp(m, 53 - how)), e - (53 - how))
    return np.asarray(c).astype(how).astype(np.float64)


def goertzel16_powers(x, B, nfft, w, bins, twiddle=np.float64, drop_segment=None, shift=0, leak=False):
    """textbook float64 Goertzel with block_delta2_kernel's segmentation: 16 segments of spl samples,
    y = s_{N-1} - e^{-i th} s_{N-2} = sum_m v_m e^{i th (N-1-m)}, rotated by e^{-i th (n0 + N - 1)} to
    the block origin, the 16 summed.  |X_k|^2 [blocks][bins] float64.
    The keyword arguments corrupt it on purpose (tests/test_band_signals.py, the teeth): `twiddle`
    rounds 2 cos th to that type, `drop_segment` zeroes one 16-sample stretch, `shift` reads the
    samples one later, `leak` lets sample L in (with the last window value)."""
    L = min(B, nfft)
    spl = spl_of(L)
    nb = len(x) // B
    xs = np.asarray(x)[shift: shift + nb * B] if shift else np.asarray(x)[: nb * B]
    nb = len(xs) // B
    v = np.zeros((nb, 16 * spl))
    v[:, :L] = xs[: nb * B].reshape(nb, B)[:, :L].astype(np.float64) * w
    if leak and B > L:  # one sample too many on the last lane: x_L w_{L-1} lands on the last position
        v[:, L - 1] += xs[: nb * B].reshape(nb, B)[:, L].astype(np.float64) * w[-1]
    if drop_segment is not None:
        v[:, 16 * drop_segment: 16 * drop_segment + 16] = 0.0
    k = np.asarray(bins, np.int64)
    th = 2.0 * np.pi * (k % nfft).astype(np.float64) / float(nfft)
    c2 = round_twiddle(2.0 * np.cos(th), twiddle)
    s1, s2 = _goertzel(v.reshape(nb, 16, spl, 1), c2, spl)
    y = (s1 - np.cos(th) * s2) + 1j * (np.sin(th) * s2)
    seg = np.arange(16, dtype=np.int64)[:, None]
    a = -2.0 * np.pi * ((k[None, :] * (seg * spl + spl - 1)) % nfft).astype(np.float64) / float(nfft)
    X = (y * (np.cos(a) + 1j * np.sin(a))).sum(axis=1)
    return X.real ** 2 + X.imag ** 2


def rotation_powers(x, B, nfft, w, bins):
    """float64 direct rotation recurrence with block_delta_kernel's segmentation: 64 lanes of SPL
    samples, the lane's twiddle stepped by e^{-i th} from its start value, lanes summed"""
    L = min(B, nfft)
    spl = generic_spl(L)
    nb = len(x) // B
    v = np.zeros((nb, 64 * spl))
    v[:, :L] = _blocks(x, B, L).astype(np.float64) * w
    v = v.reshape(nb, 64, spl, 1)
    k = np.asarray(bins, np.int64)
    n0 = (np.arange(64, dtype=np.int64) * spl)[:, None]
    a0 = -2.0 * np.pi * ((k[None, :] * n0) % nfft).astype(np.float64) / float(nfft)
    a1 = -2.0 * np.pi * (k % nfft).astype(np.float64) / float(nfft)
    c = np.cos(a0) + 1j * np.sin(a0)
    st = np.cos(a1) + 1j * np.sin(a1)
    acc = np.zeros((nb, 64, len(k)), np.complex128)
    for q in range(spl):
        acc = acc + v[:, :, q, :] * c
        c = c * st
    X = acc.sum(axis=1)
    return np.abs(X) ** 2


# ------------------------------------------------------------------------------ block signals
BLOCK_CLASSES = ("fullscale_noise", "dc_quiet", "staircase", "carrier_weak", "alternating", "edge_impulses", "zeros",
                 "tiny")
NOISE_LIKE = ("fullscale_noise", "dc_quiet")


def off_band_bin(bins, K):
    """the middle of the widest run of bins that no band uses (the carrier's place); K // 2 if none"""
    used = np.zeros(K + 2, bool)
    used[0] = used[K + 1] = True
    used[np.asarray(bins, np.int64) + 1] = True
    at = np.flatnonzero(used)
    gap = np.diff(at)
    i = int(np.argmax(gap))
    return K // 2 if gap[i] < 2 else int(at[i] + gap[i] // 2) - 1


def cast(x, dtype):
    """int16-unit samples as the dtype: int32 up to +-2^31, uint8 raw, floats / 32768"""
    dt = np.dtype(dtype)
    if dt == np.int16:
        return x.astype(np.int16)
    if dt == np.int32:
        return (x.astype(np.int64) << 16).astype(np.int32)
    if dt == np.uint8:
        return ((x.astype(np.int32) >> 8) + 128).astype(np.uint8)
    return (x / 32768.0).astype(dt)


def class_samples(cls, n, dtype, *, N, nfft, bins, B=None, L=None, seed=0, floor=False):
    """`n` samples of a class as `dtype`.  N: the block (segment) length whose multiples the class is
    laid out on; bins: the plan's bins (staircase, carrier_weak); B, L: block size and used length
    (edge_impulses); floor: edge_impulses over 1 LSB of noise (Welch: a lone sample at index 0 of a
    periodic Hann segment leaves nothing but the detrend's constant, and no bin off DC has power)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng([BLOCK_CLASSES.index(cls) if cls in BLOCK_CLASSES else 99, N, nfft, n, seed])
    i = np.arange(n, dtype=np.float64)
    K = nfft // 2 + 1
    bins = np.asarray(bins, np.int64)
    if cls == "fullscale_noise":
        x = rng.integers(-32768, 32768, n).astype(np.float64)
    elif cls == "dc_quiet":
        if dt.kind == "f":  # 0.92 plus 1e-4 of noise: sums that are not exact
            return (0.92 + 1e-4 * rng.standard_normal(n)).astype(dt)
        if dt == np.uint8:  # raw: 3 LSB of its own
            return np.clip(np.round(235.0 + 3.0 * rng.standard_normal(n)), 0, 255).astype(np.uint8)
        x = np.round(0.92 * 32767.0 + 3.0 * rng.standard_normal(n))
    elif cls == "staircase":  # block b: only a tone on plan bin b mod nbins
        b = (np.arange(n) // N).astype(np.int64)
        k = bins[b % len(bins)].astype(np.float64)
        ph = rng.uniform(0, 2 * np.pi, n // N + 1)[b]
        x = np.round(8000.0 * np.cos(2 * np.pi * k * (i % N) / nfft + ph) + rng.uniform(-0.5, 0.5, n))
    elif cls == "carrier_weak":  # a full-scale carrier off the bands, a -80 dB tone on the first band bin
        kc, kw = off_band_bin(bins, K - 1), int(bins[0])
        x = 30000.0 * np.cos(2 * np.pi * kc * i / nfft) + 3.0 * np.cos(2 * np.pi * kw * i / nfft + 1.0)
        x = np.round(x + rng.uniform(-0.5, 0.5, n))
    elif cls == "alternating":  # +- full scale, less 0-3 LSB so that no bin is exactly empty
        x = (1.0 - 2.0 * (np.arange(n) & 1)) * (32767.0 - rng.integers(0, 4, n))
    elif cls == "edge_impulses":  # one sample per block: at 0, L - 1, 1, L - 2, L (outside: contributes nothing)
        # 1 and L - 2 alongside: a symmetric Hann of B == L is 0 at both ends
        pos = [0, L - 1, 1, L - 2] + ([L] if B > L else [])
        x = rng.integers(-1, 2, n).astype(np.float64) if floor else np.zeros(n)
        for b in range(n // B):
            x[b * B + pos[b % len(pos)]] = 32767.0 if (b // len(pos)) % 2 == 0 else -32768.0
        if dt == np.uint8:  # raw: silence is 0, not the 128 of a cast
            return np.where(np.abs(x) > 1, 255, x + 1 if floor else 0).astype(np.uint8)
    elif cls == "zeros":
        return np.zeros(n, dt)
    elif cls == "tiny":  # E far below the 1e-12 floor
        assert dt == np.float64
        return 1e-8 * rng.standard_normal(n)
    elif cls == "ramp":
        x = np.round(-32768.0 + 65535.0 * (i % N) / max(1, N - 1))
    elif cls == "tone7":  # a tone on bin 7 of nfft
        x = np.round(20000.0 * np.cos(2 * np.pi * 7.0 * i / nfft + 0.3))
    elif cls == "constant":
        x = np.full(n, 12345.0)
    else:
        raise KeyError(cls)
    return cast(x, dt)


# ------------------------------------------------------------------------------ block cases
# (B, nfft, all five dtypes: the first row of its SPL)
BLOCK_SHAPES = [
    (16, 16, True), (5, 16, False),            # SPL 16: one sample per lane; empty lanes
    (256, 256, False),                         # full lanes
    (300, 1024, True),                         # SPL 32: zero padding, ragged last lane
    (9600, 1024, True),                        # SPL 64: crop; the window is the foot of hanning(9600)
    (1201, 1024, False),                       # odd B: every later block misaligned
    (2000, 2048, True),                        # SPL 128
    (4096, 4096, True), (4096, 16384, False),  # SPL 256: G = 256; nfft >> L
    (700, 600, False), (700, 601, False),      # non-power-of-two and odd nfft
]
COUNT_SHAPES = [(9600, 1024), (300, 1024)]
COUNTS_FAST = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 63, 64)
COUNTS_GENERIC = (65, 300)
COUNT_CLASSES = ("staircase", "fullscale_noise", "carrier_weak")


def edge_bins(nfft):
    K = nfft // 2 + 1
    return [0, 1, 2, (nfft + 2) // 4, K - 2, K - 1]


def split_count(n, nfft):
    """n bins as a band from DC up and a noise band down from K - 1"""
    K = nfft // 2 + 1
    nb = (n + 1) // 2
    nn = n - nb
    return (0, nb - 1), ((K - nn, K - 1) if nn else (0, -1))


def plan_bins(band, noise):
    return list(range(band[0], band[1] + 1)) + list(range(noise[0], noise[1] + 1))


def block_cases():
    """(kernel, B, nfft, dtype, rect, band, noise, generic option, classes)"""
    out = []
    for B, nfft, first in BLOCK_SHAPES:
        e = edge_bins(nfft)
        dts = ALL_DTYPES if first else (I16, F32)
        pairs = [((e[0],) * 2, (e[1],) * 2), ((e[2],) * 2, (e[3],) * 2), ((e[4],) * 2, (e[5],) * 2),
                 ((e[3],) * 2, (0, -1))]  # the last: an empty noise band
        for dt in dts:
            cls = tuple(c for c in BLOCK_CLASSES if c != "tiny" or dt == F64)
            out += [("bd2", B, nfft, dt, False, bd, nz, False, cls) for bd, nz in pairs]
        if first:  # one rectangular-window plan per SPL beside Hann
            for dt in (I16, F32):
                cls = tuple(c for c in BLOCK_CLASSES if c != "tiny")
                out.append(("bd2", B, nfft, dt, True, (e[1],) * 2, (e[4],) * 2, False, cls))
    for B, nfft in COUNT_SHAPES:
        for dt in (I16, F32):
            for n in COUNTS_FAST:
                out.append(("bd2", B, nfft, dt, False, *split_count(n, nfft), False, COUNT_CLASSES))
            for n in COUNTS_GENERIC:
                out.append(("bd", B, nfft, dt, False, *split_count(n, nfft), False, COUNT_CLASSES))
            for n in (2, 9):
                out.append(("bd", B, nfft, dt, False, *split_count(n, nfft), True, COUNT_CLASSES))
    return out


def block_case_id(c):
    kernel, B, nfft, dt, rect, band, noise, generic, _ = c
    return (f"{kernel}{'-opt' if generic else ''}-{B}-{nfft}-{np.dtype(dt).name}-{'rect' if rect else 'hann'}-"
            f"{band[0]}_{band[1]}-{noise[0]}_{noise[1]}")


@functools.lru_cache(maxsize=None)
def block_input(cls, B, nfft, dtname, bins, nblk=NBLK):
    x = class_samples(cls, nblk * B, np.dtype(dtname), N=B, nfft=nfft, bins=bins, B=B, L=min(B, nfft))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def block_refs(cls, kernel, B, nfft, dtname, rect, band, noise, nblk=NBLK):
    """of one case and class, computed once and read-only: the samples, S per block, and per band
    (band, noise) the exact dB and energy, the yardstick's energy, numpy's dB and the device chain"""
    bins = tuple(plan_bins(band, noise))
    x = block_input(cls, B, nfft, dtname, bins, nblk)
    L = min(B, nfft)
    w = block_window(B, L, rect)
    S = block_S(x, B, nfft, w)
    P = block_powers_ld(x, B, nfft, w, bins)
    Y = (goertzel16_powers if kernel == "bd2" else rotation_powers)(x, B, nfft, w, bins) if bins else \
        np.zeros((len(S), 0))
    N = block_powers_numpy(x, B, nfft, w, bins) if bins else np.zeros((len(S), 0))
    chain = (chain_goertzel16(L, bins, nfft) if kernel == "bd2" else chain_generic(L)) if bins else 0.0
    nband = max(0, band[1] - band[0] + 1)
    per = []
    for sl in (slice(0, nband), slice(nband, None)):
        E = band_energy(P[:, sl])
        per.append(dict(n=P[:, sl].shape[1], E=E, db=db(E), Ey=band_energy(Y[:, sl]), db_np=db(band_energy(N[:, sl]))))
    out = dict(x=x, S=S, w=w, chain=chain, bands=per)
    for a in (S, w):
        a.setflags(write=False)
    return out


def model_bound(ref_db, n, chain, S):
    """assertion 1's right-hand side: margin.band_db_error with the device-only chain"""
    return M.band_db_error(ref_db, n, chain * U * np.asarray(S, np.float64))


def ratio(err, bound):
    """max err / bound with 0 / 0 = 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if np.size(r) else 0.0


def rms_amp(E, E_exact):
    """rms over blocks of |sqrt E - sqrt E_exact|"""
    d = np.sqrt(np.asarray(E).astype(LD)) - np.sqrt(np.asarray(E_exact).astype(LD))
    return float(np.sqrt(np.mean(d * d)))


def db_floor(ref_db, E_exact):
    """what a dB value's round trip through 10 log10 and back costs in sqrt E: 4 u (|dB| + 1) sqrt E, rms"""
    f = 4.0 * U * (np.abs(ref_db) + 1.0) * np.sqrt(np.asarray(E_exact).astype(np.float64))
    return float(np.sqrt(np.mean(f * f)))


# ------------------------------------------------------------------------------ Welch
WELCH_CLASSES = BLOCK_CLASSES + ("ramp", "tone7", "constant")
# (nperseg, nfft multiple, noverlap, nseg, sample_scale, nslots or "all", all five dtypes)
WELCH_ROWS = [
    (256, 1, 128, 3, 1.0 / 32768, 3, True),
    (256, 1, 0, 1, 1.0, "all", False),         # every bin of the 129
    (256, 4, 128, 7, 1.0, 128, False),         # two bins per lane, nothing left
    (256, 4, 0, 3, 1.0 / 32768, 129, False),   # two per lane, then one
    (255, 1, 127, 3, 1.0, 63, False),          # odd nperseg: the tail sample; odd nfft: no Nyquist bin
    (255, 4, 0, 7, 1.0 / 32768, 200, False),
    (1000, 1, 500, 3, 1.0, 64, False),
    (1000, 4, 0, 1, 1.0 / 32768, 65, False),
    (1000, 4, 500, 7, 1.0, 200, False),
    (4096, 1, 2048, 3, 1.0 / 32768, 3, False),
    (4096, 4, 0, 1, 1.0, 65, False),
]


def welch_bands(nfft, nslots):
    """three bands 0..a, a mid band, K-1-c..K-1 with nslots bins together (K = nfft // 2 + 1)"""
    K = nfft // 2 + 1
    if nslots == "all":
        a = K // 3
        return [(0, a - 1), (a, 2 * a - 1), (2 * a, K - 1)]
    a = (nslots + 2) // 3
    m = (nslots - a + 1) // 2
    c = nslots - a - m
    mid = K // 2 - m // 2
    assert a - 1 < mid and mid + m - 1 < K - c
    return [(0, a - 1), (mid, mid + m - 1), (K - c, K - 1)]


def welch_cases():
    """(nperseg, nfft, noverlap, nseg, block_size, sample_scale, bands, dtype)"""
    out = []
    for nperseg, mult, nov, nseg, ss, nslots, first in WELCH_ROWS:
        nfft = nperseg * mult
        block = nperseg + (nseg - 1) * (nperseg - nov)
        for dt in (ALL_DTYPES if first else (F64, I16)):
            out.append((nperseg, nfft, nov, nseg, block, ss, tuple(welch_bands(nfft, nslots)), dt))
    return out


def welch_case_id(c):
    nperseg, nfft, nov, nseg, block, ss, bands, dt = c
    return f"{nperseg}-{nfft}-{nov}-seg{nseg}-{'s15' if ss != 1.0 else 's0'}-{sum(h - l + 1 for l, h in bands)}-" \
           f"{np.dtype(dt).name}"


def welch_window(nperseg):
    from scipy.signal import get_window
    return get_window("hann", nperseg)  # periodic


def welch_scale(w, fs=FS):
    return 1.0 / (fs * float((w * w).sum()))


def welch_segments(x, block, nperseg, noverlap, sample_scale):
    """float64 samples times the sample scale, [blocks][segments][nperseg]"""
    nb = len(x) // block
    v = np.asarray(x)[: nb * block].astype(np.float64).reshape(nb, block) * sample_scale
    step = nperseg - noverlap
    nseg = (block - nperseg) // step + 1
    return np.stack([v[:, s * step: s * step + nperseg] for s in range(nseg)], axis=1)


def _ck(bins, nfft):
    k = np.asarray(bins, np.int64)
    edge = (k == 0) | ((nfft % 2 == 0) & (k == nfft // 2))
    return np.where(edge, 1.0, 2.0)


def welch_psd_ld(seg, w, nfft, bins, scale):
    """Welch PSD per bin in long double: exact mean detrend, window, scale, factor 2 off DC and off
    Nyquist, mean over segments; seg [blocks][segments][nperseg] -> [blocks][bins]"""
    nb, nseg, n = seg.shape
    v = seg.astype(LD)
    d = (v - v.sum(axis=2, keepdims=True) / LD(n)) * np.asarray(w, np.float64).astype(LD)
    re, im = dft_ld(d.reshape(nb * nseg, n), bins, nfft)
    P = (re * re + im * im).reshape(nb, nseg, -1) * LD(scale) * _ck(bins, nfft).astype(LD)
    return P.sum(axis=1) / LD(nseg)


def welch_psd_yardstick(seg, w, nfft, bins, scale, twiddle=np.float64):
    """one-lane textbook float64 Goertzel over each detrended, windowed segment"""
    nb, nseg, n = seg.shape
    d = (seg - seg.mean(axis=2, keepdims=True)) * w
    k = np.asarray(bins, np.int64)
    th = 2.0 * np.pi * k.astype(np.float64) / float(nfft)
    c2 = round_twiddle(2.0 * np.cos(th), twiddle)
    s1, s2 = _goertzel(d.reshape(nb, nseg, n, 1), c2, n)
    re, im = s1 - np.cos(th) * s2, np.sin(th) * s2
    P = (re * re + im * im) * scale * _ck(bins, nfft)
    return P.sum(axis=1) / nseg


def welch_S(seg, w):
    """(S_rms, A_rms) per block: S_s = sum |(x - mean) w| and A_s = mean |x| of each segment"""
    d = (seg - seg.mean(axis=2, keepdims=True)) * w
    S = np.abs(d).sum(axis=2)
    A = np.abs(seg).mean(axis=2)
    return np.sqrt((S * S).mean(axis=1)), np.sqrt((A * A).mean(axis=1))


def welch_dx(nperseg, nfft, bins, w, S_rms, A_rms):
    """per block and bin: the transform bound chain_w u S_rms + MEAN_CHAIN u A_rms |W_k| (module docstring)"""
    chain = np.array([M._goertzel_chain(nperseg, [k], nfft) + 2.0 for k in bins])
    Wk = np.abs(np.fft.rfft(w, n=nfft))[list(bins)] * (1 + 1e-9) + 64 * U * float(np.abs(w).sum())
    return chain[None, :] * U * S_rms[:, None] + mean_chain(nperseg) * U * A_rms[:, None] * Wk[None, :]


def welch_bin_bound(P_exact, dx, bins, nfft, scale):
    """|sqrt P_gpu - sqrt P_exact| <= sqrt(scale c_k) dx + 4 u sqrt P"""
    return np.sqrt(scale * _ck(bins, nfft))[None, :] * dx + 4.0 * U * np.sqrt(P_exact.astype(np.float64))


@functools.lru_cache(maxsize=None)
def welch_refs(cls, case, nblk=5):
    nperseg, nfft, nov, nseg, block, ss, bands, dt = case
    bins = tuple(k for lo, hi in bands for k in range(lo, hi + 1))
    x = class_samples(cls, nblk * block, np.dtype(dt), N=block, nfft=nfft, bins=bins, B=block, L=nperseg,
                      floor=True)
    x.setflags(write=False)
    w = welch_window(nperseg)
    scale = welch_scale(w)
    seg = welch_segments(x, block, nperseg, nov, ss)
    P = welch_psd_ld(seg, w, nfft, bins, scale)
    Y = welch_psd_yardstick(seg, w, nfft, bins, scale)
    S_rms, A_rms = welch_S(seg, w)
    dx = welch_dx(nperseg, nfft, bins, w, S_rms, A_rms)
    return dict(x=x, w=w, scale=scale, bins=bins, P=P, Y=Y, S_rms=S_rms, A_rms=A_rms, dx=dx)


def welch_band_db(P, bands):
    """10 log10 of each band's sum, -inf without power: [bands][blocks]"""
    out, j = [], 0
    for lo, hi in bands:
        n = hi - lo + 1
        s = P[:, j: j + n].sum(axis=1).astype(np.float64)
        with np.errstate(divide="ignore"):
            out.append(np.where(s > 0, 10 * np.log10(np.where(s > 0, s, 1.0)), -np.inf))
        j += n
    return np.array(out)
