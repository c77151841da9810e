"""Shapes, inputs, the long-double truth and the error bounds for the whole-band Welch row
(csrc/welch_fft.hip, msd_welch_spectrum*); helper, not a test module.

Truth: per processing block, ``spec_signals.ref_ld`` (the explicit long-double pipeline: samples times
sample_scale, minus the segment mean, times the float64 Hann values, rfft, |X|^2 scale, interior bins
doubled) gives every segment's power R_s[k]; the row is their mean over the segments in long double.

Per-bin bound.  ``spec_signals.bound_ratio``'s right-hand side with u = U64 bounds a segment in the
amplitude domain, |sqrt S_s - sqrt R_s| <= e_s with

    e_s[k] = sqrt(c_k) chain u sqrt(1.001 sum_k R_s[k]) + 3 u sqrt R_s[k],   c_0 = c_{nfft/2} = 1, else 2,

hence |S_s - R_s| <= 2 sqrt(R_s) e_s + e_s^2, and for the row averaged over nseg segments

    |S - R| <= (1 / nseg) sum_s (2 sqrt(R_s) e_s + e_s^2) + (nseg + 1) u R

(the last term: the nseg - 1 additions and the division).

``chain`` is counted from welch_fft.hip / welch_fft_plan.h by the rules of spec_signals.py (an add 1; a
complex multiply with FMA 2.83, its rounded twiddle 1.41 more; a multiply by -i or by an exact power of
two 0; detrend, window and its rounding 3), along the longest path from a sample to a bin, with
Lp = min(nperseg rounded up to a power of two, nfft / 2) and l = log2 Lp:
  * the sample_scale product 1;
  * the two-part mean subtraction, the window product 3;
  * the fold v[n] +- v[n + Lp] 1 (only where nperseg > nfft / 2; counted always);
  * the modulation, a real value times a rounded root: one rounded product per component, which is
    1 on the complex value, and the root's rounding 1.41: 2.41;
  * one radix-2 pass when l is odd (1 add), l // 2 radix-4 passes (2 adds each, the -i free);
  * a twiddle multiply in front of every pass but the first (4.24 each).
      chain = 1 + 3 + 1 + 2.41 + (l & 1) + 2 (l // 2) + 4.24 (passes - 1)
  256 / 4096 (l = 8): 28.1 -> 29;  16 / 16 (l = 3): 14.7 -> 15;  3000 / 4096 (l = 11): 39.6 -> 40;
  8192 / 16384 (l = 13): 45.9 -> 46.  There is no real split: the sub-transforms are complex.
It may not exceed ``spec_signals.CHAIN_ANY[nfft] + 1`` (stft_any's float64 chain plus the sample_scale
product): ``chain`` asserts that.  Never fitted to a measured error.

dB-mean bound: with B the row bound above, |sqrt S - sqrt R| <= B / sqrt R, so with t_k = (B_k / sqrt R_k) /
sqrt R_k a bin's dB value lies at most 20 log10(1 + t_k) above the reference's -- and at most
-20 log10(1 - t_k) below it, which is the larger of the two, equal to first order, and without limit
once t_k >= 1: the bin may then be exactly zero, -inf dB.  (scipy's own float64 row is, on nyquist_dc:
bins that are 1e-38 of the row in long double come out as exact zeros, tests/test_welch_fft_signals.py.
The upward term alone is therefore no bound that the reference passes.)  The bound on
np.mean(10 log10(row)) is the mean over the bins of -20 log10(1 - t_k), from the reference alone; where a
term is not finite (t_k >= 1, or a reference bin that is exactly zero) only finiteness and the -inf
handling are checked: the value is no NaN and not +inf.

The float64 reference's own detrend.  These bounds leave no bin out because the kernel claims an exact
detrend at any offset (its mean comes off in two parts).  scipy claims none: it subtracts
m^ = fl(np.mean(segment)), off the mean m by at most (ceil(log2 nperseg) + 2) u mean|x| (numpy's
pairwise sum, then the division), and that offset reaches bin k as delta |W_k| with W the window's
nfft-point transform.  On dc_quiet at a segment length that is no power of two (200, 3000), where the
quotient of the exact int16 sum is inexact, this is 52 to 124 times the kernel's bound at bin 0.
``scipy_mean_allowance`` is that term in the bound's units, per segment; tests/test_welch_fft_signals.py
adds it to e_s when it is scipy that is held to the bound, and only then: the kernel's bound
(tests/test_gpu_welch_spectrum.py) never includes it.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.signal import welch as sp_welch

import spec_signals as ss

FS = 4000
U = ss.U64

# (block_size, nperseg, noverlap, nfft) and the sample formats each is run in
SHAPES = (
    ((800, 256, 128, 4096), ("int16", "float32", "float64", "uint8")),   # the live default
    ((256, 256, 128, 256), ("int16",)),                                  # one segment, no padding
    ((64, 16, 8, 16), ("int16",)),                                       # smallest nfft
    ((200, 200, 100, 256), ("int16",)),                                  # nperseg no power of two
    ((800, 256, 255, 512), ("int16",)),                                  # step 1, many segments
    ((800, 256, 0, 4096), ("int16",)),                                   # no overlap, 3 segments
    ((512, 256, 128, 16384), ("int16",)),                                # maximal pruning
    ((16384, 8192, 4096, 16384), ("int16", "float64")),                  # R = 2
    ((4099, 3000, 1000, 4096), ("int16",)),                              # Lp = nfft / 2, folded: nothing to prune
)
CASES = tuple((shape, dt) for shape, dts in SHAPES for dt in dts)
CLASSES = ("carrier_weak", "fullscale_noise", "nyquist_dc", "dc_quiet", "impulses", "const")


def case_id(case):
    (bs, nper, nov, nfft), dt = case
    return f"{bs}-{nper}-{nov}-{nfft}-{dt}"


def sub_length(nperseg, nfft):
    """Lp of welch_fft_plan.h"""
    lp = 2
    while lp < nperseg and lp < nfft // 2:
        lp *= 2
    return lp


def chain(nperseg, nfft):
    """the kernel's chain (module docstring), held under its cap"""
    l = ss._log2(sub_length(nperseg, nfft))
    passes = (l & 1) + l // 2
    c = math.ceil(1 + 3 + 1 + (1 + ss.TWID) + (l & 1) + 2 * (l // 2) + (ss.CMUL + ss.TWID) * max(passes - 1, 0))
    assert c <= ss.CHAIN_ANY[nfft] + 1, (nperseg, nfft, c, ss.CHAIN_ANY[nfft])
    return c


def nseg_of(shape):
    bs, nper, nov, _ = shape
    return (bs - nper) // (nper - nov) + 1


def sample_scale(dtype):
    """the factor to soundfile's float64 of the cast samples (spec_signals.cast)"""
    dt = np.dtype(dtype)
    if dt == np.int16:
        return 1.0 / 32768.0
    if dt == np.int32:
        return 1.0 / 8388608.0
    if dt == np.uint8:
        return 1.0 / 128.0
    return 1.0


@functools.lru_cache(maxsize=None)
def block_signal(cls, shape, dtype, blocks=2):
    """class `cls` cast to `dtype`: `blocks` blocks and three samples short of another (impulses: its own
    length, at least one block); read-only"""
    bs, nper, _, _ = shape
    x = ss.cast(ss.samples(cls, nper, blocks * bs + bs - 3), dtype, cls)
    assert len(x) >= bs
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def nblocks(x, shape):
    return len(x) // shape[0]


@functools.lru_cache(maxsize=None)
def truth(cls, shape, dtype, blocks=2):
    """R_s [nb][nseg][K] in long double for block_signal(cls, shape, dtype, blocks)"""
    return truth_of(block_signal(cls, shape, dtype, blocks), shape, dtype)


def truth_of(x, shape, dtype):
    bs, nper, nov, nfft = shape
    ld = np.longdouble
    xs = np.asarray(x).astype(ld) * ld(sample_scale(dtype))
    out = [ss.ref_ld(xs[b * bs: (b + 1) * bs], FS, nper, nov, nfft).T for b in range(nblocks(x, shape))]
    R = np.stack(out)
    assert R.shape == (nblocks(x, shape), nseg_of(shape), nfft // 2 + 1) and R.dtype == ld
    R.setflags(write=False)
    return R


def scipy_mean_allowance(x, shape, dtype):
    """[nb][nseg][K]: the amplitude, in sqrt-of-density units, that the rounding of scipy's segment mean may
    put into each bin (module docstring); for the float64 reference's rows only"""
    import scipy.fft
    from scipy.signal import get_window
    bs, nper, nov, nfft = shape
    ld = np.longdouble
    w = get_window("hann", nper).astype(np.float64).astype(ld)
    Wk = np.abs(scipy.fft.rfft(w, n=nfft))
    ck = np.full(nfft // 2 + 1, 2.0, ld)
    ck[0] = ck[-1] = 1.0
    amp = Wk * np.sqrt(ck / (ld(FS) * (w * w).sum()))
    xs = np.abs(np.asarray(x).astype(ld) * ld(sample_scale(dtype)))
    slack = (math.ceil(math.log2(nper)) + 2) * ld(U)
    out = []
    for b in range(nblocks(x, shape)):
        fr = ss._frames(xs[b * bs: (b + 1) * bs], nper, nper - nov)
        out.append((slack * fr.mean(axis=1))[:, None] * amp[None, :])
    return np.stack(out)


def row_bound(Rseg, chain_c, extra=None):
    """(R [nb][K], B [nb][K]): the averaged reference row and the bound on |S - R| (module docstring);
    extra [nb][nseg][K]: added to e_s (scipy_mean_allowance, for scipy's own rows)"""
    ld = np.longdouble
    nb, nseg, K = Rseg.shape
    ck = np.full(K, 2.0, ld)
    ck[0] = ck[K - 1] = 1.0
    tot = Rseg.sum(axis=2, keepdims=True)
    e = np.sqrt(ck)[None, None, :] * (chain_c * ld(U)) * np.sqrt(ld(1.001) * tot) + 3 * ld(U) * np.sqrt(Rseg)
    if extra is not None:
        e = e + extra
    R = Rseg.sum(axis=1) / ld(nseg)
    B = (2 * np.sqrt(Rseg) * e + e * e).sum(axis=1) / ld(nseg) + (nseg + 1) * ld(U) * R
    return R, B


def row_ratio(S, R, B):
    """the largest |S - R| / B over every bin of every block (+inf: a non-finite or negative value, or an
    error where the bound is zero), and where: (ratio, (block, bin))"""
    S = np.asarray(S).astype(np.longdouble)
    assert S.shape == R.shape
    if not (np.all(np.isfinite(S)) and np.all(S >= 0)):
        return np.inf, (0, 0)
    err = np.abs(S - R)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0, err / B, np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), (int(at[0]), int(at[1]))


def db_mean_ref(R):
    with np.errstate(divide="ignore"):
        return (10 * np.log10(R)).mean(axis=1)


def db_mean_bound(R, B):
    """per block: the mean over the bins of -20 log10(1 - t), t = (B / sqrt R) / sqrt R (>= 20 log10(1 + t));
    not finite where some t >= 1 or a reference bin is zero (module docstring)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (B / np.sqrt(R)) / np.sqrt(R)
        term = np.where(t < 1, -20 * np.log10(1 - np.where(t < 1, t, 0)), np.inf)
    return term.mean(axis=1)


def scipy_rows(x, shape, dtype):
    """scipy.signal.welch of every block in float64: [nb][K]"""
    bs, nper, nov, nfft = shape
    xs = np.asarray(x).astype(np.float64) * sample_scale(dtype)
    return np.stack([sp_welch(xs[b * bs: (b + 1) * bs], FS, nperseg=nper, noverlap=nov, nfft=nfft)[1]
                     for b in range(nblocks(x, shape))])


def rms_rows(S, R):
    """spec_signals.rms_err with the blocks as frames: per block"""
    return ss.rms_err(np.asarray(S).T, np.asarray(R).T)
