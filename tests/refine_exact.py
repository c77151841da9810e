"""The exact C5 delta step (msd_iq_delta64_dev: csrc/refine_i8.hip's integer block DFT, then
csrc/refine.hip's frame_kernel) restated on the CPU.  Nothing here touches a GPU.

Three values of the same quantity -- the reference's band / noise dB delta of an STFT frame of I/Q
samples (scipy.signal.spectrogram of complex128 input, periodic Hann, constant detrend, density; band
sums in fftfreq mask order; 10 log10(E + 1e-12)) -- each one step closer to the kernel:

truth       in np.longdouble: the needed bins by a direct sum with exactly reduced twiddle angles
            (band_signals.dft_ld), the detrend, the periodic Hann as the three bin taps AND as a
            time-domain window (asserted to agree), |Y|^2 scale with scale = 8 / (3 N fs).  Its own error is
            N 2^-63 amp (truth_error), which every bar that uses it adds.
quantised   what the kernel would give if its float64 steps were exact: every 256-sample sub-block's
            sum_n x_n (T^c_n - i T^s_n) 2^-46 in exact integers, T from msd_i8_coeffs kind 2 (the very
            integers refine_i8.hip's table builder expands into digits; n < 256, the sample's place
            in its sub-block, as the kernel multiplies them), then the sub-blocks (W^{256 k s}), the R
            blocks (W^{k j D}), the taps, |Y|^2 and the band sums in long double, with the kernel's
            float64 scale (its sequential sum of w^2) so that only roundings separate the two.
yardstick   the same in plain float64 in the kernel's order: per sub-block the six digit sums A_d (exact
            integers; the kernel's 256 Ah + Al with its column constant) and the Horner p = fl(p 2^-8 +
            A_d) from d = 5 down to 0 (p 2^-8 is exact, so the kernel's fma rounds as the plain sum
            does: this step restates bit for bit), p 2^-6; the four sub-blocks summed with the
            float64-rounded W^{256 k s} in the kernel's order (bins 8 and 9: per digit, scaled, then
            the eight-lane tree); the R blocks rotated with the rounded W^{k j D}; the taps, |Y|^2
            scale, the band sums from 0.0 in mask order, 10 log10(E + 1e-12).  Products and sums round
            separately here where the kernel's fmas (and the compiler's contraction in frame_kernel)
            round once: no bit equality of delta is claimed, only a float64 computation of the same
            order to measure another one's precision against.

corrupt= makes the yardstick wrong the way a subtly wrong kernel or table would be (CORRUPTIONS); the
CPU tests (test_refine_exact.py) measure by what factor each misses which bar, and the GPU tests
(test_gpu_refine_exact.py) hold the kernel to the same bars."""
import functools
import math

import numpy as np

from band_signals import LD, _trig_ld, dft_ld
from meteorgpu import _lib

U = 2.0 ** -53
DBK = 4.342944819032518  # 10 / ln 10 as csrc/refine.hip's band_db_bound64 writes it
FLOOR = 1e-12
SUB, D8, ND = 256, 1024, 6
FLOOR_DB = 10.0 * math.log10(1e-12)  # an empty band's dB: 10 log10(0 + 1e-12)

CORRUPTIONS = ("drop_lsd", "swap_low_weights", "im_subtwiddle_sign", "swap_subblocks", "block_g_plus_1",
               "stale_tile", "rot_j_minus_1")


# ----------------------------------------------------------------------------- the plan
class Plan:
    """csrc/refine_plan.h's plan_refine restated: the needed bins (every band / noise bin and its two
    neighbours mod N, each once, in the order they are first asked for), the band lists in np.sum's
    mask order (bins >= 0 ascending, then the negative ones), the block geometry and the kernel's
    float64 density scale"""

    def __init__(self, N, hop, fs, band, noise):
        self.N, self.hop, self.fs = int(N), int(hop), float(fs)
        self.band, self.noise = (int(band[0]), int(band[1])), (int(noise[0]), int(noise[1]))
        self.D = math.gcd(self.N, self.hop)
        self.R = self.N // self.D
        self.k = []
        self.bidx, self.nidx = self._fill(*self.band), self._fill(*self.noise)
        self.km = [k % self.N for k in self.k]
        self.nk, self.nb, self.nn = len(self.k), len(self.bidx), len(self.nidx)
        self.dc = self.km.index(0) if 0 in self.km else -1
        sw = 0.0
        for n in range(self.N):  # plan_refine's sequential float64 sum of w^2
            w = 0.5 - 0.5 * math.cos(2.0 * math.pi * float(n) / float(self.N))
            sw += w * w
        self.scale = 1.0 / (self.fs * sw)
        self.scale_ld = LD(8) / (LD(3) * LD(self.N) * LD(self.fs))  # sum w^2 = 3 N / 8 exactly

    def _slot(self, kk):
        km = kk % self.N
        for i, k in enumerate(self.k):
            if k % self.N == km:
                return i
        self.k.append(kk)
        return len(self.k) - 1

    def _fill(self, lo, hi):
        order = [b for b in range(lo, hi + 1) if b >= 0] + [b for b in range(lo, hi + 1) if b < 0]
        return [(self._slot(b - 1), self._slot(b), self._slot(b + 1)) for b in order]

    def i8(self):
        """csrc/refine_i8.hip's i8_supported"""
        return self.D == D8 and self.dc < 0 and 1 <= self.nk <= 10

    def frame(self, x, t):
        """frame t's samples [N, 2]"""
        return np.asarray(x)[t * self.hop: t * self.hop + self.N]

    def first_block(self, t):
        return t * self.hop // self.D


def _pairs(x):
    """interleaved I/Q [2 n] or pairs [n, 2] -> [n, 2]"""
    x = np.asarray(x)
    return x.reshape(-1, 2) if x.ndim == 1 else x


# ----------------------------------------------------------------------------- truth
def _taps(V, idx):
    """Y = V[k] / 2 - V[k - 1] / 4 - V[k + 1] / 4 for the bins of idx; V = (re, im) [F, nk]"""
    a, c, e = (np.array([t[i] for t in idx], np.int64) for i in range(3))
    return tuple(v[:, c] / 2 - v[:, a] / 4 - v[:, e] / 4 for v in V)


def _cdft_ld(re, im, km, N):
    """sum_n (re + i im)_n e^{-2 pi i k n / N} at the bins km, long double"""
    ar, ai = dft_ld(re, km, N)
    br, bi = dft_ld(im, km, N)
    return ar - bi, ai + br


def truth(P, x, frames):
    """(delta, E_band, E_noise) of the frames in long double, from the samples (int16 integers or
    float32 values) alone"""
    x = _pairs(x)
    Z = np.stack([P.frame(x, t) for t in frames]).astype(LD)  # [F, N, 2]
    re, im = Z[..., 0], Z[..., 1]
    re = re - re.sum(axis=1, keepdims=True) / LD(P.N)
    im = im - im.sum(axis=1, keepdims=True) / LD(P.N)
    V = _cdft_ld(re, im, P.km, P.N)
    cs, _ = _trig_ld(P.N)
    w = LD(0.5) - cs / 2  # the periodic Hann, as a time-domain window
    out = []
    for idx in (P.bidx, P.nidx):
        if not idx:
            out.append(np.zeros(len(Z), LD))
            continue
        yr, yi = _taps(V, idx)
        wr, wi = _cdft_ld(re * w, im * w, [P.km[t[1]] for t in idx], P.N)
        l1 = (np.abs(re) + np.abs(im)).sum(axis=1, keepdims=True)
        tol = LD(P.N) * LD(2.0) ** -61 * l1 + LD(1e-4000)
        assert (np.abs(yr - wr) <= tol).all() and (np.abs(yi - wi) <= tol).all(), "taps and window disagree"
        out.append(((yr * yr + yi * yi) * P.scale_ld).sum(axis=1))
    Eb, En = out
    return _delta_ld(Eb, En), Eb, En


def _delta_ld(Eb, En):
    f = LD(10) / np.log(LD(10))
    return f * np.log(Eb + LD(FLOOR)) - f * np.log(En + LD(FLOOR))


def truth_error(P, amp):
    """truth's own error in a bin's amplitude: N 2^-63 amp"""
    return P.N * 2.0 ** -63 * np.asarray(amp, np.float64)


# ----------------------------------------------------------------------------- digits and integers
def digits6(T):
    """balanced base-256 digits of int64 T (i8_digits.h's balanced_digits<6>): d [6, ...] with
    T = sum_b d[b] 256^(5 - b), every digit in [-128, 127]; and whether every T fits"""
    T = np.array(T, dtype=np.int64)
    d = np.empty((ND,) + T.shape, np.int64)
    for b in range(ND - 1, -1, -1):
        r = (T % 256 + 128) % 256 - 128
        d[b] = r
        T = (T - r) // 256
    return d, bool((T == 0).all())


@functools.lru_cache(maxsize=64)
def coeffs(N, km):
    """(T^c, T^s) [256] of bin km: the library's integers (msd_i8_coeffs kind 2)"""
    return (_lib.i8_coeffs(_lib.I8_REFINE, SUB, N, km, 0), _lib.i8_coeffs(_lib.I8_REFINE, SUB, N, km, 1))


@functools.lru_cache(maxsize=64)
def column_digits(N, km):
    """the digits of the kernel's four coefficient columns of bin km, [6, 256] each: the real
    component's (I: T^c, Q: T^s) and the imaginary component's (I: -T^s, Q: T^c).  -T^s is expanded on
    its own: balanced digits are not odd (128 = (1, -128), -128 = (0, -128))"""
    Tc, Ts = coeffs(N, km)
    out = []
    for T in (Tc, Ts, -Ts, Tc):
        d, fits = digits6(T)
        assert fits
        out.append(d)
    return out


def _imm(X, C):
    """X [M, L] @ C [L] or [L, n] in int64 (numpy's integer matmul: exact, no BLAS)"""
    return np.matmul(np.ascontiguousarray(X, dtype=np.int64), np.ascontiguousarray(C, dtype=np.int64))


def _subblocks(P, x, blocks):
    """(I, Q) [nblk * 4, 256] int64 of the blocks (sub-block s of block i at row 4 i + s)"""
    x = _pairs(x)
    X = np.stack([x[m * P.D: (m + 1) * P.D] for m in blocks]).astype(np.int64).reshape(len(blocks) * 4, SUB, 2)
    return X[..., 0], X[..., 1]


def _unit_ld(P, j):
    """(cos, sin) of 2 pi j / N in long double, j reduced exactly"""
    c, s = _trig_ld(P.N)
    j = np.asarray(j, np.int64) % P.N
    return c[j], s[j]


def block_values_quantised(P, x, blocks):
    """B_m[k] = sum_s W^{256 k s} sum_{n < 256} x_{256 s + n} (T^c_n - i T^s_n) 2^-46 for the blocks m and the
    needed bins: the inner sums exact integers (T in two 23-bit halves: |sum| <= 2^15 2^23 2^9 = 2^47 per
    half in int64), the rest long double; (re, im) [nblk, nk]"""
    I, Q = _subblocks(P, x, blocks)
    nblk = len(blocks)
    re, im = np.empty((nblk, P.nk), LD), np.empty((nblk, P.nk), LD)
    for b, km in enumerate(P.km):
        Tc, Ts = coeffs(P.N, km)
        parts = []
        for T in (Tc, Ts):
            Th, Tl = T >> 23, T & ((1 << 23) - 1)
            parts.append([(_imm(V, Th).astype(LD) * LD(2.0 ** 23) + _imm(V, Tl).astype(LD)) * LD(2.0 ** -46)
                          for V in (I, Q)])
        (Ic, Qc), (Is, Qs) = parts
        pr, pi = (Ic + Qs).reshape(nblk, 4), (Qc - Is).reshape(nblk, 4)  # re = I C + Q S, im = Q C - I S
        c, s = _unit_ld(P, km * SUB * np.arange(4))
        re[:, b] = (pr * c + pi * s).sum(axis=1)
        im[:, b] = (pi * c - pr * s).sum(axis=1)
    return re, im


def _frame_blocks(P, frames, extra=0):
    """the blocks the frames read (plus `extra` past each), sorted, and each frame's row indices [F, R + extra]"""
    need = sorted({P.first_block(t) + j for t in frames for j in range(P.R + extra)})
    pos = {m: i for i, m in enumerate(need)}
    return need, np.array([[pos[P.first_block(t) + j] for j in range(P.R + extra)] for t in frames], np.int64)


def quantised(P, x, frames):
    """(delta, E_band, E_noise) in long double from the exact integer sub-block sums: the kernel with
    exact float64 steps (int8 path only: blocks of 1024 samples, no needed bin 0)"""
    assert P.i8()
    need, rows = _frame_blocks(P, frames)
    br, bi = block_values_quantised(P, x, need)
    vr, vi = br[rows], bi[rows]  # [F, R, nk]
    c, s = _unit_ld(P, P.D * ((np.array(P.km, np.int64)[None, :] * np.arange(P.R)[:, None]) % P.R))  # [R, nk]
    V = ((vr * c + vi * s).sum(axis=1), (vi * c - vr * s).sum(axis=1))
    out = []
    for idx in (P.bidx, P.nidx):
        if not idx:
            out.append(np.zeros(len(frames), LD))
            continue
        yr, yi = _taps(V, idx)
        out.append(((yr * yr + yi * yi) * LD(P.scale)).sum(axis=1))
    return _delta_ld(out[0], out[1]), out[0], out[1]


# ----------------------------------------------------------------------------- the yardstick
def _unit_f64(P, j):
    c, s = _unit_ld(P, j)
    return c.astype(np.float64), s.astype(np.float64)


def block_values_f64(P, x, blocks, corrupt=None):
    """the kernel's block values in float64 in its own order; (re, im) [nblk, nk]"""
    I, Q = _subblocks(P, x, blocks)
    nblk = len(blocks)
    re, im = np.empty((nblk, P.nk)), np.empty((nblk, P.nk))
    for b, km in enumerate(P.km):
        dig = [d.copy() for d in column_digits(P.N, km)]
        if corrupt == "drop_lsd":
            for d in dig:
                d[5] = 0
        elif corrupt == "swap_low_weights":
            for d in dig:
                d[[4, 5]] = d[[5, 4]]
        # the digit sums A_d per sub-block: exact integers, |A_d| <= 2^15 2^7 2^9 = 2^31, exact as float64
        Ar = np.stack([(_imm(I, dig[0][d]) + _imm(Q, dig[1][d])).reshape(nblk, 4) for d in range(ND)]).astype(np.float64)
        Ai = np.stack([(_imm(I, dig[2][d]) + _imm(Q, dig[3][d])).reshape(nblk, 4) for d in range(ND)]).astype(np.float64)
        if corrupt == "swap_subblocks":  # sub-blocks 1 and 2 meet each other's twiddle
            Ar, Ai = Ar[:, :, [0, 2, 1, 3]], Ai[:, :, [0, 2, 1, 3]]
        c, s = _unit_f64(P, km * SUB * np.arange(4))
        si = s if corrupt == "im_subtwiddle_sign" else -s  # the imaginary lane's partner twiddle: -sin
        if b < 8:  # a lane per component: the Horner over the digits, then the four sub-blocks
            pr, pi = Ar[5], Ai[5]
            for d in range(4, -1, -1):
                pr = pr * 2.0 ** -8 + Ar[d]
                pi = pi * 2.0 ** -8 + Ai[d]
            pr, pi = pr * 2.0 ** -6, pi * 2.0 ** -6
            yr, yi = np.zeros(nblk), np.zeros(nblk)
            for r in range(4):
                yr = yr + pr[:, r] * c[r]
                yr = yr + pi[:, r] * s[r]
                yi = yi + pi[:, r] * c[r]
                yi = yi + pr[:, r] * si[r]
        else:  # bins 8, 9: a lane per digit: the four sub-blocks, the digit's scale, the eight-lane tree
            ar, ai = [], []
            for d in range(ND):
                xr, xi = np.zeros(nblk), np.zeros(nblk)
                for r in range(4):
                    xr = xr + Ar[d][:, r] * c[r]
                    xr = xr + Ai[d][:, r] * s[r]
                    xi = xi + Ai[d][:, r] * c[r]
                    xi = xi + Ar[d][:, r] * si[r]
                ar.append(xr * 2.0 ** (-6 - 8 * d))
                ai.append(xi * 2.0 ** (-6 - 8 * d))
            yr = ((ar[0] + ar[1]) + (ar[2] + ar[3])) + (ar[4] + ar[5])
            yi = ((ai[0] + ai[1]) + (ai[2] + ai[3])) + (ai[4] + ai[5])
        re[:, b], im[:, b] = yr, yi
    return re, im


def yardstick(P, x, frames, corrupt=None, where=None):
    """(delta, E_band, E_noise) in float64 in the kernel's order.  corrupt: one of CORRUPTIONS; where: the
    positions in `frames` that the frame-level corruptions (block_g_plus_1: block 1 of the frame taken
    from the next compact position; stale_tile: all R blocks those of the frame R blocks earlier, a
    tile's four blocks never rewritten) hit -- default all"""
    assert P.i8()
    assert corrupt is None or corrupt in CORRUPTIONS
    frames = list(frames)
    hit = np.zeros(len(frames), bool)
    hit[list(range(len(frames))) if where is None else list(where)] = True
    need, rows = _frame_blocks(P, frames, extra=1 if corrupt == "block_g_plus_1" else 0)
    if corrupt == "stale_tile":
        old = [t - (4 * P.D // P.hop if 4 * P.D % P.hop == 0 else 1) for t in frames]
        assert min(old) >= 0
        need2, rows2 = _frame_blocks(P, old)
        br2, bi2 = block_values_f64(P, x, need2)
    br, bi = block_values_f64(P, x, need, corrupt)
    vr, vi = br[rows], bi[rows]  # [F, R (+ 1), nk]
    if corrupt == "block_g_plus_1":
        j = min(1, P.R - 1)
        vr[hit, j], vi[hit, j] = vr[hit, j + 1], vi[hit, j + 1]
        vr, vi = vr[:, :P.R], vi[:, :P.R]
    elif corrupt == "stale_tile":
        vr[hit], vi[hit] = br2[rows2][hit], bi2[rows2][hit]
    jr = np.arange(P.R) - (1 if corrupt == "rot_j_minus_1" else 0)
    c, s = _unit_f64(P, P.D * ((np.array(P.km, np.int64)[None, :] * jr[:, None]) % P.R))  # rot = (c, -s) [R, nk]
    zr, zi = vr[:, 0].copy(), vi[:, 0].copy()
    for j in range(1, P.R):  # z + cmul(rot_j, v_j), rot = c - i s
        zr = zr + (c[j] * vr[:, j] - (-s[j]) * vi[:, j])
        zi = zi + (c[j] * vi[:, j] + (-s[j]) * vr[:, j])
    out = []
    for idx in (P.bidx, P.nidx):
        E = np.zeros(len(frames))
        for a, cc, e in idx:
            yr = 0.5 * zr[:, cc] - 0.25 * zr[:, a] - 0.25 * zr[:, e]
            yi = 0.5 * zi[:, cc] - 0.25 * zi[:, a] - 0.25 * zi[:, e]
            E = E + (yr * yr + yi * yi) * P.scale
        out.append(E)
    return 10.0 * np.log10(out[0] + FLOOR) - 10.0 * np.log10(out[1] + FLOOR), out[0], out[1]


# ----------------------------------------------------------------------------- bounds
def frame_sums(P, x, frames):
    """(sum I, sum Q) [F, 2] int64 and sum (|I| + |Q|) [F] int64 of the frames: exact"""
    x = _pairs(x)
    Z = np.stack([P.frame(x, t) for t in frames]).astype(np.int64)
    return Z.sum(axis=1), np.abs(Z).sum(axis=(1, 2))


def _amp(P, l1, sums):
    """frame_kernel's amp = (l1 + N (|mean I| + |mean Q|)) sqrt(scale) in float64"""
    sums = np.asarray(sums, np.float64)
    mx, my = sums[:, 0] / P.N, sums[:, 1] / P.N
    return (np.asarray(l1, np.float64) + float(P.N) * (np.abs(mx) + np.abs(my))) * math.sqrt(P.scale)


def amp(P, x, frames):
    """frame_kernel's amp of the frames from the exact integer sums: an upper bound of sum |v_n w_n| sqrt(scale)"""
    sums, l1 = frame_sums(P, x, frames)
    return _amp(P, l1, sums)


def l1_device(P, x, frames):
    """the int8 kernel's own upper bound of a frame's sum (|I| + |Q|): 256 (sum |x >> 8| + 2 D) per block,
    doubled where the block table carries no sums (at most 8 needed bins)"""
    x = _pairs(x)
    out = []
    for t in frames:
        z = P.frame(x, t).astype(np.int64).reshape(P.R, P.D * 2)
        l1 = 256.0 * (np.abs(z >> 8).sum(axis=1).astype(np.float64) + 2.0 * P.D)
        out.append(float((l1 * (2.0 if P.nk <= 8 else 1.0)).sum()))
    return np.array(out)


def amp_device(P, x, frames):
    """frame_kernel's amp as the int8 path forms it (l1_device; the block sums all 0 where nk <= 8)"""
    sums, _ = frame_sums(P, x, frames)
    if P.nk <= 8:
        sums = np.zeros_like(sums)
    return _amp(P, l1_device(P, x, frames), sums)


def db_bound(E, n, d):
    """csrc/refine.hip's band_db_bound64: the dB error of a band of n bins with energy E when every
    bin's amplitude is off by at most d"""
    E, d = np.asarray(E, np.float64), np.asarray(d, np.float64)
    if n <= 0:
        return np.zeros(np.broadcast(E, d).shape)
    dE = 2.0 * d * np.sqrt(float(n) * E) + 3.0 * float(n) * d * d + 2.0 * (float(n) + 4.0) * U * E
    den = E + 1e-12 - dE
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, DBK * dE / den * (1.0 + 1e-9), np.inf)


def ed(P, Eb, En, amp_, chain):
    """frame_kernel's ed from the band energies, amp and the chain (own + combine + reference)"""
    d = chain * U * np.asarray(amp_, np.float64)
    return db_bound(Eb, P.nb, d) + db_bound(En, P.nn, d) + 1e-13


def delta_bar(P, Eb, En, d):
    """a bin amplitude bound d carried through both bands' dB: the bar on |delta - delta_ref|"""
    return db_bound(Eb, P.nb, d) + db_bound(En, P.nn, d) + 1e-13


def chains(P, dtype_code, goertzel=False):
    """(own, combine, reference) from the library (msd_iq_delta64_chain)"""
    return _lib.iq_delta64_chain(P.N, P.hop, P.fs, P.band, P.noise, dtype_code, goertzel)


def sqrtE_bar(P, n, E, amp_, own, combine):
    """bar 2: |sqrt E_gpu - sqrt E_quantised| <= sqrt n (own - 91 + combine) u amp + 3 u sqrt E"""
    return (math.sqrt(n) * (own - _lib.REFINE_I8_CHAIN_QUANT + combine) * U * np.asarray(amp_, np.float64)
            + 3.0 * U * np.sqrt(np.asarray(E, np.float64)))


def rms_ld(delta, dq):
    """bar 3's figure: the rms over the frames of delta - delta_quantised, the difference taken in long
    double (delta_quantised rounded to float64 first would hide half an ulp of it)"""
    d = np.asarray(delta).astype(LD) - np.asarray(dq, LD)
    return float(np.sqrt(np.mean(d * d)))


def recover_E(db_other_empty_delta, band):
    """E of the one non-empty band from delta when the other band is empty (its dB exactly
    10 log10(1e-12)): band = 0 the signal band (delta = dB_b - floor), 1 the noise band"""
    d = np.asarray(db_other_empty_delta, np.float64)
    db = d + FLOOR_DB if band == 0 else FLOOR_DB - d
    return 10.0 ** (db / 10.0) - FLOOR


# ----------------------------------------------------------------------------- inputs
def signals(P, nframes, seed=0):
    """{name: interleaved int16 [2 n]} of the issue's input classes for nframes frames of the plan;
    NOISE_LIKE names the ones bar 3 (precision) applies to"""
    rng = np.random.default_rng(seed)
    n = (nframes - 1) * P.hop + P.N
    N = P.N
    t = np.arange(n)
    out = {}

    def put(name, z):
        z = np.asarray(z)
        if z.ndim == 1 and np.iscomplexobj(z):
            z = np.stack([z.real, z.imag], axis=1)
        out[name] = np.clip(np.round(z), -32768, 32767).astype(np.int16).reshape(-1)

    put("noise300", rng.normal(0, 300, (n, 2)))
    put("full_scale", rng.choice([-32768, 32767], (n, 2)))
    put("small3", rng.integers(-3, 4, (n, 2)))
    for c in (32767, -32768, 255, 256, -128, -129, -1, 0):
        put(f"const{c}", np.full((n, 2), c))
    for at in (0, 255, 256, 1023, 1024, N - 1):
        if at < N:
            z = np.zeros((n, 2))
            z[at::N, 0] = 1  # frame 0 has it at n = at, frame t at (at - t hop) mod N
            put(f"impulse{at}", z)
    kb = P.k[P.bidx[0][1]] if P.bidx else P.k[P.nidx[0][1]]
    for name, k in (("tone_on_bin", kb), ("tone_on_neighbour", kb + 1), ("tone_two_off", kb + 2)):
        put(name, 23000 * np.exp(2j * np.pi * ((k * t) % N) / N))
    put("weak_beside_carrier", 23000 * np.exp(2j * np.pi * (((kb + 40) * t) % N) / N)
        + 2.3 * np.exp(2j * np.pi * ((kb * t) % N) / N))
    # per digit, the +- full-scale pattern that follows that digit's sign along one column (the real
    # component's I coefficients of the first needed bin, tiled over the sub-blocks): the digit sum at its extreme
    if P.i8():
        dig = column_digits(P.N, P.km[0])
        for d in range(ND):
            zi = np.resize(np.where(dig[0][d] > 0, 32767, -32768), n)
            zq = np.resize(np.where(dig[1][d] > 0, 32767, -32768), n)
            put(f"digit{d}_pos", np.stack([zi, zq], axis=1))
            put(f"digit{d}_neg", np.stack([-1 - zi, -1 - zq], axis=1))
    return out


NOISE_LIKE = ("noise300", "full_scale")
