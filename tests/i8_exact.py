"""The arithmetic of the two int8 matrix-core band kernels (csrc/block_i8.hip, csrc/welch_i8.hip)
restated on the CPU: in integers from the library's own coefficients (msd_i8_coeffs, the functions
the plans' builders call), then in float64 in each kernel's own order.  Nothing here touches a GPU.

Block path.  T_n = round(w_n cos / -sin 2^54) in seven balanced base-256 digits d_0 (most
significant) .. d_6.  Per digit A_d = sum_n x_n d_dn is an exact integer (|A_d| <= 2^15 2^7 2^10 =
2^32: the kernel's 256 Ah + Al with its column constant 128 sum d, exact in float64), then the
kernel's Horner p = fl(p 2^-8 + A_d) from d = 6 down to 0 (p 2^-8 is exact, so the fma's single
rounding is float64's plain one), p 2^-6 (exact), E_k = fl(fl(p^2) + fl(q^2)), the band sums in
numpy's order (np_sum_small: one pairwise leaf), + 1e-12, 10 log10, delta.

Welch path.  T_n ~ c'_n 2^53 summing to zero.  v = float(sum_n x_n T_n): the integer sum exactly
(each T in two 27-bit halves, int64 matmuls: |sum| <= 2^15 2^28 2^9 = 2^52; combined as Python
ints) and Python's correctly rounded int -> float, the single rounding digit_sum / digit_sum_pairs
claim.  Then x xscale when the scale is not folded, fl(fl(v^2) + fl(q^2)) (the file compiles with
contraction off), x (pscale x doubling) with pscale as launch_welch_i8 forms it, the segment sum in
segment order and s / nseg (the kernel's Markstein step claims the correctly rounded quotient).

mutate() corrupts a plan's digits the way a subtly wrong kernel would, and adversarial_blocks()
builds the int16 inputs that reach the sample split's and the accumulators' edges; the CPU tests
(test_i8_exact.py) and the GPU tests (test_gpu_i8_exact.py) share both."""
import math

import numpy as np

from meteorgpu import _lib

U = 2.0 ** -53
ND = 7
DB = 10.0 / math.log(10.0)


# ----------------------------------------------------------------------------- digits
def digits7(T):
    """balanced base-256 digits of int64 T: (d [7, ...] with T = sum_b d[b] 256^(6 - b), every digit
    in [-128, 127]; fits: no carry left over anywhere), i8_digits.h's balanced_digits<7>"""
    T = np.array(T, dtype=np.int64)
    d = np.empty((ND,) + T.shape, np.int64)
    for b in range(ND - 1, -1, -1):
        r = (T % 256 + 128) % 256 - 128
        d[b] = r
        T = (T - r) // 256
    return d, bool((T == 0).all())


def undigits(d):
    """T = sum_b d[b] 256^(6 - b)"""
    T = np.zeros(d.shape[1:], np.int64)
    for b in range(ND):
        T = T * 256 + d[b]
    return T


def frag_sample(ks, g, j):
    """the sample that byte j (< 16) of lane group g's (< 4) fragment of K step ks holds (i8_digits.h)"""
    return 64 * ks + (8 * g + j if j < 8 else 32 + 8 * g + (j - 8))


MUTATIONS = ("drop_lsd", "swap_low_weights", "drop_k_step", "swap_frag_bytes")


def mutate(dig, kind, comp=0):
    """a copy of the digits dig [7, ncomp, L] corrupted as a subtly wrong kernel or table would be:
    drop_lsd: the least-significant digit lost; swap_low_weights: the two lowest digits take each
    other's weight (a digit weight off by one place); drop_k_step: one K step of 64 samples (the
    last) skipped; swap_frag_bytes: two bytes of one fragment (digit 3 of component comp, K step 0,
    lane group 1, bytes 2 and 9) exchanged"""
    d = dig.copy()
    if kind == "drop_lsd":
        d[6] = 0
    elif kind == "swap_low_weights":
        d[[5, 6]] = d[[6, 5]]
    elif kind == "drop_k_step":
        d[:, :, d.shape[2] - 64:] = 0
    elif kind == "swap_frag_bytes":
        n1, n2 = frag_sample(0, 1, 2), frag_sample(0, 1, 9)
        d[3, comp, [n1, n2]] = d[3, comp, [n2, n1]]
    else:
        raise ValueError(kind)
    return d


def np_sum_small(p):
    """np.sum over the last axis (n <= 8 values) in numpy's order, as np_reduce.h's np_sum_small
    takes it: 0.0 + the pairwise leaf (n < 8: in order from 0.0; n = 8: the eight accumulators as
    ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)))"""
    n = p.shape[-1]
    assert n <= 8
    if n == 0:
        return np.zeros(p.shape[:-1])
    if n < 8:
        s = np.zeros(p.shape[:-1])
        for i in range(n):
            s = s + p[..., i]
    else:
        s = ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])) + ((p[..., 4] + p[..., 5]) + (p[..., 6] + p[..., 7]))
    return 0.0 + s


def _imatmul(X, C):
    """X [R, L] @ C [ncol, L]^T in int64 (no BLAS: exact)"""
    return np.matmul(np.ascontiguousarray(X, dtype=np.int64), np.ascontiguousarray(C, dtype=np.int64).T)


# ----------------------------------------------------------------------------- block path
class BlockI8:
    """block_i8.hip's plan for a window (the L = min(B, nfft) values used), nfft and the inclusive
    bin ranges band / noise ((0, -1): empty)"""

    def __init__(self, window, nfft, band, noise):
        self.w = np.ascontiguousarray(window, dtype=np.float64)
        self.L, self.nfft = self.w.size, int(nfft)
        self.nband = max(0, band[1] - band[0] + 1)
        self.nnoise = max(0, noise[1] - noise[0] + 1)
        self.bins = list(range(band[0], band[1] + 1)) + list(range(noise[0], noise[1] + 1))
        # [ncomp, L]: component 2 j the real part of bin j, 2 j + 1 the imaginary part
        self.T = np.stack([_lib.i8_coeffs(_lib.I8_BLOCK, self.w, self.nfft, k, part)
                           for k in self.bins for part in (0, 1)])
        self.dig, self.fits = digits7(self.T)

    def components(self, X, dig=None):
        """the kernel's float64 components [nblk, ncomp] of blocks X [nblk, >= L] (the first L used)"""
        dig = self.dig if dig is None else dig
        X = np.asarray(X)[:, :self.L]
        p = _imatmul(X, dig[ND - 1]).astype(np.float64)  # |A_d| <= 2^32: exact
        for d in range(ND - 2, -1, -1):
            p = p * 2.0 ** -8 + _imatmul(X, dig[d]).astype(np.float64)  # one rounding per step
        return p * 2.0 ** -6

    def energies(self, X, dig=None):
        """(band energy + 1e-12, noise energy + 1e-12) per block, the kernel's output pair"""
        p = self.components(X, dig)
        re, im = p[:, 0::2], p[:, 1::2]
        E = re * re + im * im
        return np_sum_small(E[:, :self.nband]) + 1e-12, np_sum_small(E[:, self.nband:]) + 1e-12

    def db(self, X, dig=None):
        """(band dB, noise dB, delta) per block (block_db_kernel)"""
        eb, en = self.energies(X, dig)
        bd, nd = 10.0 * np.log10(eb), 10.0 * np.log10(en)
        return bd, nd, bd - nd


def block_db_bound(db):
    """the bar on |dB_gpu - dB_restated| of one band: (10 / ln 10) 2 u for one rounding of each bin
    power's p p + q q either way (contracted into an fma or not; relative, so it carries through the
    sums of non-negative terms), 4 u (|dB| + 1) for the logarithm and its product (the term
    margin.band_db_error charges).  Recounted in block_i8.hip: the Makefile compiles that file with
    -ffp-contract=off and the power is a plain p * p + q * q, so no product contracts and the first
    term is slack in this build; it stays, so that the bar does not depend on that flag."""
    db = np.asarray(db, dtype=np.float64)
    return DB * 2.0 * U + 4.0 * U * (np.abs(db) + 1.0)


# ----------------------------------------------------------------------------- Welch path
def _normal(v):
    return math.isfinite(v) and abs(v) >= 2.2250738585072014e-308


class WelchI8:
    """welch_i8.hip's plan: block_size, nperseg, noverlap, nfft, the sample scale, the density scale
    1 / (fs sum w^2), the inclusive band bin ranges and the window"""

    def __init__(self, block_size, nperseg, noverlap, nfft, sample_scale, scale, bands, window):
        self.B, self.L, self.nfft = int(block_size), int(nperseg), int(nfft)
        self.step = self.L - int(noverlap)
        self.nseg = (self.B - self.L) // self.step + 1
        self.w = np.ascontiguousarray(window, dtype=np.float64)
        self.bands = [(int(lo), int(hi)) for lo, hi in bands]
        self.bins = [k for lo, hi in self.bands for k in range(lo, hi + 1)]
        self.nslots = len(self.bins)
        self.dbl = np.array([1.0 if k == 0 or (self.nfft % 2 == 0 and k == self.nfft // 2) else 2.0
                             for k in self.bins])
        self.T = np.stack([_lib.i8_coeffs(_lib.I8_WELCH, self.w, self.nfft, k, part)
                           for k in self.bins for part in (0, 1)])
        self.dig, self.fits = digits7(self.T)
        # launch_welch_i8: xscale = 2^-53 sample_scale; folded into the density scale when a power of two
        self.xscale = math.ldexp(float(sample_scale), -53)
        folded = float(scale) * self.xscale * self.xscale
        self.fold = (abs(math.frexp(self.xscale)[0]) == 0.5 and _normal(folded)
                     and _normal(self.xscale * self.xscale))
        self.pscale = folded if self.fold else float(scale)
        # welch_i8_build: |a_w| <= 128 (sum_n |d_(7-w)n| + sum_n |d_(6-w)n|); the int32 pairs need
        # |a_w| + 256 |a_(w+1)| < 2^31 at w = 0, 2, 4, 6 in every component
        sad = np.abs(self.dig).sum(axis=2)  # [7, ncomp]
        z = np.zeros_like(sad[0])
        bound = [128 * ((sad[7 - w] if w >= 1 else z) + (sad[6 - w] if w <= 6 else z)) for w in range(8)]
        self.pair_bound = np.stack([bound[w] + 256 * bound[w + 1] for w in range(0, 8, 2)])  # [4, ncomp]
        self.pairs = bool((self.pair_bound < 2 ** 31).all())

    def segments(self, X):
        """X [nb, B] -> [nb * nseg, L], a block's segments in order"""
        X = np.asarray(X)
        return np.stack([X[:, s * self.step: s * self.step + self.L] for s in range(self.nseg)],
                        axis=1).reshape(-1, self.L)

    def sums(self, S, T=None):
        """the exact integers sum_n x_n T_n of segments S [R, L]: object array [R, ncomp] of Python ints"""
        T = self.T if T is None else T
        Th, Tl = T >> 27, T & ((1 << 27) - 1)  # T = 2^27 Th + Tl, |Th| <= 2^28, 0 <= Tl < 2^27
        return _imatmul(S, Th).astype(object) * (1 << 27) + _imatmul(S, Tl).astype(object)

    def accumulators(self, S):
        """the kernel's eight int32 accumulators per (segment, component) as int64 [8, R, ncomp]:
        a_w = sum_n h_n d_(7-w)n + sum_n l'_n d_(6-w)n with x = 256 h + l' + 128"""
        S = np.asarray(S, dtype=np.int64)
        h, lp = S >> 8, (S & 255) - 128
        R = S.shape[0]
        zero = np.zeros((R, self.dig.shape[1]), np.int64)
        return np.stack([(_imatmul(h, self.dig[7 - w]) if w >= 1 else zero)
                         + (_imatmul(lp, self.dig[6 - w]) if w <= 6 else zero) for w in range(8)])

    def psd(self, X, T=None, offset=None):
        """the per-block PSD of the band bins [nb, nslots] of blocks X [nb, B].  T: other integers
        (a mutated plan's); offset: an integer added to every digit sum (a wrapped int32 pair)"""
        nb = np.asarray(X).shape[0]
        S = self.sums(self.segments(X), T)
        if offset is not None:
            S = S + offset
        v = S.astype(np.float64)  # Python int -> float: correctly rounded
        if not self.fold:
            v = v * self.xscale
        re, im = v[:, 0::2], v[:, 1::2]
        p = (re * re + im * im) * (self.pscale * self.dbl)
        p = p.reshape(nb, self.nseg, self.nslots)
        s = p[:, 0]
        for k in range(1, self.nseg):
            s = s + p[:, k]
        return s / float(self.nseg)

    def band_db(self, psd):
        """10 log10(np.sum(psd[band])) per band [nbands, nb], -inf where the sum is not > 0"""
        out, s0 = [], 0
        for lo, hi in self.bands:
            n = max(0, hi - lo + 1)
            P = np.array([np.sum(row[s0: s0 + n]) for row in np.ascontiguousarray(psd)]) if n else np.zeros(len(psd))
            with np.errstate(divide="ignore"):
                out.append(np.where(P > 0, 10.0 * np.log10(np.where(P > 0, P, 1.0)), -np.inf))
            s0 += n
        return np.array(out)


# ----------------------------------------------------------------------------- inputs
CONSTANTS = (32767, -32768, 1, -1, 255, 256, -128, -129)  # full scale and the boundaries of h and l'
IMPULSES = (0, 7, 8, 31, 32, 39, 63, 64)                  # + L - 1: every group and half of frag_sample


def adversarial_blocks(B, L, dig_comp, seed):
    """(names, int16 [n, B]): the inputs of the exactness tests for blocks of B samples whose first L
    (block path) or nseg overlapping stretches of L (Welch path) are transformed.  dig_comp [7, L]:
    one component's digits, for the inputs that drive an accumulator to its extreme -- per weight
    256^w the digit that h multiplies into it (digit 7 - w; w = 0: digit 6 through l'), x_n = -32768
    where the digit is positive else 32767, and the opposite assignment"""
    rng = np.random.default_rng(seed)
    names, rows = [], []

    def add(name, v):
        names.append(name)
        rows.append(np.resize(np.asarray(v), B) if np.asarray(v).size != B else np.asarray(v))

    for i in range(2):
        add(f"noise{i}", np.clip(np.round(rng.normal(0, 300, B)), -32768, 32767))
    add("random_full_scale", rng.choice([-32768, 32767], B))
    for c in CONSTANTS:
        add(f"const{c}", np.full(B, c))
    add("alternating", np.where(np.arange(B) % 2, 32767, -32768))
    for n in sorted({n for n in IMPULSES + (L - 1,) if n < B}):
        v = np.zeros(B)
        v[n] = 1
        add(f"impulse{n}", v)
    add("dc25000", np.clip(np.round(25000 + 3 * rng.standard_normal(B)), -32768, 32767))
    add("silence", np.zeros(B))
    for b in range(ND):
        pos = dig_comp[b] > 0
        add(f"digit{b}_neg", np.where(pos, -32768, 32767))  # tiled over the block by np.resize
        add(f"digit{b}_pos", np.where(pos, 32767, -32768))
    return names, np.array(rows).astype(np.int16)
