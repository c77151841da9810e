// Planning and arithmetic of the pruned real transform behind welch_fft.hip (the whole-band Welch
// row): which sub-transform owns which bin, the modulation indices, the pass schedule and the
// float64 butterflies.  Compiles for the device (hipcc) and for a plain host compiler, so the same
// plan runs on a CPU against a long-double DFT (welch_fft_check.cpp).
//
// The nperseg windowed values v[n] are followed by nfft - nperseg zeros.  With Lp a power of two,
// R = nfft / Lp and k = r + R q,
//     X[r + R q] = sum_n v[n] W_nfft^{n (r + R q)} = sum_{n < Lp} y_r[n] W_Lp^{n q},
//     y_r[n]     = sum_j v[n + j Lp] W_nfft^{(n + j Lp) r}:
// bin r + R q is bin q of an Lp-point transform of the modulated (and, where nperseg > Lp, folded)
// input.  Lp = min(nperseg rounded up to a power of two, nfft / 2), at least 2:
//   * nperseg <= nfft / 2: one term, j = 0 -- no pass ever touches the zero padding;
//   * nperseg >  nfft / 2 (nothing to prune): Lp = nfft / 2, R = 2, two terms, and the second one's
//     factor W_nfft^{Lp r} = (-1)^r is exact: y_r[n] = (v[n] +- v[n + Lp]) W_nfft^{n r}, which is the
//     first radix-2 step of a decimation in frequency.  R >= 2 always, so the widest transform is
//     8192 complex points (nfft 16384): one workgroup's LDS holds it.
// The input is real, X[nfft - k] = conj X[k], so the sub-transforms r = 0 .. R/2 give every bin of
// the one-sided spectrum exactly once:
//   r = 0:          bins R q,       q = 0 .. Lp/2         (the rest are their mirror images)
//   r = R/2:        bins R/2 + R q, q = 0 .. Lp/2 - 1
//   0 < r < R/2:    bins r + R q for q < Lp/2 and nfft - (r + R q) (residue R - r) for q >= Lp/2
// (Lp/2 + 1) + Lp/2 + (R/2 - 1) Lp = nfft/2 + 1.  At nperseg 256, nfft 4096: 9 modulated 256-point
// transforms, 4 radix-4 passes each, instead of 11 passes over 2048 packed points.
//
// Every sub-transform is a Stockham autosort FFT, natural order in and out: one radix-2 pass when
// log2 Lp is odd, then radix-4 passes.  The arithmetic is that of stft_any.hip's float64 Stockham
// pass; it is restated here on a plain struct because that file's pass is tied to one transform per
// workgroup and to the device's double2, and this header has to compile on the host.  One table
// W_nfft^j, j < nfft, serves the modulation and every pass (W_Lp^j = W_nfft^{R j}).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSD_WFFT_FN __host__ __device__ __forceinline__
#else
#define MSD_WFFT_FN inline
#endif

namespace msd {
namespace wfft {

struct alignas(16) cd {
    double x, y;
};

constexpr int MIN_NFFT = 16, MAX_NFFT = 16384;

struct Plan {
    int nperseg, nfft, K;  // K = nfft/2 + 1 bins
    int Lp, logLp, R;      // sub-transform length, R = nfft / Lp >= 2
    int nsub;              // sub-transforms r = 0 .. R/2
    int fold;              // nperseg > Lp: y_r[n] takes v[n + Lp] too (then R = 2)
    int npass;             // (logLp & 1) radix-2 + logLp / 2 radix-4
};

// false: a shape the transform does not take (nfft no power of two in [16, 16384], nperseg outside 1..nfft)
MSD_WFFT_FN bool make_plan(int nperseg, int nfft, Plan &P) {
    if (nfft < MIN_NFFT || nfft > MAX_NFFT || (nfft & (nfft - 1)) || nperseg < 1 || nperseg > nfft) return false;
    int Lp = 2, lg = 1;
    while (Lp < nperseg && Lp < nfft / 2) Lp *= 2, ++lg;
    P.nperseg = nperseg;
    P.nfft = nfft;
    P.K = nfft / 2 + 1;
    P.Lp = Lp;
    P.logLp = lg;
    P.R = nfft / Lp;
    P.nsub = P.R / 2 + 1;
    P.fold = nperseg > Lp;
    P.npass = (lg & 1) + lg / 2;
    return true;
}

// pass p's radix and the product Ns of the radices before it
MSD_WFFT_FN int pass_radix(const Plan &P, int p) { return (P.logLp & 1) && p == 0 ? 2 : 4; }
MSD_WFFT_FN int pass_ns(const Plan &P, int p) {
    if (p == 0) return 1;
    return (P.logLp & 1) ? 2 << (2 * (p - 1)) : 1 << (2 * p);
}

// the bin of the one-sided spectrum that output q of sub-transform r is, or -1 where another output owns it
MSD_WFFT_FN int owned_bin(const Plan &P, int r, int q) {
    if (r == 0 && q > P.Lp / 2) return -1;
    if (2 * r == P.R && q >= P.Lp / 2) return -1;
    const int k = r + P.R * q;
    return k <= P.nfft / 2 ? k : P.nfft - k;
}

// the inverse: the sub-transform r and its output q that own bin k (0 <= k <= nfft/2)
MSD_WFFT_FN void bin_source(const Plan &P, int k, int &r, int &q) {
    const int res = k & (P.R - 1);
    if (2 * res <= P.R) {
        r = res;
        q = (k - res) / P.R;
    } else {  // the mirror image nfft - k = r + R q lies in residue R - res
        r = P.R - res;
        q = (P.nfft - k - r) / P.R;
    }
}

// index into the table W_nfft^j of point n's modulation in sub-transform r
MSD_WFFT_FN int mod_index(const Plan &P, int r, int n) { return (n * r) & (P.nfft - 1); }

// y_r[n] from v[n] and v[n + Lp] (b: 0 unless the plan folds)
MSD_WFFT_FN cd modulated(const Plan &P, int r, double a, double b, cd w) {
    if (P.fold) a = (r & 1) ? a - b : a + b;  // W_nfft^{Lp r} = (-1)^r at R = 2
    return cd{a * w.x, a * w.y};
}

MSD_WFFT_FN cd cadd(cd a, cd b) { return cd{a.x + b.x, a.y + b.y}; }
MSD_WFFT_FN cd csub(cd a, cd b) { return cd{a.x - b.x, a.y - b.y}; }
MSD_WFFT_FN cd cmul(cd a, cd b) {
    return cd{__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x)};
}
MSD_WFFT_FN cd mul_mi(cd a) { return cd{a.y, -a.x}; }  // a * (-i)

// butterfly j (< Lp / RDX) of the pass with Ns: read, twiddle + radix, write
// (out[(j - k) RDX + k + q Ns] = sum over in[j + q Lp / RDX], k = j mod Ns)
template <int RDX>
MSD_WFFT_FN void bf_read(const cd *src, int Lp, int j, cd *v) {
    const int nbf = Lp / RDX;
    for (int q = 0; q < RDX; ++q) v[q] = src[j + q * nbf];
}
template <int RDX>
MSD_WFFT_FN void bf_compute(cd *v, const cd *W, int nfft, int Ns, int j) {
    if (Ns > 1) {
        const int k = j & (Ns - 1), step = nfft / (Ns * RDX);  // W_{Ns RDX}^{k q} = W_nfft^{k q step}
        for (int q = 1; q < RDX; ++q) v[q] = cmul(v[q], W[k * q * step]);
    }
    if (RDX == 4) {
        const cd t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), t3 = mul_mi(csub(v[1], v[3]));
        v[0] = cadd(t0, t2);
        v[1] = cadd(t1, t3);
        v[2] = csub(t0, t2);
        v[3] = csub(t1, t3);
    } else {
        const cd a = v[0];
        v[0] = cadd(a, v[1]);
        v[1] = csub(a, v[1]);
    }
}
template <int RDX>
MSD_WFFT_FN void bf_write(cd *dst, int Ns, int j, const cd *v) {
    const int k = j & (Ns - 1), o = (j - k) * RDX + k;
    for (int q = 0; q < RDX; ++q) dst[o + q * Ns] = v[q];
}
template <int RDX>
MSD_WFFT_FN void butterfly(const cd *src, cd *dst, const cd *W, int Lp, int nfft, int Ns, int j) {
    cd v[RDX];
    bf_read<RDX>(src, Lp, j, v);
    bf_compute<RDX>(v, W, nfft, Ns, j);
    bf_write<RDX>(dst, Ns, j, v);
}

// |X|^2 scale, doubled on the interior bins (scipy's onesided density)
MSD_WFFT_FN double bin_power(const Plan &P, int bin, cd X, double scale) {
    double p = (X.x * X.x + X.y * X.y) * scale;
    if (bin != 0 && bin != P.nfft / 2) p = p * 2.0;
    return p;
}

// W_n^j = exp(-2 pi i j / n), n a multiple of 8: the angle reduced to the first octant in integers, so
// that the axes are exact and the table has the symmetries of the roots
inline cd unit_root(int j, int n) {
    const long double tau = 6.283185307179586476925286766559005768L;
    j &= n - 1;
    const int quad = j / (n / 4), m = j - quad * (n / 4);
    long double c, s;
    if (m <= n / 8) {
        c = cosl(tau * m / n), s = sinl(tau * m / n);
    } else {
        c = sinl(tau * (n / 4 - m) / n), s = cosl(tau * (n / 4 - m) / n);
    }
    if (m == 0) c = 1, s = 0;
    cd w{(double)c, (double)-s};           // e^{-i t}
    for (int i = 0; i < quad; ++i) w = mul_mi(w);
    return w;
}
inline void unit_roots(int n, cd *W) {
    for (int j = 0; j < n; ++j) W[j] = unit_root(j, n);
}

}  // namespace wfft
}  // namespace msd
