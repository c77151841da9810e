// The digit code the three int8-MFMA kernels share (block_i8.hip, refine_i8.hip, welch_i8.hip): an
// int16 sample is x = 256 h + l' + 128 with h = x >> 8 and l' = (x & 255) - 128 both int8, a real
// coefficient T is ND balanced base-256 digits in [-128, 127], and a lane's 16-byte fragment of a
// K step of 64 samples holds 8 samples at 8 g and 8 at 32 + 8 g (g = lane >> 4).  The device part
// splits the samples; the host part (plain C++: host_check.cpp compiles it with g++ under the
// sanitizers) computes the band kernels' integer coefficients (the plans' builders and msd_i8_coeffs
// share these functions, so a test restates the kernels from the very integers they run on), expands
// them into digits and maps fragment bytes to samples.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace msd {

#if defined(__HIPCC__)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// A fragments of one K step from the lane's 16 samples (w[0..7], two per dword): the high bytes
// h = x >> 8 and the low bytes l' = (x & 255) - 128 (offset-binary byte ^ 0x80), both as int8
__device__ __forceinline__ void digits(const uint32_t *w, v4i &hi, v4i &lo) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        hi[o] = (int)__builtin_amdgcn_perm(w[2 * o + 1], w[2 * o], 0x07050301u);
        lo[o] = (int)(__builtin_amdgcn_perm(w[2 * o + 1], w[2 * o], 0x06040200u) ^ 0x80808080u);
    }
}

// the same, also adding sum |h| over the 16 samples to habs
__device__ __forceinline__ void digits(const uint32_t *w, v4i &hi, v4i &lo, uint32_t &habs) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const uint32_t h = __builtin_amdgcn_perm(w[2 * o + 1], w[2 * o], 0x07050301u);
        const uint32_t l = __builtin_amdgcn_perm(w[2 * o + 1], w[2 * o], 0x06040200u) ^ 0x80808080u;
        hi[o] = (int)h;
        lo[o] = (int)l;
        // sum |h| over the 4 bytes: |h| = |(h ^ 0x80) - 0x80| on the offset-binary bytes
        habs = __builtin_amdgcn_sad_u8(h ^ 0x80808080u, 0x80808080u, habs);
    }
}
#endif

// one balanced base-256 digit expansion of T: T = sum_b d[b] 256^(ND - 1 - b), every digit in
// [-128, 127]; false if T does not fit the ND digits (a carry left over)
template <int ND>
inline bool balanced_digits(int64_t T, int8_t (&d)[ND]) {
    for (int b = ND - 1; b >= 0; --b) {
        int64_t r = ((T % 256) + 256) % 256;  // 0..255
        if (r >= 128) r -= 256;               // -128..127
        d[b] = (int8_t)r;
        T = (T - r) / 256;
    }
    return T == 0;
}

// T_n = round(v_n 2^53) with sum_n T_n = 0 exactly: floors, then the largest remainders rounded up
// (sum_n v_n = 0 up to long double rounding, so the count to round up lies in [0, L)); |T_n - v_n 2^53| < 1
inline bool zero_sum_round(const std::vector<long double> &v, std::vector<int64_t> &T) {
    const int L = (int)v.size();
    std::vector<long double> frac(L);
    std::vector<int> idx(L);
    int64_t S = 0;
    for (int n = 0; n < L; ++n) {
        const long double s = v[n] * 0x1p53L, f = floorl(s);
        T[n] = (int64_t)f;
        frac[n] = s - f;
        S += T[n];
        idx[n] = n;
    }
    const int64_t R = -S;
    if (R < 0 || R > L) return false;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return frac[a] > frac[b]; });
    for (int64_t r = 0; r < R; ++r) T[idx[r]] += 1;
    return true;
}

// cos and sin of 2 pi j / N for any integer j, for host-built twiddle tables: j is reduced mod N into
// [-N/2, N/2] in exact integer arithmetic, the angle and the functions are evaluated in long double
// (x86-64: 64-bit significand), so each value rounded to double is within ~0.5 ulp of the exact one.
// (A double angle 2 pi m / N up to 2 pi is itself off by up to ~2 pi u, several u of twiddle error.)
inline void unit_root_ld(int64_t j, int64_t N, long double &c, long double &s) {
    int64_t r = j % N;
    if (r < 0) r += N;
    if (2 * r > N) r -= N;
    const long double a = 6.283185307179586476925286766559005768L * (long double)r / (long double)N;
    c = cosl(a);
    s = sinl(a);
}

// block_i8.hip's integers of bin k: T_n = round(w_n cos(2 pi k n / nfft) 2^54) (part 0, the real
// part) or round(-w_n sin(...) 2^54) (part 1), n < L; the argument reduced exactly into [0, 2 pi),
// long double
inline void block_i8_coeffs(const double *window, int L, int nfft, int64_t k, int part, int64_t *T) {
    for (int n = 0; n < L; ++n) {
        const int64_t m = (k * n) % nfft;
        const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)nfft;
        const long double v = (long double)window[n] * (part ? -sinl(a) : cosl(a));
        T[n] = llroundl(v * 0x1p54L);
    }
}

// welch_i8.hip's integers of bin k: c'_n = w_n e^{-i theta n} - W_k / L (W_k = sum_n w_n e^{-i theta n},
// theta = 2 pi k / nfft, long double: the segment detrend folded in), its real (part 0) or
// imaginary part rounded to T_n ~ c'_n 2^53 with sum_n T_n = 0 (zero_sum_round); false if that
// rounding refuses
inline bool welch_i8_coeffs(const double *window, int L, int nfft, int64_t k, int part, int64_t *T) {
    long double Wre = 0.0L, Wim = 0.0L;
    std::vector<long double> cr(L), ci(L), cv(L);
    for (int n = 0; n < L; ++n) {
        long double cs, sn;
        unit_root_ld(k * n, nfft, cs, sn);
        cr[n] = (long double)window[n] * cs;
        ci[n] = -(long double)window[n] * sn;
        Wre += cr[n];
        Wim += ci[n];
    }
    const long double Wc = (part ? Wim : Wre) / (long double)L;
    for (int n = 0; n < L; ++n) cv[n] = (part ? ci[n] : cr[n]) - Wc;
    std::vector<int64_t> Tv(L);
    if (!zero_sum_round(cv, Tv)) return false;
    std::copy(Tv.begin(), Tv.end(), T);
    return true;
}

// refine_i8.hip's integers of bin k (0 <= k < nfft): T_n = round(cos(2 pi k n / nfft) 2^46) (part 0) or
// round(sin(...) 2^46) (part 1), n < L, from the long-double unit root whose argument was reduced
// exactly (unit_root_ld): |T_n 2^-46 - w_n| <= 2^-47 (1 + 2^-16), |T_n| <= 2^46 (six balanced digits).
// The kernel's columns take T^c, T^s and -T^s (re = I C + Q S, im = Q C - I S) at n < 256, the
// sample's place in its sub-block.
inline void refine_i8_coeffs(int L, int nfft, int64_t k, int part, int64_t *T) {
    for (int n = 0; n < L; ++n) {
        long double c, s;
        unit_root_ld(k * n, nfft, c, s);
        T[n] = (int64_t)llroundl(ldexpl(part ? s : c, 46));
    }
}

// the sample of a K dimension that byte j (< 16) of lane group g's (< 4) fragment of K step ks holds:
// the A fragments' load order, which the B fragments' builders follow
constexpr int frag_sample(int ks, int g, int j) { return 64 * ks + (j < 8 ? 8 * g + j : 32 + 8 * g + (j - 8)); }

}  // namespace msd
