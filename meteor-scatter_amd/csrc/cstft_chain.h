// Pass structure and rounding-chain constant of the complex (I/Q) spectrogram kernels: what
// cstft_any_kernel (cstft_any.hip) instantiates, what msd_cstft_chain reports and what the delta error
// bound of iq_band_delta_kernel (stream.hip) multiplies by u.  Host and device, no HIP needed.
#pragma once

#if defined(__HIPCC__)
#define MSD_CHAIN_FN __host__ __device__ constexpr
#else
#define MSD_CHAIN_FN constexpr
#endif

namespace msd {

constexpr int CSA_MIN_LOG2 = 4;   // nfft 16
constexpr int CSA_MAX_LOG2 = 13;  // nfft 8192: 8192 complex points + padding in one workgroup's LDS

// cstft_any_kernel at nfft = 2^L: one leading radix-2^(L mod 4) pass (none when L is a multiple of 4), then
// L / 4 radix-16 passes (fft_butterfly.h dft16).  Only the first pass of all runs without twiddles.
MSD_CHAIN_FN int csa_first_radix(int L) { return 1 << (L & 3); }
MSD_CHAIN_FN int csa_radix16_passes(int L) { return L >> 2; }

// log2 of nfft if it is a power of two the generic kernel runs, else -1
MSD_CHAIN_FN int csa_log2(int nfft) {
    for (int L = CSA_MIN_LOG2; L <= CSA_MAX_LOG2; ++L)
        if (nfft == (1 << L)) return L;
    return -1;
}

// The chain of cstft_any_kernel, counted by the rules above IQ_CHAIN in stream.hip: an add 1, a complex
// multiply with FMA 2 sqrt 2, a rounded twiddle sqrt 2 more (so a twiddle multiply 3 sqrt 2 = 4.2426);
// exact powers of two and -+i free; detrend, window and the window's rounding 3.  Longest path per pass:
//   radix 2    1 add                                                     1
//   radix 4    2 adds (dft4: -i is free)                                 2
//   radix 8    3 adds and one sqrt(1/2) rotation, taken as a full
//              twiddle multiply (dft8_tail folds it into FMAs)           3 + 4.2426 = 7.2426
//   radix 16   dft4, internal twiddle W16^m, dft4                        4 + 4.2426 = 8.2426
//   between two passes: one twiddle multiply                             4.2426
// chain = 3 + first pass + 8.2426 * (L / 4) + 4.2426 * (passes - 1), rounded up:
//   nfft    16    32    64   128   256   512  1024  2048  4096  8192
//   passes  16  2.16  4.16  8.16 16.16 2.16.16 4.16.16 8.16.16 16.16.16 2.16.16.16
//   sum  11.24 16.49 17.49 22.73 23.73 28.97 29.97 35.21 36.21 41.46
//   chain   12    17    18    23    24    29    30    36    37    42
// (4096: the same three radix-16 passes as cstft4096_kernel, the same 37.)
MSD_CHAIN_FN double cstft_any_chain(int L) {
    const double tw = 4.242640687119286;  // 3 sqrt 2, rounded up in the last place
    const int r0 = csa_first_radix(L), n16 = csa_radix16_passes(L);
    const double first = r0 == 2 ? 1.0 : r0 == 4 ? 2.0 : r0 == 8 ? 3.0 + tw : 0.0;
    const int passes = n16 + (r0 > 1 ? 1 : 0);
    const double sum = 3.0 + first + (4.0 + tw) * n16 + tw * (passes - 1);
    const int fl = (int)sum;
    return (double)fl < sum ? (double)(fl + 1) : (double)fl;
}

// cstft4096_kernel's own count (stream.hip, IQ_CHAIN)
constexpr double CSTFT4096_CHAIN = 37.0;

// the chain of the kernel that produces rows of N = nperseg = nfft floats; `generic`: MSD_OPT_GENERIC_CSTFT
// is set, so 4096 may come from either kernel (the larger count).  0 for a row length no kernel writes.
MSD_CHAIN_FN double cstft_row_chain(int N, bool generic) {
    const int L = csa_log2(N);
    if (L < 0) return 0.0;
    const double any = cstft_any_chain(L);
    if (N != 4096) return any;
    return generic && any > CSTFT4096_CHAIN ? any : CSTFT4096_CHAIN;
}

}  // namespace msd
