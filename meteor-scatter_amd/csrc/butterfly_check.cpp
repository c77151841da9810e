// CPU check of the STFT kernels' butterflies (fft_butterfly.h, the header stft.hip, stft1024.hip and
// cstft.hip compile): dft8 and dft8_windowed against a long-double 8-point DFT on random inputs and
// the unit vectors, dft4 and dft16 likewise against the 4- and 16-point DFT.  Every output must lie within 4 float ulp of the input's norm (the norm of the windowed
// points for dft8_windowed), an ulp taken as the relative spacing 2^-23 times the norm: rounding
// errors scale with the norm itself, while the spacing of floats at the norm is a step function
// that drops to 2^-24 of it just above a power of two.  Against that step the four-rounding sum
// path of any float radix-2 DFT8 (worst case about 5 x 2^-23 of the norm) passes 4 only on
// average: about 5 outputs in a million, in the a-half and the b-half, before and after the FMA
// fold alike, reach 4 to 5 spacings.  The worst error in spacings is printed beside the bound's.
//
// dft4 and dft16 are held to bounds counted from their roundings.  An output component is a sum of
// input components x_c times twiddle components t_c (|t_c| <= 1); if every path from an input to the
// output passes at most m roundings, each a factor (1 + d), |d| <= u = 2^-24, the error is at most
// ((1 + u)^m - 1) sum_c |x_c t_c|, and sum_c |x_c t_c| <= sum_j |x_j| <= sqrt(n) ||x|| for n points
// (|re cos| + |im sin| <= |x_j|).  In ulp of the norm (2 u ||x||) that is m sqrt(n) / 2 to first order:
//   dft4:  m = 2 (two add levels; the rotation by -i is exact), n = 4:   2 ulp;
//   dft16: m = 7 along the longest path -- the first radix-4 stage 2, the twiddle product 3 (the
//          constant's own rounding to float, the product, the sum of the two products), the second
//          radix-4 stage 2 --, n = 16:                                    14 ulp.
// The assertion allows (1 + 2^-20) times these for the higher-order terms of (1 + u)^m.  A build that
// contracts the twiddle product into an FMA (the device's) drops one rounding and stays inside.  The
// measured worst error is printed beside each bound (10^6 random inputs, seed 1: dft4 1.600 of 2,
// dft16 3.607 of 14).
// No HIP.  `make -C meteor-scatter_amd/csrc butterfly` builds
// build/butterfly_check_san with g++ -fsanitize=address,undefined.
//   butterfly_check [N [SEED]]     N random inputs (default 10000); prints "ok ..." or "FAIL ..."
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "fft_butterfly.h"

namespace {

struct Worst {
    double ulps = 0;    // largest error seen, in ulp of the input norm
    double spacings = 0;  // the same in float spacings at the norm (printed, not asserted)
    long fails = 0;
};

// forward DFT of z[0..n) in long double (n a power of two)
void dft_ref(int n, const long double (*z)[2], long double (*o)[2]) {
    const long double tau = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < n; ++k) {
        long double re = 0, im = 0;
        for (int j = 0; j < n; ++j) {
            const int q = (j * k) & (n - 1);  // exact angle reduction
            const long double c = cosl(tau * q / n), s = -sinl(tau * q / n);
            re += z[j][0] * c - z[j][1] * s;
            im += z[j][0] * s + z[j][1] * c;
        }
        o[k][0] = re;
        o[k][1] = im;
    }
}

// float ulp of a norm x: 2^-23 x
double ulp_of(long double x) { return (double)x * ldexp(1.0, -23); }

// the spacing of floats at x's magnitude
double spacing_of(long double x) {
    const float f = (float)x;
    if (f == 0.f) return 0.0;
    int e;
    frexpf(f, &e);  // f = m 2^e, 0.5 <= m < 1
    return ldexp(1.0, e - 24);
}

// the n outputs `got` against the DFT of z, each within `bound` ulp of z's norm
void compare(const char *what, int n, double bound, const float2 *got, const long double (*z)[2], Worst &w) {
    long double o[16][2], n2 = 0;
    dft_ref(n, z, o);
    for (int j = 0; j < n; ++j) n2 += z[j][0] * z[j][0] + z[j][1] * z[j][1];
    const double u = ulp_of(sqrtl(n2)), sp = spacing_of(sqrtl(n2));
    for (int k = 0; k < n; ++k) {
        const double ex = fabs((double)((long double)got[k].x - o[k][0]));
        const double ey = fabs((double)((long double)got[k].y - o[k][1]));
        const double e = ex > ey ? ex : ey;
        if (u == 0.0 ? e != 0.0 : e > bound * u) {
            if (w.fails++ < 5) fprintf(stderr, "FAIL %s: output %d off by %.3g (ulp of the norm %.3g)\n", what, k, e, u);
        } else if (u != 0.0 && e / u > w.ulps) {
            w.ulps = e / u;
        }
        if (sp != 0.0 && e / sp > w.spacings) w.spacings = e / sp;
    }
}

void check(const float2 *d, const float2 *win, float s, Worst &w_plain, Worst &w_win) {
    long double z[8][2];
    float2 v[8];
    for (int j = 0; j < 8; ++j) {
        v[j] = d[j];
        z[j][0] = d[j].x;
        z[j][1] = d[j].y;
    }
    msd::bfly::dft8(v, s);
    compare("dft8", 8, 4.0, v, z, w_plain);
    for (int j = 0; j < 8; ++j) {
        z[j][0] = (long double)d[j].x * win[j].x;
        z[j][1] = (long double)d[j].y * win[j].y;
    }
    msd::bfly::dft8_windowed(v, d, win, s);
    compare("dft8_windowed", 8, 4.0, v, z, w_win);
}

constexpr double HIGHER_ORDER = 1.0 + 0x1p-20;  // (1 + u)^m - 1 against m u
constexpr double DFT4_BOUND = 2.0, DFT16_BOUND = 14.0;

// dft4 of d[0..3] and dft16 of d[0..15]
void check_4_16(const float2 *d, Worst &w4, Worst &w16) {
    long double z[16][2];
    float2 v[16];
    for (int j = 0; j < 16; ++j) {
        v[j] = d[j];
        z[j][0] = d[j].x;
        z[j][1] = d[j].y;
    }
    msd::bfly::dft4(v[0], v[1], v[2], v[3]);
    compare("dft4", 4, DFT4_BOUND * HIGHER_ORDER, v, z, w4);
    for (int j = 0; j < 16; ++j) v[j] = d[j];
    msd::bfly::dft16(v);
    compare("dft16", 16, DFT16_BOUND * HIGHER_ORDER, v, z, w16);
}

}  // namespace

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 10000;
    const unsigned seed = argc > 2 ? (unsigned)atol(argv[2]) : 1u;
    const float s = 0.70710678118654752440f;
    std::mt19937 rng(seed);
    std::normal_distribution<float> g(0.f, 1.f);
    std::uniform_real_distribution<float> u01(0.f, 1.f);
    // points 8..15 (dft16) from a generator and distribution of their own: dft8's inputs stay as they were
    std::mt19937 rng2(seed + 0x9e3779b9u);
    std::normal_distribution<float> g2(0.f, 1.f);
    Worst wp, ww, w4, w16;
    float2 d[16], win[8];
    for (long i = 0; i < n; ++i) {
        // sample-like magnitudes over the int16 range, with and without a common offset
        const float amp = std::ldexp(1.f, (int)(i % 16)), dc = (i & 16) ? amp * g(rng) : 0.f;
        for (int j = 0; j < 8; ++j) {
            d[j] = make_float2(dc + amp * g(rng), dc + amp * g(rng));
            win[j] = make_float2(u01(rng), u01(rng));
        }
        for (int j = 8; j < 16; ++j) d[j] = make_float2(dc + amp * g2(rng2), dc + amp * g2(rng2));
        check(d, win, s, wp, ww);
        check_4_16(d, w4, w16);
    }
    for (int j = 0; j < 16; ++j)
        for (int c = 0; c < 2; ++c) {  // the unit vectors e_j and i e_j, unit window
            for (int r = 0; r < 16; ++r) d[r] = make_float2(0.f, 0.f);
            for (int r = 0; r < 8; ++r) win[r] = make_float2(1.f, 1.f);
            (c ? d[j].y : d[j].x) = 1.f;
            if (j < 8) check(d, win, s, wp, ww);
            check_4_16(d, w4, w16);
        }
    if (wp.fails || ww.fails) {
        printf("FAIL dft8 %ld dft8_windowed %ld outputs past 4 ulp of the input norm\n", wp.fails, ww.fails);
        return 1;
    }
    if (w4.fails || w16.fails) {
        printf("FAIL dft4 %ld outputs past %g, dft16 %ld past %g ulp of the input norm\n", w4.fails, DFT4_BOUND,
               w16.fails, DFT16_BOUND);
        return 1;
    }
    printf("ok %ld random + 16 unit inputs: worst error dft8 %.3f, dft8_windowed %.3f ulp of the input norm "
           "(%.3f, %.3f float spacings at the norm)\n", n, wp.ulps, ww.ulps, wp.spacings, ww.spacings);
    printf("ok %ld random + 32 unit inputs: worst error dft4 %.3f (bound %g), dft16 %.3f (bound %g) ulp of the input "
           "norm\n", n, w4.ulps, DFT4_BOUND, w16.ulps, DFT16_BOUND);
    return 0;
}
