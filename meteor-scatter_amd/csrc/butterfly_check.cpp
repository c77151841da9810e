// CPU check of the STFT kernels' radix-8 butterflies (fft_butterfly.h, the header stft1024.hip
// compiles): dft8 and dft8_windowed against a long-double 8-point DFT on random inputs and the unit
// vectors.  Every output must lie within 4 float ulp of the input's norm (the norm of the windowed
// points for dft8_windowed), an ulp taken as the relative spacing 2^-23 times the norm: rounding
// errors scale with the norm itself, while the spacing of floats at the norm is a step function
// that drops to 2^-24 of it just above a power of two.  Against that step the four-rounding sum
// path of any float radix-2 DFT8 (worst case about 5 x 2^-23 of the norm) passes 4 only on
// average: about 5 outputs in a million, in the a-half and the b-half, before and after the FMA
// fold alike, reach 4 to 5 spacings.  The worst error in spacings is printed beside the bound's.
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

// forward DFT of z[0..7] in long double
void dft8_ref(const long double (*z)[2], long double (*o)[2]) {
    const long double tau = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < 8; ++k) {
        long double re = 0, im = 0;
        for (int j = 0; j < 8; ++j) {
            const int q = (j * k) & 7;  // exact angle reduction
            const long double c = cosl(tau * q / 8), s = -sinl(tau * q / 8);
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

void compare(const char *what, const float2 *got, const long double (*z)[2], Worst &w) {
    long double o[8][2], n2 = 0;
    dft8_ref(z, o);
    for (int j = 0; j < 8; ++j) n2 += z[j][0] * z[j][0] + z[j][1] * z[j][1];
    const double u = ulp_of(sqrtl(n2)), sp = spacing_of(sqrtl(n2));
    for (int k = 0; k < 8; ++k) {
        const double ex = fabs((double)((long double)got[k].x - o[k][0]));
        const double ey = fabs((double)((long double)got[k].y - o[k][1]));
        const double e = ex > ey ? ex : ey;
        if (u == 0.0 ? e != 0.0 : e > 4.0 * u) {
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
    compare("dft8", v, z, w_plain);
    for (int j = 0; j < 8; ++j) {
        z[j][0] = (long double)d[j].x * win[j].x;
        z[j][1] = (long double)d[j].y * win[j].y;
    }
    msd::bfly::dft8_windowed(v, d, win, s);
    compare("dft8_windowed", v, z, w_win);
}

}  // namespace

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 10000;
    const unsigned seed = argc > 2 ? (unsigned)atol(argv[2]) : 1u;
    const float s = 0.70710678118654752440f;
    std::mt19937 rng(seed);
    std::normal_distribution<float> g(0.f, 1.f);
    std::uniform_real_distribution<float> u01(0.f, 1.f);
    Worst wp, ww;
    float2 d[8], win[8];
    for (long i = 0; i < n; ++i) {
        // sample-like magnitudes over the int16 range, with and without a common offset
        const float amp = std::ldexp(1.f, (int)(i % 16)), dc = (i & 16) ? amp * g(rng) : 0.f;
        for (int j = 0; j < 8; ++j) {
            d[j] = make_float2(dc + amp * g(rng), dc + amp * g(rng));
            win[j] = make_float2(u01(rng), u01(rng));
        }
        check(d, win, s, wp, ww);
    }
    for (int j = 0; j < 8; ++j)
        for (int c = 0; c < 2; ++c) {  // the unit vectors e_j and i e_j, unit window
            for (int r = 0; r < 8; ++r) {
                d[r] = make_float2(0.f, 0.f);
                win[r] = make_float2(1.f, 1.f);
            }
            (c ? d[j].y : d[j].x) = 1.f;
            check(d, win, s, wp, ww);
        }
    if (wp.fails || ww.fails) {
        printf("FAIL dft8 %ld dft8_windowed %ld outputs past 4 ulp of the input norm\n", wp.fails, ww.fails);
        return 1;
    }
    printf("ok %ld random + 16 unit inputs: worst error dft8 %.3f, dft8_windowed %.3f ulp of the input norm "
           "(%.3f, %.3f float spacings at the norm)\n", n, wp.ulps, ww.ulps, wp.spacings, ww.spacings);
    return 0;
}
