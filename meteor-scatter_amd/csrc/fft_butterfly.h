// Radix-4 / radix-8 / radix-16 butterflies of the STFT kernels (stft.hip, stft1024.hip, cstft.hip), in
// registers, natural order in and out.  Compiles for the device (hipcc) and for a plain host compiler, so the arithmetic can be
// checked on a CPU against a long-double DFT (butterfly_check.cpp).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSD_BFLY_FN __host__ __device__ __forceinline__
#define MSD_BFLY_UNROLL _Pragma("unroll")
#else
#define MSD_BFLY_FN inline
#define MSD_BFLY_UNROLL
struct float2 {
    float x, y;
};
inline float2 make_float2(float x, float y) { return float2{x, y}; }
#endif

namespace msd {
namespace bfly {

MSD_BFLY_FN float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
MSD_BFLY_FN float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
MSD_BFLY_FN float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
MSD_BFLY_FN float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)

MSD_BFLY_FN void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
    a0 = cadd(t0, t2);
    a1 = cadd(t1, t3);
    a2 = csub(t0, t2);
    a3 = csub(t1, t3);
}

// forward 16-point DFT, natural order in and out: n = n1 + 4 n2, k = k2 + 4 k1
MSD_BFLY_FN void dft16(float2 *v) {
    const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, h = 0.70710678118654752440f;
    MSD_BFLY_UNROLL
    for (int n1 = 0; n1 < 4; ++n1) dft4(v[n1], v[n1 + 4], v[n1 + 8], v[n1 + 12]);  // v[n1 + 4 k2]
    // twiddles W16^(n1 k2)
    v[5] = cmul(v[5], make_float2(c1, -s1));    // n1 1, k2 1: W^1
    v[9] = cmul(v[9], make_float2(h, -h));      // n1 1, k2 2: W^2
    v[13] = cmul(v[13], make_float2(s1, -c1));  // n1 1, k2 3: W^3
    v[6] = cmul(v[6], make_float2(h, -h));      // n1 2, k2 1: W^2
    v[10] = mul_mi(v[10]);                      // n1 2, k2 2: W^4 = -i
    v[14] = cmul(v[14], make_float2(-h, -h));   // n1 2, k2 3: W^6
    v[7] = cmul(v[7], make_float2(s1, -c1));    // n1 3, k2 1: W^3
    v[11] = cmul(v[11], make_float2(-h, -h));   // n1 3, k2 2: W^6
    v[15] = cmul(v[15], make_float2(-c1, s1));  // n1 3, k2 3: W^9
    MSD_BFLY_UNROLL
    for (int k2 = 0; k2 < 4; ++k2) dft4(v[4 * k2], v[4 * k2 + 1], v[4 * k2 + 2], v[4 * k2 + 3]);
    // v[4 k2 + k1] holds X[k2 + 4 k1]: reorder to natural
    float2 o[16];
    MSD_BFLY_UNROLL
    for (int k2 = 0; k2 < 4; ++k2)
        MSD_BFLY_UNROLL
        for (int k1 = 0; k1 < 4; ++k1) o[k2 + 4 * k1] = v[4 * k2 + k1];
    MSD_BFLY_UNROLL
    for (int i = 0; i < 16; ++i) v[i] = o[i];
}

// second half of a forward 8-point DFT: a_j = v_j + v_{j+4}, b_j = v_j - v_{j+4} given; s = sqrt(1/2)
// in a VGPR (vgpr_f: as an SGPR or literal operand its multiplies issue slower).
// The odd outputs are the DFT4 of (b0, s u1, -i b2, s u3) with the unscaled rotations u1 = (1 - i) b1 =
// (b1.x + b1.y, b1.y - b1.x) and u3 = (-1 - i) b3 = (b3.y - b3.x, -(b3.x + b3.y)).  The scaled terms only ever
// enter that DFT4's last stage as s (u1 + u3) and s (-i)(u1 - u3), so the four multiplies by s ride on
// the last stage's eight add / subs as FMAs: 12 add / sub + 8 FMA instead of 20 add / sub + 4 mul.
MSD_BFLY_FN void dft8_tail(float2 *v, float2 a0, float2 a1, float2 a2, float2 a3, float2 b0, float2 b1, float2 b2,
                           float2 b3, float s) {
    dft4(a0, a1, a2, a3);
    const float u1x = b1.x + b1.y, u1y = b1.y - b1.x;
    const float u3x = b3.y - b3.x, n3y = b3.x + b3.y;                      // u3 = (u3x, -n3y)
    const float2 p = make_float2(u1x + u3x, u1y - n3y);                     // u1 + u3
    const float2 m = make_float2(u1x - u3x, u1y + n3y);                     // u1 - u3
    const float2 t0 = make_float2(b0.x + b2.y, b0.y - b2.x);                // b0 + (-i b2)
    const float2 t1 = make_float2(b0.x - b2.y, b0.y + b2.x);                // b0 - (-i b2)
    v[0] = a0; v[2] = a1; v[4] = a2; v[6] = a3;
    v[1] = make_float2(__builtin_fmaf(s, p.x, t0.x), __builtin_fmaf(s, p.y, t0.y));    // t0 + s p
    v[3] = make_float2(__builtin_fmaf(s, m.y, t1.x), __builtin_fmaf(-s, m.x, t1.y));   // t1 + s (-i m)
    v[5] = make_float2(__builtin_fmaf(-s, p.x, t0.x), __builtin_fmaf(-s, p.y, t0.y));  // t0 - s p
    v[7] = make_float2(__builtin_fmaf(-s, m.y, t1.x), __builtin_fmaf(s, m.x, t1.y));   // t1 - s (-i m)
}

// in-place forward DFT of 8 points, natural order in and out
MSD_BFLY_FN void dft8(float2 *v, float s) {
    dft8_tail(v, cadd(v[0], v[4]), cadd(v[1], v[5]), cadd(v[2], v[6]), cadd(v[3], v[7]), csub(v[0], v[4]),
              csub(v[1], v[5]), csub(v[2], v[6]), csub(v[3], v[7]), s);
}

// dft8 of the windowed points d_j * w_j (componentwise), the window product of v_{j+4} shared
// by the first-stage sum and difference: 3 ops per component pair instead of 4
MSD_BFLY_FN void dft8_windowed(float2 *v, const float2 *d, const float2 *w, float s) {
    float2 a[4], b[4];
    MSD_BFLY_UNROLL
    for (int j = 0; j < 4; ++j) {
        const float px = d[j + 4].x * w[j + 4].x, py = d[j + 4].y * w[j + 4].y;
        a[j] = make_float2(__builtin_fmaf(d[j].x, w[j].x, px), __builtin_fmaf(d[j].y, w[j].y, py));
        b[j] = make_float2(__builtin_fmaf(d[j].x, w[j].x, -px), __builtin_fmaf(d[j].y, w[j].y, -py));
    }
    dft8_tail(v, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], s);
}

}  // namespace bfly
}  // namespace msd
