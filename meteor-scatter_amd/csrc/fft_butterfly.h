// Radix-4 / radix-8 butterflies of the STFT kernels (stft1024.hip), in registers, natural order in
// and out.  Compiles for the device (hipcc) and for a plain host compiler, so the arithmetic can be
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
MSD_BFLY_FN float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }

MSD_BFLY_FN void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
    a0 = cadd(t0, t2);
    a1 = cadd(t1, t3);
    a2 = csub(t0, t2);
    a3 = csub(t1, t3);
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
