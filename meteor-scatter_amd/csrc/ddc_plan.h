// Host-side plan of the decimating down-converter (ddc.hip): parameter validation, the reduced tuning
// fraction p / q, the exact phase index r(n) = (n p) mod q, the phase tables, the tile geometry and the
// polyphase layout of a tile's samples in LDS, the output-count arithmetic and the rounding chain.
// No HIP: ddc.hip compiles it, and so does ddc_check.cpp with g++ under the sanitizers.
//
// The operation (include/msdsp.h): v[m] = sum_k h[k] z[m D + c - k], c = (ntaps - 1) / 2, z = x (REAL) or
// x[n] e^{-2 pi i r(n) / q} (SSB), y[m] = gain v[m] (REAL) or gain Re(i^m v[m]) (SSB).
//
// Summation order of one output, a function of (ntaps, D) alone: the taps are cut into G contiguous
// groups of K4 = ceil(ntaps / G); each group is one FMA chain from +0.0 in ascending k; the G partial
// sums are added in ascending group order, p0 + p1, + p2, ...  G = THREADS / TM, and TM (outputs per
// tile) is the largest power of two whose tile fits the LDS budget at the SSB element size, whatever the
// plan's mode.  A zero sample adds +-0 to a chain that started at +0.0, which leaves it as it is: a
// sample outside what a row or a stream has seen and a zero inside it give the same bits.
//
// LDS layout of a tile (S = TM D + ntaps - 1 samples, sample j at global index n0 + j): polyphase,
// slot(j) = (j mod D) U + j div D with U = ceil(S / D) made odd.  Output i reads j = i D + a for the tap
// a = ntaps - 1 - k: slot (a mod D) U + a div D + i, consecutive over the lanes' outputs (no bank
// conflict), and consecutive j are U slots apart when they are stored (U odd).  SSB keeps two planes,
// Re z and Im z; output m reads one of them only, since Re(i^m v) is +Re v, -Im v, -Re v, +Im v for
// m mod 4 = 0, 1, 2, 3.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/msdsp.h"

namespace msd {
namespace ddc {

constexpr int THREADS = 256;
constexpr int MAX_DECIM = 1024;
constexpr int MAX_TAPS = 4095;
constexpr int64_t MAX_Q = (int64_t)1 << 24;
constexpr int TABLE_BITS = 12;                 // q <= 2^12: one table; above, r = rh 2^12 + rl and two
constexpr int TABLE_MAX = 1 << TABLE_BITS;
constexpr size_t LDS_PREFERRED = 64 * 1024;    // a tile this small leaves room for two workgroups per CU
constexpr size_t LDS_MAX = 150 * 1024;

struct Plan {
    int mode = 0, D = 0, ntaps = 0, c = 0, out_i16 = 0;
    int q = 1, p = 0;      // the tuning fraction in lowest terms
    int two = 0;           // the phase factor is a product of two table entries
    int step = 0;          // (THREADS p) mod q: a thread's phase step from one staged sample to its next
    int TM = 0, G = 0, K4 = 0;  // outputs per tile, tap groups, taps per group
    int U = 0, plane = 0;       // polyphase layout: slots per branch, doubles per plane (even)
    size_t lds_bytes = 0;
    double gain = 1.0;
};

inline int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a < 0 ? -a : a;
}

// ceil(a / d) for d > 0 and any sign of a
inline int64_t cdiv(int64_t a, int64_t d) { return a >= 0 ? (a + d - 1) / d : -((-a) / d); }

// r(n) = (n p) mod q, exact for every int64 n: n is reduced first, so the product stays below 2^48
inline int64_t phase(int64_t n, int64_t p, int64_t q) {
    int64_t nm = n % q;
    if (nm < 0) nm += q;
    return (nm * p) % q;
}

// the doubles of one LDS plane and U for a tile of tm outputs
inline void layout(int D, int ntaps, int tm, int &U, int &plane) {
    const int64_t S = (int64_t)tm * D + ntaps - 1;
    U = (int)((S + D - 1) / D) | 1;
    plane = (D * U + 1) & ~1;
}
inline size_t tile_bytes(int D, int ntaps, int tm) {
    int U, plane;
    layout(D, ntaps, tm, U, plane);
    return sizeof(double) * (2 * (size_t)plane + THREADS);  // two planes and the groups' partial sums
}
// outputs per tile: by (D, ntaps) alone
inline int tile_outputs(int D, int ntaps) {
    for (int tm = THREADS; tm >= 1; tm >>= 1)
        if (tile_bytes(D, ntaps, tm) <= LDS_PREFERRED) return tm;
    for (int tm = THREADS; tm >= 1; tm >>= 1)
        if (tile_bytes(D, ntaps, tm) <= LDS_MAX) return tm;
    return 0;
}
inline int slot(int j, int D, int U) { return (j % D) * U + j / D; }

// MSD_OK, or the code with *msg set
inline int validate(const msd_ddc_cfg *c, const char **msg) {
    auto bad = [&](int code, const char *m) {
        if (msg) *msg = m;
        return code;
    };
    if (!c) return bad(MSD_ERR_INVALID, "null configuration");
    if (c->mode != MSD_DDC_REAL && c->mode != MSD_DDC_SSB) return bad(MSD_ERR_INVALID, "unknown mode");
    if (c->decim < 1 || c->decim > MAX_DECIM) return bad(MSD_ERR_UNSUPPORTED, "decim outside 1 .. 1024");
    if (c->ntaps < 1 || c->ntaps > MAX_TAPS) return bad(MSD_ERR_UNSUPPORTED, "ntaps outside 1 .. 4095");
    if (!(c->ntaps & 1)) return bad(MSD_ERR_INVALID, "ntaps must be odd");
    if (c->out_dtype != MSD_F64 && c->out_dtype != MSD_I16) return bad(MSD_ERR_INVALID, "out_dtype must be MSD_F64 or MSD_I16");
    if (c->shift_den < 1 || c->shift_num < 0 || c->shift_num >= c->shift_den)
        return bad(MSD_ERR_INVALID, "shift must satisfy 0 <= shift_num < shift_den");
    const int64_t g = gcd64(c->shift_num, c->shift_den);
    if (c->shift_den / g > MAX_Q) return bad(MSD_ERR_UNSUPPORTED, "reduced shift_den above 2^24");
    if (c->mode == MSD_DDC_REAL && c->shift_num != 0) return bad(MSD_ERR_UNSUPPORTED, "REAL mode takes no shift");
    if (!std::isfinite(c->gain)) return bad(MSD_ERR_INVALID, "gain must be finite");
    return MSD_OK;
}

// whether a sample dtype fits the mode
inline bool dtype_fits(int mode, int dtype) {
    return mode == MSD_DDC_SSB ? (dtype == MSD_CI16 || dtype == MSD_CF32) : (dtype == MSD_I16 || dtype == MSD_F32);
}
inline size_t elem_size(int dtype) {
    switch (dtype) {
        case MSD_I16: return 2;
        case MSD_F32: return 4;
        case MSD_CI16: return 4;
        case MSD_CF32: return 8;
        default: return 0;
    }
}

inline int make_plan(const msd_ddc_cfg *c, Plan &P, const char **msg) {
    if (int rc = validate(c, msg)) return rc;
    P = Plan{};
    P.mode = c->mode;
    P.D = c->decim;
    P.ntaps = c->ntaps;
    P.c = (c->ntaps - 1) / 2;
    P.out_i16 = c->out_dtype == MSD_I16;
    const int64_t g = gcd64(c->shift_num, c->shift_den);
    P.q = (int)(c->shift_den / g);
    P.p = (int)(c->shift_num / g);
    P.two = P.q > TABLE_MAX;
    P.step = (int)(((int64_t)THREADS * P.p) % P.q);
    P.gain = c->gain;
    P.TM = tile_outputs(P.D, P.ntaps);
    if (P.TM < 1) {
        if (msg) *msg = "tile does not fit the LDS";
        return MSD_ERR_UNSUPPORTED;
    }
    P.G = THREADS / P.TM;
    P.K4 = (P.ntaps + P.G - 1) / P.G;
    layout(P.D, P.ntaps, P.TM, P.U, P.plane);
    P.lds_bytes = tile_bytes(P.D, P.ntaps, P.TM);
    return MSD_OK;
}

// outputs of a row holding samples [pos0, pos0 + n): every m with pos0 <= m D < pos0 + n
inline int out_len(const msd_ddc_cfg *c, int64_t pos0, int64_t n, int64_t *m0, int64_t *count, const char **msg) {
    if (int rc = validate(c, msg)) return rc;
    if (pos0 < 0 || n < 0 || pos0 > INT64_MAX - n - MAX_DECIM) {
        if (msg) *msg = "pos0 and n must be non-negative and pos0 + n representable";
        return MSD_ERR_INVALID;
    }
    const int64_t lo = cdiv(pos0, c->decim);
    if (m0) *m0 = lo;
    if (count) *count = cdiv(pos0 + n, c->decim) - lo;
    return MSD_OK;
}

// (cos, -sin) of 2 pi r / q, 0 <= r < q: the angle is reduced exactly in integers to j quarter turns plus
// (pi / 2) num / q with |num| <= q / 2, evaluated in long double and rounded once to double.  Multiples of
// a quarter turn are exact.
inline void unit(int64_t r, int64_t q, double &wr, double &wi) {
    const int64_t j = (8 * r + q) / (2 * q);  // round(4 r / q), 0 .. 4
    const int64_t num = 4 * r - j * q;
    const long double a = (long double)num / (long double)q * 1.57079632679489661923132169163975144L;
    const long double ca = cosl(a), sa = num == 0 ? 0.0L : sinl(a);
    long double c, s;
    switch (j & 3) {
        case 0: c = ca, s = sa; break;
        case 1: c = -sa, s = ca; break;
        case 2: c = -ca, s = -sa; break;
        default: c = sa, s = -ca; break;
    }
    wr = (double)c;
    wi = (double)-s;
    if (wr == 0.0) wr = 0.0;  // no negative zeros in the tables
    if (wi == 0.0) wi = 0.0;
}

// the phase tables, interleaved (re, im): one table of q entries, t1[r] = e^{-2 pi i r / q}; or two,
// t1[rl] for rl < 2^12 and t2[rh] = e^{-2 pi i (rh 2^12 mod q) / q} for rh < ceil(q / 2^12): the factor of
// r = rh 2^12 + rl is t2[rh] t1[rl]
inline void tables(const Plan &P, std::vector<double> &t1, std::vector<double> &t2) {
    const int64_t q = P.q;
    const int64_t n1 = P.two ? TABLE_MAX : q;
    t1.assign(2 * (size_t)n1, 0.0);
    for (int64_t r = 0; r < n1; ++r) unit(r, q, t1[2 * (size_t)r], t1[2 * (size_t)r + 1]);
    t2.clear();
    if (!P.two) return;
    const int64_t n2 = (q + TABLE_MAX - 1) >> TABLE_BITS;
    t2.assign(2 * (size_t)n2, 0.0);
    for (int64_t rh = 0; rh < n2; ++rh) unit((rh << TABLE_BITS) % q, q, t2[2 * (size_t)rh], t2[2 * (size_t)rh + 1]);
}

// The longest rounding chain from a sample to an output, in units of u = 2^-53, so that
// |y - y_exact| <= chain u gain S_m, S_m = sum_k |h_k| |x_{m D + c - k}|.  Counted from ddc_kernel by the
// rules above IQ_CHAIN in stream.hip (an add or FMA 1, a complex multiply with FMA 2 sqrt 2, a rounded
// table entry sqrt 2 more): the conversion of a sample to float64 is exact; SSB mixes it by one complex
// multiply with a rounded factor, 2 sqrt 2 + sqrt 2 = 4.24, taken as 5; above 2^12 the factor is itself
// the product of two rounded entries, 2 sqrt 2 + 2 sqrt 2 = 5.66 on the factor, 8.49 with the mix, taken
// as 9; K4 FMAs of the group's chain; G - 1 adds of the partial sums; the gain product 1.  The output
// mixer i^m and the choice of the plane are exact.  The second-order terms, (chain u)^2 / 2 < 1e-12 of the
// bound, are inside the rounding up of the mix.
inline double chain(const Plan &P) {
    const double mix = P.mode == MSD_DDC_SSB ? (P.two ? 9.0 : 5.0) : 0.0;
    return mix + (double)P.K4 + (double)(P.G - 1) + 1.0;
}

}  // namespace ddc
}  // namespace msd
