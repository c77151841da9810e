// Host-side plan of the echo measurement (echo.hip): parameter validation, the span arithmetic the kernel and
// the host share, and a plain scalar restatement of one detection's record.  No HIP calls: echo.hip compiles
// it, and so does echo_check.cpp with g++ under the sanitizers.
//
// The contract is include/msdsp.h's (section "echo measurement").  In short, for detection i of a file with T
// frames, block size B, frame t covering samples [t hop, t hop + nperseg):
//   c(s)  = the lowest t >= 0 with t hop + nperseg / 2 >= s            (first frame centred at or after s)
//   a0    = min(T, c(start B)),  a1 = min(T, c(stop B))                (the core)
//   lo    = a1 of detection i - 1 (0 for i = 0),  hi = a0 of detection i + 1 (T for the last stored one)
//   t0    = max(a0 - pre, min(lo, a0), 0),  t1 = min(a1 + post, max(hi, a1), T)
// and per frame of [t0, t1), in float64 without contraction: S_t / N_t the band / noise-band column sums in
// ascending k from 0.0, k*_t the lowest row of the column maximum, delta_t its parabolic offset,
// r_t = (k*_t - k_lo) + delta_t.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/msdsp.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSD_ECHO_FN __host__ __device__ __forceinline__
#else
#define MSD_ECHO_FN inline
#endif

namespace msd {
namespace echo {

constexpr int MAX_BAND = MSD_ECHO_MAX_BAND;  // rows a lane walks per frame, signal or noise band
constexpr int WAVES = 4;                     // detections in flight per workgroup, one wave each
constexpr int THREADS = 64 * WAVES;
constexpr int MAX_GRID_Y = 8;                // workgroups per file: a wave strides over the file's slots
constexpr double INV_E = 0.36787944117144233;
static_assert(sizeof(msd_echo) == 128, "msd_echo is 128 bytes");
static_assert(sizeof(msd_echo_cfg) == 40, "msd_echo_cfg is 40 bytes");

inline int bad(const char **msg, int code, const char *m) {
    if (msg) *msg = m;
    return code;
}

// MSD_OK, or the code with *msg set
inline int validate(const msd_echo_cfg *c, int64_t K, const char **msg) {
    if (!c) return bad(msg, MSD_ERR_INVALID, "null configuration");
    if (K < 1 || K > 0x7fffffffLL) return bad(msg, MSD_ERR_INVALID, "need 1 <= K < 2^31");
    if (c->block_size < 1 || c->nperseg < 1 || c->hop < 1)
        return bad(msg, MSD_ERR_INVALID, "block_size, nperseg and hop must be >= 1");
    if (c->pre_frames < 0 || c->post_frames < 0) return bad(msg, MSD_ERR_INVALID, "negative padding");
    if (c->k_lo > c->k_hi || c->k_lo < 0 || c->k_hi >= K)
        return bad(msg, MSD_ERR_INVALID, "need 0 <= k_lo <= k_hi < K");
    if (c->n_lo <= c->n_hi && (c->n_lo < 0 || c->n_hi >= K))
        return bad(msg, MSD_ERR_INVALID, "noise band outside [0, K)");
    if ((int64_t)c->k_hi - c->k_lo + 1 > MAX_BAND || (int64_t)c->n_hi - c->n_lo + 1 > MAX_BAND)
        return bad(msg, MSD_ERR_UNSUPPORTED, "a band wider than MSD_ECHO_MAX_BAND rows");
    return MSD_OK;
}

// c(s): the first frame whose centre is at or after sample s
MSD_ECHO_FN int64_t first_frame_at(int64_t s, int64_t nperseg, int64_t hop) {
    const int64_t need = s - nperseg / 2;
    if (need <= 0) return 0;
    return need / hop + (need % hop != 0);
}

MSD_ECHO_FN int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
MSD_ECHO_FN int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

struct Span {
    int64_t a0, a1, t0, t1;
    int32_t flags;  // bits 0 and 1
};

// the core [a0, a1) of one detection
MSD_ECHO_FN void core_of(const msd_det &d, const msd_echo_cfg &c, int64_t T, int64_t *a0, int64_t *a1) {
    *a0 = min64(T, first_frame_at(d.start * c.block_size, c.nperseg, c.hop));
    *a1 = min64(T, first_frame_at(d.stop * c.block_size, c.nperseg, c.hop));
}

// the span of detection i among the m stored detections dets[0 .. m) of a file with T frames
MSD_ECHO_FN Span span_of(const msd_det *dets, int64_t i, int64_t m, const msd_echo_cfg &c, int64_t T) {
    Span s;
    core_of(dets[i], c, T, &s.a0, &s.a1);
    int64_t lo = 0, hi = T, x;
    if (i > 0) core_of(dets[i - 1], c, T, &x, &lo);
    if (i + 1 < m) core_of(dets[i + 1], c, T, &hi, &x);
    s.t0 = max64(max64(s.a0 - c.pre_frames, min64(lo, s.a0)), 0);
    s.t1 = min64(min64(s.a1 + c.post_frames, max64(hi, s.a1)), T);
    s.flags = (s.t0 > s.a0 - c.pre_frames ? 1 : 0) | (s.t1 < s.a1 + c.post_frames ? 2 : 0);
    return s;
}

// one frame's values
struct Column {
    double S, N, delta;
    int32_t k;
};

// column t of one file's spectrogram (rows ld apart); the band rows are read once for S and the maximum, the
// maximum's neighbours again for the parabola
template <typename T>
MSD_ECHO_FN double band_sum(const T *col, int64_t ld, int32_t lo, int32_t hi) {
    double s = 0.0;
    for (int32_t k = lo; k <= hi; ++k) s = s + (double)col[(int64_t)k * ld];
    return s;
}

template <typename T>
MSD_ECHO_FN Column column_of(const T *col, int64_t ld, int32_t K, const msd_echo_cfg &c) {
    Column o;
    double s = 0.0, best = (double)col[(int64_t)c.k_lo * ld];
    int32_t kb = c.k_lo;
    for (int32_t k = c.k_lo; k <= c.k_hi; ++k) {
        const double v = (double)col[(int64_t)k * ld];
        s = s + v;
        if (v > best) best = v, kb = k;
    }
    o.S = s, o.k = kb, o.delta = 0.0;
    if (kb > 0 && kb < K - 1) {
        const double a = (double)col[(int64_t)(kb - 1) * ld], cc = (double)col[(int64_t)(kb + 1) * ld];
        const double den = (a - 2.0 * best) + cc;
        if (den < 0) o.delta = (0.5 * (a - cc)) / den;
    }
    o.N = band_sum(col, ld, c.n_lo, c.n_hi);
    return o;
}

MSD_ECHO_FN double quiet_nan() {
    const uint64_t bits = 0x7ff8000000000000ull;
    double v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __builtin_bit_cast(double, bits);
#else
    std::memcpy(&v, &bits, sizeof v);
#endif
    return v;
}

// the record of an empty span
MSD_ECHO_FN msd_echo empty_record(const Span &s) {
    msd_echo e;
    e.t0 = s.t0, e.t1 = s.t1;
    e.t_peak = e.t_half_first = e.t_half_last = e.t_efold = s.t0;
    e.k_peak = -1, e.flags = s.flags;
    e.p_peak = e.n_peak = quiet_nan();
    e.d_peak = 0.0;
    e.e_sig = e.e_noise = e.w_r = e.w_u = e.w_uu = e.w_ur = 0.0;
    return e;
}

// Scalar restatement of one detection's record over one file's spectrogram spec[k ld + t] (the sums in
// ascending t; the kernel's order differs, within the header's bound).  Host only.
template <typename T>
inline msd_echo measure_one(const T *spec, int32_t K, int64_t frames, int64_t ld, const msd_det *dets, int64_t i,
                            int64_t m, const msd_echo_cfg &c) {
    const Span s = span_of(dets, i, m, c, frames);
    if (s.t1 <= s.t0) return empty_record(s);
    msd_echo e = empty_record(s);
    bool have = false;
    for (int64_t t = s.t0; t < s.t1; ++t) {
        const Column col = column_of(spec + t, ld, K, c);
        if (!have || col.S > e.p_peak)
            have = true, e.p_peak = col.S, e.t_peak = t, e.k_peak = col.k, e.d_peak = col.delta, e.n_peak = col.N;
        const double u = (double)(t - s.t0), r = (double)(col.k - c.k_lo) + col.delta, su = col.S * u;
        e.e_sig = e.e_sig + col.S;
        e.e_noise = e.e_noise + col.N;
        e.w_r = e.w_r + col.S * r;
        e.w_u = e.w_u + su;
        e.w_uu = e.w_uu + su * u;
        e.w_ur = e.w_ur + su * r;
    }
    const double half = 0.5 * e.p_peak, fold = e.p_peak * INV_E;
    e.t_half_first = e.t_half_last = e.t_peak;
    e.t_efold = s.t1;
    bool first = true;
    for (int64_t t = s.t0; t < s.t1; ++t) {
        const double S = band_sum(spec + t, ld, c.k_lo, c.k_hi);
        if (S >= half) {
            if (first) e.t_half_first = t, first = false;
            e.t_half_last = t;
        }
        if (t > e.t_peak && S <= fold && e.t_efold == s.t1) e.t_efold = t;
    }
    e.flags = s.flags | (e.t_efold == s.t1 ? 4 : 0) | (e.t_peak == s.t0 || e.t_peak == s.t1 - 1 ? 8 : 0);
    return e;
}

}  // namespace echo
}  // namespace msd
