// Host-side plan of the rational resampler (resamp.hip): parameter validation, the output-count and
// branch / offset arithmetic, the tile geometry, the LDS layouts, the lane map, the summation order and
// the rounding chain.  The tuning fraction, r(n), the phase tables and the LDS budgets are ddc_plan.h's.
// No HIP: resamp.hip compiles it, and so does resamp_check.cpp with g++ under the sanitizers.
//
// The operation (include/msdsp.h): L = up, M = down, c = (ntaps - 1) / 2.  Output m: t = m M + c,
// phi = t mod L, n0 = t div L, v[m] = sum_{i < I_phi} h[phi + i L] z[n0 - i], I_phi = ceil((ntaps - phi) / L)
// (0 where phi >= ntaps), z = x (REAL) or x[n] e^{-2 pi i r(n) / q} (SSB), y[m] = gain v[m] (REAL) or
// gain Re(i^m v[m]) (SSB).
//
// Summation order of one output, a function of (ntaps, L, M) and the output's branch phi alone:
// I = ceil(ntaps / L) is the longest branch; the index i of a branch is cut into G contiguous groups of
// K = ceil(I / G); group g is one FMA chain from +0.0 over i = g K .. min((g + 1) K, I_phi) - 1 in ascending
// i (empty: +0.0); the G partial sums are added in ascending group order, p0 + p1, + p2, ...  No padded
// tap takes part: a branch stops at its own I_phi, so the result for non-finite samples is the plain
// IEEE value of the definition's sum.  G = THREADS / TM, and TM (outputs per tile) is the largest power of
// two whose tile fits the LDS budget at the SSB element size, whatever the plan's mode.  A zero sample
// adds +-0 to a chain that started at +0.0, which leaves it as it is: a sample outside what a row or a
// stream has seen and a zero inside it give the same bits.
//
// LDS of a tile of outputs m0 .. m0 + nout - 1:
//   samples  linear: staged sample j has global index nb + j, nb = n0(m0) - (I - 1), slot j; at most
//            SMAX = ceil((TM - 1) M / L) + I of them; SSB keeps two planes, Re z and Im z, and output m
//            reads one of them only (Re(i^m v) is +Re v, -Im v, -Re v, +Im v for m mod 4 = 0, 1, 2, 3).
//            Output m0 + o reads slot (I - 1) + dn(o) - i, dn(o) = (phi0 + o M) div L, phi0 = (m0 M + c) mod L.
//   taps     branch-minor, [i][phi] at i L + phi, which is h's own order (k = phi + i L), zero up to I L.
//   partial sums  [G][TM].
// Lane map: thread t of a group computes output o(t) = (t mod A) B + t div A, A = TM / B, B a power of two.
// A half-wave (32 lanes, one LDS cycle of a 64-bit read when their doubles lie on 32 distinct banks or
// coincide) thereby reads sample slots about B M / L apart.  B is the power of two with the fewest modelled
// extra LDS cycles (samples and taps, over the tile phases phi0), ties to the smaller: lane_map().  The map
// decides which lane computes an output, never how.
#pragma once

#include "ddc_plan.h"

namespace msd {
namespace resamp {

using ddc::THREADS;
constexpr int MAX_UP = 256;
constexpr int MAX_DOWN = 1024;
constexpr int64_t MAX_POS = (int64_t)1 << 62;  // (pos0 + n) up may not exceed it

struct Plan {
    int mode = 0, L = 0, M = 0, ntaps = 0, c = 0, out_i16 = 0;
    int q = 1, p = 0, two = 0, step = 0;  // the tuning fraction and the phase step, as in ddc::Plan
    int I = 0;                            // taps of the longest branch
    int TM = 0, G = 0, K = 0;             // outputs per tile, groups, taps of a branch per group
    int B = 1;                            // the lane map
    int smax = 0, plane = 0, tapn = 0;    // staged samples at most, doubles per plane (even), I L
    size_t lds_bytes = 0;
    double gain = 1.0;
};

// the configuration's shared part as the down-converter's, so that one validation serves both
inline msd_ddc_cfg as_ddc(const msd_resamp_cfg *c) {
    msd_ddc_cfg d{};
    d.mode = c->mode, d.decim = 1, d.ntaps = c->ntaps, d.out_dtype = c->out_dtype;
    d.shift_num = c->shift_num, d.shift_den = c->shift_den, d.gain = c->gain;
    return d;
}

// MSD_OK, or the code with *msg set
inline int validate(const msd_resamp_cfg *c, const char **msg) {
    auto bad = [&](int code, const char *m) {
        if (msg) *msg = m;
        return code;
    };
    if (!c) return bad(MSD_ERR_INVALID, "null configuration");
    if (c->up < 1 || c->up > MAX_UP) return bad(MSD_ERR_UNSUPPORTED, "up outside 1 .. 256");
    if (c->down < 1 || c->down > MAX_DOWN) return bad(MSD_ERR_UNSUPPORTED, "down outside 1 .. 1024");
    const msd_ddc_cfg d = as_ddc(c);
    if (int rc = ddc::validate(&d, msg)) return rc;
    if (ddc::gcd64(c->up, c->down) != 1) return bad(MSD_ERR_INVALID, "up and down must be coprime");
    return MSD_OK;
}

inline int staged_max(int L, int M, int ntaps, int tm) {
    const int I = (ntaps + L - 1) / L;
    return (int)(((int64_t)(tm - 1) * M + L - 1) / L) + I;
}
inline size_t tile_bytes(int L, int M, int ntaps, int tm) {
    const int I = (ntaps + L - 1) / L;
    const size_t plane = ((size_t)staged_max(L, M, ntaps, tm) + 1) & ~(size_t)1;
    return sizeof(double) * (2 * plane + (size_t)I * L + THREADS);
}
// outputs per tile: by (L, M, ntaps) alone
inline int tile_outputs(int L, int M, int ntaps) {
    for (int tm = THREADS; tm >= 1; tm >>= 1)
        if (tile_bytes(L, M, ntaps, tm) <= ddc::LDS_PREFERRED) return tm;
    for (int tm = THREADS; tm >= 1; tm >>= 1)
        if (tile_bytes(L, M, ntaps, tm) <= ddc::LDS_MAX) return tm;
    return 0;
}

// taps of branch phi
inline int branch_len(int ntaps, int L, int phi) { return phi < ntaps ? (ntaps - phi + L - 1) / L : 0; }
// output o of a tile whose first output has phi0 = (m0 M + c) mod L: its branch and dn = n0(m0 + o) - n0(m0)
inline void branch_of(int L, int M, int phi0, int o, int &phi, int &dn) {
    const int t = phi0 + o * M;  // below 256 + 255 * 1024
    phi = t % L;
    dn = t / L;
}
inline int lane_output(int t, int TM, int B) {
    const int A = TM / B;
    return (t % A) * B + t / A;
}

// extra LDS cycles (MI355X: a 64-bit read goes in two half-waves of 32 lanes; a half-wave takes one cycle
// more for every further distinct double on its busiest pair of banks) of the first wave's sample and tap
// reads at one i, summed over up to 16 tile phases phi0
inline int lane_map_cost(int L, int M, int ntaps, int TM, int B, int *samples = nullptr, int *taps = nullptr) {
    const int lanes = TM < 64 ? TM : 64;
    int cs = 0, ct = 0;
    const int nph = L < 16 ? L : 16;
    for (int s = 0; s < nph; ++s) {
        const int phi0 = (int)((int64_t)s * L / nph);
        for (int h0 = 0; h0 < lanes; h0 += 32) {
            int seen_s[32][33], seen_t[32][33], ns[32] = {0}, nt[32] = {0};
            for (int t = h0; t < h0 + 32 && t < lanes; ++t) {
                int phi, dn;
                branch_of(L, M, phi0, lane_output(t, TM, B), phi, dn);
                if (branch_len(ntaps, L, phi) == 0) continue;  // (the lane reads nothing)
                auto put = [](int (*seen)[33], int *n, int a) {
                    const int b = a & 31;
                    for (int k = 0; k < n[b]; ++k)
                        if (seen[b][k] == a) return;
                    seen[b][n[b]++] = a;
                };
                put(seen_s, ns, dn);
                put(seen_t, nt, phi);
            }
            int ms = 1, mt = 1;
            for (int b = 0; b < 32; ++b) ms = ns[b] > ms ? ns[b] : ms, mt = nt[b] > mt ? nt[b] : mt;
            cs += ms - 1, ct += mt - 1;
        }
    }
    if (samples) *samples = cs;
    if (taps) *taps = ct;
    return cs + ct;
}
inline int lane_map(int L, int M, int ntaps, int TM) {
    int best = 1, cost = lane_map_cost(L, M, ntaps, TM, 1);
    for (int B = 2; B <= TM && cost > 0; B <<= 1) {
        const int cb = lane_map_cost(L, M, ntaps, TM, B);
        if (cb < cost) best = B, cost = cb;
    }
    return best;
}

inline int make_plan(const msd_resamp_cfg *c, Plan &P, const char **msg) {
    if (int rc = validate(c, msg)) return rc;
    P = Plan{};
    P.mode = c->mode;
    P.L = c->up, P.M = c->down;
    P.ntaps = c->ntaps;
    P.c = (c->ntaps - 1) / 2;
    P.out_i16 = c->out_dtype == MSD_I16;
    const int64_t g = ddc::gcd64(c->shift_num, c->shift_den);
    P.q = (int)(c->shift_den / g);
    P.p = (int)(c->shift_num / g);
    P.two = P.q > ddc::TABLE_MAX;
    P.step = (int)(((int64_t)THREADS * P.p) % P.q);
    P.gain = c->gain;
    P.I = (P.ntaps + P.L - 1) / P.L;
    P.TM = tile_outputs(P.L, P.M, P.ntaps);
    if (P.TM < 1) {
        if (msg) *msg = "tile does not fit the LDS";
        return MSD_ERR_UNSUPPORTED;
    }
    P.G = THREADS / P.TM;
    P.K = (P.I + P.G - 1) / P.G;
    P.B = lane_map(P.L, P.M, P.ntaps, P.TM);
    P.smax = staged_max(P.L, P.M, P.ntaps, P.TM);
    P.plane = (P.smax + 1) & ~1;
    P.tapn = P.I * P.L;
    P.lds_bytes = tile_bytes(P.L, P.M, P.ntaps, P.TM);
    return MSD_OK;
}

// the phase tables of the plan's tuning fraction: ddc_plan.h's
inline void tables(const Plan &P, std::vector<double> &t1, std::vector<double> &t2) {
    ddc::Plan D;
    D.q = P.q, D.p = P.p, D.two = P.two;
    ddc::tables(D, t1, t2);
}

// ceil(a L / M) for 0 <= a, a L <= 2^62 + 2^18
inline int64_t out_index(int64_t a, int L, int M) { return ddc::cdiv(a * L, M); }

// outputs of a row holding samples [pos0, pos0 + n): every m with pos0 L <= m M < (pos0 + n) L.  The
// products are formed only after pos0 + n <= 2^62 / up has been checked by division.
inline int out_len(const msd_resamp_cfg *c, int64_t pos0, int64_t n, int64_t *m0, int64_t *count, const char **msg) {
    if (int rc = validate(c, msg)) return rc;
    if (pos0 < 0 || n < 0 || pos0 > MAX_POS / c->up || n > MAX_POS / c->up - pos0) {
        if (msg) *msg = "pos0 and n must be non-negative and (pos0 + n) up at most 2^62";
        return MSD_ERR_INVALID;
    }
    const int64_t lo = out_index(pos0, c->up, c->down);
    if (m0) *m0 = lo;
    if (count) *count = out_index(pos0 + n, c->up, c->down) - lo;
    return MSD_OK;
}

// what a stream reset to `start` that holds samples up to `count` has emitted: [first, emitted); a push of
// n more emits up to stream_emitted(count + n), the flush up to out_index(count)
inline int64_t stream_emitted(int64_t start, int64_t count, int L, int M, int c) {
    const int64_t first = out_index(start, L, M);
    const int64_t e = ddc::cdiv(count * L - c, M);  // every m with m M + c < count L
    return e < first ? first : e;
}

// The longest rounding chain from a sample to an output, in units of u = 2^-53, so that
// |y - y_exact| <= chain u |gain| S_m, S_m = sum_i |h[phi + i L]| |x[n0 - i]|.  Counted from resamp_kernel by
// the rules of ddc::chain: the conversion is exact; the mix is 0 (REAL), 5 (one table) or 9 (two); K FMAs of
// the longest group chain; G - 1 adds of the partial sums; the gain product 1.  The output mixer i^m and the
// choice of the plane are exact.  At most 10 + I + (G - 1), since K <= I.
inline double chain(const Plan &P) {
    const double mix = P.mode == MSD_DDC_SSB ? (P.two ? 9.0 : 5.0) : 0.0;
    return mix + (double)P.K + (double)(P.G - 1) + 1.0;
}

}  // namespace resamp
}  // namespace msd
