// The float64 refinement's block step for int16 I/Q on the matrix cores (msd_iq_delta64_dev,
// refine.hip): the DFT of each D = 1024-sample block at the needed bins as an EXACT integer GEMM.
//
// Samples are integers, so the only rounding in sum_n x_n W^{k n} is the twiddles'.  Each real
// twiddle entry (cos, sin of 2 pi k m / N) is stored as T = round(w 2^46), |T| <= 2^46, written in
// six balanced base-256 digits d_0..d_5 in [-128, 127] (T = sum_b d_b 256^(5-b)); each int16 sample
// as x = 256 h + l' + 128 with h = x >> 8 and l' = (x & 255) - 128 both int8.  Then
//   sum_n x_n T_n = sum_b 256^(5-b) (256 sum_n h_n d_bn + sum_n l'_n d_bn + 128 sum_n d_bn)
// and every inner sum is a v_mfma_i32_16x16x64_i8 accumulation, exact in int32.  The only error
// against the true DFT is the twiddles' quantisation, |T 2^-46 - w| <= 2^-47 per real entry: the
// block's bin is off by at most sqrt 2 * 2^-47 * sum (|I| + |Q|) -- 90.5 u (u = 2^-53) against the
// float64 Goertzel's ~3 L / |sin theta| u (~6000 u at C5) -- before the float64 combination.
//
// GEMM shape per 16-row tile = four consecutive compact blocks of 1024 complex samples: row
// 4 b + s = sub-block s (256 samples) of block b, K = 512 (the sub-block's I, Q values interleaved
// as they sit in memory, 8 K steps of 64), columns = the needed bins' real and imaginary parts
// times the six digits, packed in NT tiles of 16 columns:
//   tiles 0..5: column c = component c (bin c >> 1, part c & 1) of bins 0..7, digit = tile;
//   tile 6 + e: bin 8 + e, part c >> 3, digit c & 7 (< 6); tile 6's columns 6, 7: ones on I, Q.
// A lane of the result (column c = lane & 15, rows 4 (lane >> 4) + r) thus holds, for block
// lane >> 4, all four sub-blocks and all six digits of its component (tiles 0..5) in its own
// registers: the sub-block partials combine with float64 twiddles W^{256 k s} without a
// cross-lane sum; the extra bins' digits spread over 8 lanes of the half-row (3 DPP adds).  With
// K = 512 the digit products reach 2^31 in the worst case, so 256 h_d + l_d is formed in float64
// (exact) rather than int32.  The output is refine.hip's bin-major block table (a tile's values
// staged in LDS, then one store instruction), which frame_kernel turns into frames, delta and ed.
//
// Tiles interleaved over the waves, one wave per SIMD (~370 VGPRs: two accumulator sets of 56 and
// two tiles of samples, 2 x 256 B per lane, in flight), software-pipelined: tile k's MFMAs run
// while tile k - 1's float64 reduction is interleaved slice by slice (1.98 -> 1.93 ms for the delta
// step against two waves per SIMD without it); the B fragments (NT x 8 KB), lane twiddles and
// column offsets sit in LDS.  Per block: 28 MFMAs (~850 cycles of the matrix core), 4 KB of
// samples from HBM, ~30 float64 VALU ops per lane.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "i8_digits.h"
#include "msd_internal.h"
#include "refine_plan.h"
#include "refine_i8.h"

namespace msd {
namespace {

constexpr int I8_ND = 6;     // twiddle digits
constexpr int I8_BPT = 4;    // blocks per 16-row tile
constexpr int I8_SB = 4;     // sub-blocks per block (rows of the tile per block)
constexpr int I8_SUB = 256;  // complex samples per sub-block
constexpr int I8_KS = 8;     // K steps of 64 int16 values per sub-block row (2 I8_SUB values)

__device__ __forceinline__ int find_range_i8(const int64_t *cs, int nr, int64_t g) {
    int lo = 0, hi = nr - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cs[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// int sums of lane l and lane l ^ 16 / l ^ 32 (v_permlane16/32_swap: VALU, no LDS round trip)
__device__ __forceinline__ int add_xor16_i(int v) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return (int)(r[0] + r[1]);
}
__device__ __forceinline__ int add_xor32_i(int v) {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)(r[0] + r[1]);
}

template <int NT>
struct Acc {
    v4i h[NT], l[NT];
};

// out (bin-major, refine.hip's block table): out[b * nblocks + g] = B_g[k_b] for b < nk, then the
// block's sample sum (b = nk) and an upper bound of sum (|re| + |im|) (b = nk + 1, .x)
//
// A wave takes every nwaves-th tile of four compact blocks (one 16-row tile; the chip sweeps the
// samples in order: 4 % faster than contiguous per-wave ranges); the next tile's samples are
// requested K step by K step as the current one's are turned into digits.
template <int NT>
__global__ __launch_bounds__(256, 1) void block_i8_kernel(const int16_t *__restrict__ x, int64_t D,
                                                          const int64_t *__restrict__ bstart,
                                                          const int64_t *__restrict__ bcs, int nr, int64_t nblocks,
                                                          int nk, const v4i *__restrict__ bfrag,
                                                          const int *__restrict__ colinit,
                                                          const double2 *__restrict__ ltw, double2 *__restrict__ out) {
    constexpr int NX = NT - 6;  // extra bins (8 + e), two components each, in tiles 6 ..
    __shared__ v4i sB[NT * I8_KS * 64];
    // per column: the lane twiddles (below) and the K offsets' column sums, read where used
    __shared__ double2 sTw[(1 + NX) * I8_SB * 16];
    __shared__ int sInit[NT * 16];
    // per wave: one tile's output rows (4 blocks x RW entries)
    constexpr int RW = 12;  // >= nk + 2 (nk <= 10)
    __shared__ double2 sOut[4][I8_BPT * RW];
    for (int i = threadIdx.x; i < NT * I8_KS * 64; i += 256) sB[i] = bfrag[i];
    for (int i = threadIdx.x; i < (1 + NX) * I8_SB * 16; i += 256) sTw[i] = ltw[i];
    for (int i = threadIdx.x; i < NT * 16; i += 256) sInit[i] = colinit[i];
    __syncthreads();
    const int l = threadIdx.x & 63;
    const int c = l & 15, grp = l >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv;
    // tiles interleaved over the waves (tile = wave + j * nwaves): the chip sweeps the samples in
    // order, a window of ~nwaves tiles at a time
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ntiles = (nblocks + I8_BPT - 1) / I8_BPT;
    if (wave >= ntiles) return;
    const int64_t g1 = nblocks;
    // sTw[(e * I8_SB + r) * 16 + c]: column c's sub-block twiddle W^{256 k r} (a lane's C rows r =
    // 0..3 are the 4 sub-blocks of block grp) for its component's bin, the imaginary part signed by
    // the component (re: +, im: -); e > 0: the same for extra bin 8 + e - 1
    auto tw = [&](int e, int r) { return sTw[(e * I8_SB + r) * 16 + c]; };
    const int ncomp = 2 * (nk < 8 ? nk : 8);
    const int dg = c & 7;  // extra tiles: this lane's digit (6, 7: the sum columns / zero)
    const double xscale = dg < 6 ? __builtin_ldexp(1.0, -6 - 8 * dg) : 0.0;
    // the lane's A row (l & 15) = sub-block (l & 3) of the tile's block (l & 15) >> 2; in K step ks
    // its 16 values are the row's bytes 128 ks + 16 (l >> 4) and 128 ks + 64 + 16 (l >> 4), 16 each:
    // each load instruction reads 64 contiguous bytes per row (plain loads: non-temporal ones
    // measured 2.5 % slower).  The compact-block -> sample-block map is looked up per tile for its
    // four blocks (uniform: scalar loads).  No vector load but the samples' in the loop: a wait for
    // one would also wait for the prefetched samples.
    const int ab = (l & 15) >> 2, as = l & 3;
    auto src = [&](int64_t gt) {
        int64_t mb[I8_BPT];
#pragma unroll
        for (int b = 0; b < I8_BPT; ++b) {
            const int64_t gb = gt + b < g1 ? gt + b : g1 - 1;
            const int r = find_range_i8(bcs, nr, gb);
            mb[b] = bstart[r] + (gb - bcs[r]);
        }
        const int64_t m = ab == 0 ? mb[0] : ab == 1 ? mb[1] : ab == 2 ? mb[2] : mb[3];
        return reinterpret_cast<const v4u *>(x + 2 * (m * D + as * I8_SUB)) + grp;
    };
    // the staged tile [pend, pend + 4) to out (bin-major): lane 4 row + b one 16-B entry, one
    // store instruction per tile (nk + 2 segments of 64 B)
    const int rw = nk + 2;
    int64_t pend = -1;
    auto flush = [&]() __attribute__((always_inline)) {
        if (pend < 0) return;
        const int64_t nv = g1 - pend < I8_BPT ? g1 - pend : I8_BPT;
        const int row = l >> 2, b = l & 3;
        __builtin_amdgcn_wave_barrier();
        if (row < rw && b < nv) out[row * nblocks + pend + b] = sOut[wv][b * RW + row];
        __builtin_amdgcn_wave_barrier();
    };
    // Software-pipelined over tile pairs, one wave per SIMD (512 VGPRs): tile k's MFMAs run into
    // one accumulator set while the float64 reduction of tile k - 1 (the other set) is interleaved
    // slice by slice between its K steps; two tiles of samples in flight per wave.
    struct Post {
        double ym;
        double ax[NX > 0 ? NX : 1];
        uint32_t bsum;
    };
    auto slice = [&](const Acc<NT> &A, int s, Post &P) __attribute__((always_inline)) {
        if (s < I8_SB) {  // this lane's component, sub-block s
            const int r = s;
            double p = __builtin_fma(256.0, (double)A.h[5][r], (double)A.l[5][r]);
#pragma unroll
            for (int d = 4; d >= 0; --d)
                p = __builtin_fma(p, 0x1p-8, __builtin_fma(256.0, (double)A.h[d][r], (double)A.l[d][r]));
            p *= 0x1p-6;
            const double q = dpp64<0xB1>(p);
            const double2 w = tw(0, r);
            P.ym = __builtin_fma(p, w.x, P.ym);
            P.ym = __builtin_fma(q, w.y, P.ym);
        } else {  // the extra bins' digit lanes, sub-block s - 4
            const int r = s - I8_SB;
#pragma unroll
            for (int e = 0; e < NX; ++e) {
                if (e == 0) P.bsum += ((uint32_t)A.h[6][r] << 8) + (uint32_t)A.l[6][r];
                const double v = __builtin_fma(256.0, (double)A.h[6 + e][r], (double)A.l[6 + e][r]);
                const double u = dpp64<0x128>(v);
                const double2 w = tw(1 + e, r);
                P.ax[e] = __builtin_fma(v, w.x, P.ax[e]);
                P.ax[e] = __builtin_fma(u, w.y, P.ax[e]);
            }
        }
    };
    auto finish = [&](Post &P, uint32_t habs, int64_t gt) __attribute__((always_inline)) {
        double yx[NX > 0 ? NX : 1];
#pragma unroll
        for (int e = 0; e < NX; ++e) {
            double acc = P.ax[e] * xscale;
            acc += dpp64<0xB1>(acc);
            acc += dpp64<0x4E>(acc);
            acc += dpp64<0x141>(acc);
            yx[e] = acc;
        }
        int hs = (int)habs;
        hs += __builtin_amdgcn_mov_dpp(hs, 0xB1, 0xf, 0xf, true);
        hs += __builtin_amdgcn_mov_dpp(hs, 0x4E, 0xf, 0xf, true);
        hs = add_xor32_i(add_xor16_i(hs));
        double *st = reinterpret_cast<double *>(sOut[wv]);
        if (c < ncomp) st[2 * (grp * RW + (c >> 1)) + (c & 1)] = P.ym;
#pragma unroll
        for (int e = 0; e < NX; ++e)
            if (dg == 0) st[2 * (grp * RW + 8 + e) + (c >> 3)] = yx[e];
        const double l1 = 256.0 * ((double)hs + 2.0 * D);
        if constexpr (NX > 0) {
            if (c == 6 || c == 7) st[2 * (grp * RW + nk) + (c - 6)] = (double)(int32_t)P.bsum;
            if (c == 4 * grp) sOut[wv][grp * RW + nk + 1] = make_double2(l1, 0.0);
        } else if (c == 4 * grp) {
            sOut[wv][grp * RW + nk] = make_double2(0.0, 0.0);
            sOut[wv][grp * RW + nk + 1] = make_double2(2.0 * l1, 0.0);
        }
        pend = gt;
    };
    auto post_all = [&](const Acc<NT> &A, uint32_t habs, int64_t gt) __attribute__((always_inline)) {
        Post P{};
#pragma unroll
        for (int s = 0; s < 2 * I8_SB; ++s) slice(A, s, P);
        finish(P, habs, gt);
    };
    const int64_t cnt = (ntiles - wave + nwaves - 1) / nwaves;  // this wave's tiles: wave + k nwaves
    auto tg = [&](int64_t k) { return (wave + (k < cnt ? k : cnt - 1) * nwaves) * I8_BPT; };
    // tile k's MFMAs from R into A (R refilled with tile k2's samples), the reduction of the other
    // set PA (tile kp) interleaved when DO_POST
    auto kloop = [&](v4u (&R)[2 * I8_KS], Acc<NT> &A, uint32_t &habs, int64_t k2, auto do_post, const Acc<NT> &PA,
                     uint32_t phabs, int64_t pgt) __attribute__((always_inline)) {
        const v4u *pn = src(tg(k2));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            A.h[t] = v4i{0, 0, 0, 0};
            const int ci = sInit[t * 16 + c];
            A.l[t] = v4i{ci, ci, ci, ci};
        }
        habs = 0;
        int boff = l;
        asm volatile("" : "+v"(boff));
        Post P{};
#pragma unroll
        for (int ks = 0; ks < I8_KS; ++ks) {
            v4i bk[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bk[t] = sB[(t * I8_KS + ks) * 64 + boff];
            uint32_t w[8];
            __builtin_memcpy(w, &R[2 * ks], 32);
            v4i ah, al;
            digits(w, ah, al, habs);
            R[2 * ks] = pn[8 * ks];
            R[2 * ks + 1] = pn[8 * ks + 4];
            if (ks == 0) flush();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                A.h[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bk[t], A.h[t], 0, 0, 0);
                A.l[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bk[t], A.l[t], 0, 0, 0);
                if constexpr (decltype(do_post)::value)
                    if (t == NT / 2) slice(PA, ks, P);  // a slice of the other tile's reduction
            }
        }
        if constexpr (decltype(do_post)::value) finish(P, phabs, pgt);
    };
    v4u R0[2 * I8_KS], R1[2 * I8_KS];
    {
        const v4u *p0 = src(tg(0)), *p1 = src(tg(1));
#pragma unroll
        for (int ks = 0; ks < I8_KS; ++ks) {
            R0[2 * ks] = p0[8 * ks];
            R0[2 * ks + 1] = p0[8 * ks + 4];
            R1[2 * ks] = p1[8 * ks];
            R1[2 * ks + 1] = p1[8 * ks + 4];
        }
    }
    Acc<NT> A0, A1;
    uint32_t h0 = 0, h1 = 0;
    kloop(R0, A0, h0, 2, std::false_type{}, A1, 0u, 0);
    int64_t k = 1;
    for (; k + 1 < cnt; k += 2) {
        kloop(R1, A1, h1, k + 2, std::true_type{}, A0, h0, tg(k - 1));
        kloop(R0, A0, h0, k + 3, std::true_type{}, A1, h1, tg(k));
    }
    if (k < cnt) {
        kloop(R1, A1, h1, k, std::true_type{}, A0, h0, tg(k - 1));
        flush();
        post_all(A1, h1, tg(k));
    } else {
        flush();
        post_all(A0, h0, tg(k - 1));
    }
    flush();
}

}  // namespace

bool i8_supported(const RefineGeom &G, const RefineBins &K) {
    return G.D == I8_SB * I8_SUB && K.dc < 0 && K.nk >= 1 && K.nk <= 10;
}

int launch_refine_i8(msd_ctx *ctx, const int16_t *x, const RefineGeom &G, const RefineBins &K, const int64_t *d_bstart,
                     const int64_t *d_bcs, int64_t nblocks, double2 *blk) {
    const int nk = K.nk;
    const int NT = nk <= 8 ? 6 : 6 + (nk - 8);
    const int N = G.N;
    // host tables (B fragments, column starts, lane twiddles), built once per (N, bins) and kept
    uint64_t key = (uint64_t)N * 1000003u + (uint64_t)nk;
    for (int b = 0; b < nk; ++b) key = key * 1000003u + (uint64_t)K.km[b];
    const size_t nb_frag = sizeof(v4i) * (size_t)NT * I8_KS * 64;
    const size_t nb_init = sizeof(int) * (size_t)NT * 16;
    const size_t nb_tw = sizeof(double2) * (size_t)(1 + (NT - 6)) * I8_SB * 16;
    const size_t nb_all = nb_frag + nb_init + nb_tw;
    RefineI8Cache &c8 = ctx->refine_i8;
    bool same = c8.i8_tab.get() && c8.i8_key == key && c8.i8_n == N && c8.i8_nk == nk;
    for (int b = 0; same && b < nk; ++b) same = c8.i8_km[b] == K.km[b];
    if (!same) {
        // column (t, c) -> (bin, part, digit), or -1
        auto colmap = [&](int t, int cc, int &bin, int &part, int &dig) {
            if (t < 6) {
                bin = cc >> 1, part = cc & 1, dig = t;
                return bin < nk && bin < 8;
            }
            bin = 8 + (t - 6), part = cc >> 3, dig = cc & 7;
            return bin < nk && dig < I8_ND;
        };
        // tile 6, columns 6 / 7: ones on the I / Q values (the sub-block sums, block_i8_kernel)
        auto sumcol = [&](int t, int cc) { return t == 6 && (cc == 6 || cc == 7); };
        // B[t][v][c] for v < KV: value v of a sub-block row = sample v >> 1, I (v even) or Q
        constexpr int KV = 2 * I8_SUB;
        std::vector<int8_t> Bm((size_t)NT * KV * 16, 0);
        std::vector<int> init((size_t)NT * 16, 0);
        // T^c, T^s of every needed bin over a sub-block (refine_i8_coeffs: what msd_i8_coeffs kind 2 returns)
        std::vector<int64_t> Tc((size_t)nk * I8_SUB), Ts((size_t)nk * I8_SUB);
        for (int b = 0; b < nk; ++b) {
            refine_i8_coeffs(I8_SUB, N, K.km[b], 0, &Tc[(size_t)b * I8_SUB]);
            refine_i8_coeffs(I8_SUB, N, K.km[b], 1, &Ts[(size_t)b * I8_SUB]);
        }
        for (int t = 0; t < NT; ++t)
            for (int cc = 0; cc < 16; ++cc) {
                if (sumcol(t, cc)) {
                    for (int v = 0; v < KV; ++v) Bm[((size_t)t * KV + v) * 16 + cc] = (v & 1) == cc - 6 ? 1 : 0;
                    init[t * 16 + cc] = 128 * I8_SUB;
                    continue;
                }
                int bin, part, dig;
                if (!colmap(t, cc, bin, part, dig)) continue;
                const int64_t *tc = &Tc[(size_t)bin * I8_SUB], *ts = &Ts[(size_t)bin * I8_SUB];
                for (int v = 0; v < KV; ++v) {
                    const int m = v >> 1;
                    // W^{km} = C - i S;  Y = sum (I + i Q)(C - i S): re = I C + Q S, im = Q C - I S
                    // (T = round(w 2^46) from the long-double value: |T 2^-46 - w| <= 2^-47 (1 + 2^-16);
                    // |T| <= 2^46 fits the six digits; rounding is odd, so -T^s = round(-S 2^46))
                    const int64_t T = part == 0 ? ((v & 1) ? ts[m] : tc[m]) : ((v & 1) ? tc[m] : -ts[m]);
                    int8_t d[I8_ND];
                    if (!balanced_digits(T, d))
                        return fail(MSD_ERR_INVALID, "refine_i8: twiddle beyond 6 digits");
                    Bm[((size_t)t * KV + v) * 16 + cc] = d[dig];
                    init[t * 16 + cc] += 128 * (int)d[dig];
                }
            }
        std::vector<char> tab(nb_all);
        auto *frag = reinterpret_cast<int8_t *>(tab.data());
        for (int t = 0; t < NT; ++t)
            for (int ks = 0; ks < I8_KS; ++ks)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 16; ++j) {  // lane l byte j of step ks (block_i8_kernel's loads)
                        const int v = frag_sample(ks, l >> 4, j);
                        frag[(((size_t)t * I8_KS + ks) * 64 + l) * 16 + j] = Bm[((size_t)t * KV + v) * 16 + (l & 15)];
                    }
        std::memcpy(tab.data() + nb_frag, init.data(), nb_init);
        auto *ltw = reinterpret_cast<double2 *>(tab.data() + nb_frag + nb_init);
        for (int e = 0; e <= NT - 6; ++e)
            for (int r = 0; r < I8_SB; ++r)
                for (int cc = 0; cc < 16; ++cc) {
                    const int s = r;  // C row r of every lane group: sub-block r of its block
                    int bin, part;
                    if (e == 0) bin = cc >> 1, part = cc & 1;
                    else bin = 8 + (e - 1), part = cc >> 3;
                    double2 w = make_double2(0.0, 0.0);
                    if (bin < nk && (e > 0 || bin < 8)) {
                        // W^{256 k s} = cos - i sin: own part p, partner q: re = p cos + q sin (own re),
                        // im = p cos - q sin (own im, partner re)
                        long double c, sn;
                        unit_root_ld((int64_t)K.km[bin] * I8_SUB * s, N, c, sn);
                        w = make_double2((double)c, part == 0 ? (double)sn : -(double)sn);
                    }
                    ltw[(e * I8_SB + r) * 16 + cc] = w;
                }
        DeviceGuard gd(ctx->device);
        MSD_HIP(hipStreamSynchronize(ctx->stream));
        c8.i8_key = 0;
        if (int rc = c8.i8_tab.upload(tab.data(), nb_all, "refine_i8: tables")) return rc;
        c8.i8_key = key;
        c8.i8_n = N;
        c8.i8_nk = nk;
        for (int b = 0; b < nk; ++b) c8.i8_km[b] = K.km[b];
    }
    const char *tb = c8.i8_tab.get();
    const v4i *d_frag = reinterpret_cast<const v4i *>(tb);
    const int *d_init = reinterpret_cast<const int *>(tb + nb_frag);
    const double2 *d_tw = reinterpret_cast<const double2 *>(tb + nb_frag + nb_init);
    // persistent: 8 waves per CU (2 workgroups of 4), the tiles interleaved over them
    const int64_t waves_max = (int64_t)ctx->num_cu * 4;
    const int64_t ntiles = (nblocks + I8_BPT - 1) / I8_BPT;
    const unsigned grid = (unsigned)((std::min(waves_max, ntiles) + 3) / 4);
    hipStream_t st = ctx->stream;
    switch (NT) {
        case 6:
            hipLaunchKernelGGL(block_i8_kernel<6>, dim3(grid), dim3(256), 0, st, x, (int64_t)G.D, d_bstart, d_bcs, G.nr,
                               nblocks, nk, d_frag, d_init, d_tw, blk);
            break;
        case 7:
            hipLaunchKernelGGL(block_i8_kernel<7>, dim3(grid), dim3(256), 0, st, x, (int64_t)G.D, d_bstart, d_bcs, G.nr,
                               nblocks, nk, d_frag, d_init, d_tw, blk);
            break;
        case 8:
            hipLaunchKernelGGL(block_i8_kernel<8>, dim3(grid), dim3(256), 0, st, x, (int64_t)G.D, d_bstart, d_bcs, G.nr,
                               nblocks, nk, d_frag, d_init, d_tw, blk);
            break;
        default: return fail(MSD_ERR_UNSUPPORTED, "refine_i8: bins");
    }
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

// our float64-side rounding chain in units of u = 2^-53 (refine_plan.h's `own`): the twiddles'
// quantisation sqrt 2 * 2^-47 (1 + 2^-16) per unit |x| (90.5; each entry rounded from a long-double
// unit root whose argument was reduced exactly, unit_root_ld), the digit Horner sum (6), the 4 sub-block
// products summed with rounded twiddles in one 8-FMA chain (10; the budget kept at 22, the
// 16-sub-block layout's figure)
double i8_chain_own() { return MSD_REFINE_I8_CHAIN_QUANT + MSD_REFINE_I8_CHAIN_HORNER + MSD_REFINE_I8_CHAIN_SUBBLOCK; }

}  // namespace msd
