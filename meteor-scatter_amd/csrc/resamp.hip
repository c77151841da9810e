// The rational-ratio resampler (include/msdsp.h, msd_resamp_*): the down-converter of ddc.hip at any ratio
// L / M = up / down.  Output m: t = m M + c, phi = t mod L, n0 = t div L,
// v[m] = sum_{i < I_phi} h[phi + i L] z[n0 - i], z = x (REAL) or x[n] e^{-2 pi i r(n) / q} (SSB),
// y[m] = gain v[m] (REAL) or gain Re(i^m v[m]) (SSB).  float64 throughout, no contraction but the explicit
// FMAs below.
//
// resamp_kernel: one workgroup produces a tile of TM outputs of one row (a grid-stride loop over the
// (row, tile) pairs).  The taps go into LDS once per workgroup, in their own order, which is branch-minor
// ([i][phi] at i L + phi): at a fixed i the lanes' branches phi_t are distinct or equal, so the lanes read
// distinct or broadcast slots.  Per tile the workgroup stages the samples nb .. n0(m0 + nout - 1),
// nb = n0(m0) - (I - 1): every sample is read once from global memory, converted, mixed once (SSB) and
// stored linearly, Re z and Im z in separate planes.  The tile's position arithmetic is 64-bit once per
// tile (phi0 = (m0 M + c) mod L and n0(m0)); a thread then finds its output's branch and sample offset from
// phi0 + o M in 32 bits.  Thread (g, t) runs the FMA chain of group g of output o(t) (the lane map of
// resamp_plan.h, which spreads a half-wave's sample reads over the banks): one tap read, one sample read of
// the plane Re(i^m v) needs, one FMA per tap.  The G partial sums go through LDS and are added in group
// order; gain, the output mixer's sign, the store (float64, or rint and saturate to int16).
// The loop is the software pipeline of ddc_kernel: behind the staging barrier the workgroup issues the
// loads of its next tile's first RS_BATCH_LOADS samples per thread, which stay in flight while the current
// tile is filtered.
// The summation order is resamp_plan.h's, by (ntaps, L, M) and the branch alone; the tile, the grid, the
// row, the lane map and the entry point only decide which thread computes an output, never how.
//
// Where a sample comes from: as in ddc.hip, with a history of H = I - 1 raw samples per stream.
//
// Bytes per input sample: its own size in, 8 L / M (2 L / M as int16) out, plus I / (TM M / L) of the sample
// size again for the tile's overlap with its neighbour.  LDS per output: I tap reads and I sample reads of
// 8 bytes.
#include <cmath>

#include "msd_internal.h"
#include "resamp_plan.h"

#pragma clang fp contract(off)

struct ResampState {  // one stream, on the device
    int64_t start;  // the position the stream was reset to
    int64_t count;  // the position of the next sample
    int64_t cur;    // which of the two history buffers is current
    int64_t reserved;
};

struct msd_resamp_plan {
    msd_ctx *ctx = nullptr;
    msd_resamp_cfg cfg{};
    msd::resamp::Plan P{};
    int64_t nstreams = 0, max_push = 0;
    msd::DevBuf<double> d_taps;
    msd::DevBuf<double2> d_tw1, d_tw2;
    msd::DevBuf<ResampState> d_state;
    msd::DevBuf<unsigned char> d_hist;  // [nstreams][2][I - 1] samples of 8 bytes at the most
    msd::DevBuf<int64_t> d_meta;        // the host forms' {off, len, pos0}
    int64_t h_meta[4] = {0, 0, 0, 0};
    std::vector<int> dtype;             // per stream: the dtype of its pushes since the last reset (0: none yet)
    std::vector<char> flushed;
};

namespace msd {
namespace {

constexpr int RS_THREADS = resamp::THREADS;
constexpr int RS_HIST_ELEM = 8;     // bytes reserved per history sample (MSD_CF32)
constexpr int RS_BATCH_LOADS = 8;   // samples a thread has in flight while it stages (a multiple of 4)
enum { RS_BATCH = 0, RS_PUSH = 1, RS_FLUSH = 2 };

struct ResampArgs {
    resamp::Plan P;
    int kind;
    int64_t nrows, tiles_per_row, ld_out, max_len, stream0;
};

// one sample as (re, im) float64: exact for every input dtype
__device__ __forceinline__ void rs_cvt(int16_t v, double &re, double &im) { re = (double)v, im = 0.0; }
__device__ __forceinline__ void rs_cvt(float v, double &re, double &im) { re = (double)v, im = 0.0; }
__device__ __forceinline__ void rs_cvt(short2 v, double &re, double &im) { re = (double)v.x, im = (double)v.y; }
__device__ __forceinline__ void rs_cvt(float2 v, double &re, double &im) { re = (double)v.x, im = (double)v.y; }
template <typename T>
__device__ __forceinline__ T rs_zero();
template <>
__device__ __forceinline__ int16_t rs_zero<int16_t>() { return 0; }
template <>
__device__ __forceinline__ float rs_zero<float>() { return 0.0f; }
template <>
__device__ __forceinline__ short2 rs_zero<short2>() { return make_short2(0, 0); }
template <>
__device__ __forceinline__ float2 rs_zero<float2>() { return make_float2(0.0f, 0.0f); }

__device__ __forceinline__ int64_t rs_cdiv(int64_t a, int64_t d) { return a >= 0 ? (a + d - 1) / d : -((-a) / d); }

// the samples and the outputs of one row
struct ResampRow {
    int64_t a_lo, a_hi;   // the call's samples: global indices [a_lo, a_hi) at x[xoff + n - a_lo]
    int64_t h_lo;         // the history covers [h_lo, a_lo) (a_lo for a batch row)
    int64_t xoff;
    int64_t m_lo, count;  // the outputs m_lo .. m_lo + count - 1
    int64_t hoff;         // the history's byte offset in the plan's buffer
};

__device__ __forceinline__ ResampRow rs_row(const ResampArgs &A, int64_t row, const int64_t *__restrict__ off,
                                            const int64_t *__restrict__ len, const int64_t *__restrict__ pos0,
                                            const ResampState *__restrict__ st) {
    const resamp::Plan &P = A.P;
    ResampRow R;
    R.hoff = 0;
    if (A.kind == RS_BATCH) {
        const int64_t n = len[row] > 0 ? len[row] : 0;
        R.a_lo = pos0[row];
        R.a_hi = R.a_lo + n;
        R.h_lo = R.a_lo;
        R.xoff = off[row];
        R.m_lo = rs_cdiv(R.a_lo * P.L, P.M);
        R.count = rs_cdiv(R.a_hi * P.L, P.M) - R.m_lo;
        return R;
    }
    const int64_t s = A.stream0 + row;
    const ResampState S = st[s];
    const int H = P.I - 1;
    int64_t n = 0;
    if (A.kind == RS_PUSH) {
        n = len[row] > 0 ? len[row] : 0;
        if (n > A.max_len) n = A.max_len;
        R.xoff = off[row];
    } else {
        R.xoff = 0;
    }
    R.a_lo = S.count;
    R.a_hi = S.count + n;
    R.h_lo = S.count - H;
    R.hoff = ((s * 2 + S.cur) * (int64_t)H) * RS_HIST_ELEM;
    // emitted so far: every m >= ceil(start L / M) with m M + c < count L
    const int64_t first = rs_cdiv(S.start * P.L, P.M);
    int64_t lo = rs_cdiv(S.count * P.L - P.c, P.M);
    if (lo < first) lo = first;
    int64_t hi = A.kind == RS_PUSH ? rs_cdiv(R.a_hi * P.L - P.c, P.M) : rs_cdiv(S.count * P.L, P.M);
    if (hi < lo) hi = lo;
    R.m_lo = lo;
    R.count = hi - lo;
    return R;
}

// one tile: outputs i0 .. i0 + nout - 1 of `row`, the first of them m0; staged sample 0 has global index nb
struct ResampTile {
    int64_t row, i0, m0, nb;
    int nout, S, phi0;
    int64_t a_lo, a_hi, h_lo, xoff, hoff;
};

// MIX: 0 REAL, 1 SSB with one table, 2 SSB with two
template <typename T, int MIX>
__global__ __launch_bounds__(RS_THREADS) void resamp_kernel(const T *__restrict__ x, const int64_t *__restrict__ off,
                                                            const int64_t *__restrict__ len,
                                                            const int64_t *__restrict__ pos0,
                                                            const ResampState *__restrict__ st,
                                                            const unsigned char *__restrict__ hist, ResampArgs A,
                                                            const double *__restrict__ taps,
                                                            const double2 *__restrict__ tw1,
                                                            const double2 *__restrict__ tw2, void *__restrict__ y,
                                                            int64_t *__restrict__ out_len) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    const resamp::Plan &P = A.P;
    double *pl = reinterpret_cast<double *>(rs_smem);  // [2][plane]: Re z, Im z (REAL: the first only)
    double *tl = pl + 2 * P.plane;                     // [I][L] taps, zero behind ntaps
    double *part = tl + P.tapn;                        // [G][TM] partial sums
    const int tid = threadIdx.x;
    const int L = P.L, M = P.M, TM = P.TM, ntaps = P.ntaps, I = P.I;
    const int64_t total = A.nrows * A.tiles_per_row;
    T raw[RS_BATCH_LOADS];  // a thread's samples j = jb + b 256 of a tile, as loaded

    // the taps, once (the first staging barrier orders them)
    for (int k = tid; k < P.tapn; k += RS_THREADS) tl[k] = k < ntaps ? taps[k] : 0.0;

    // the loads of the batch that starts at sample jb (zero outside the row and its history)
    auto load_batch = [&](const ResampTile &Q, int jb) {
#pragma unroll
        for (int b = 0; b < RS_BATCH_LOADS; ++b) {
            const int j = jb + b * RS_THREADS;
            const int64_t n = Q.nb + j;
            T v = rs_zero<T>();
            if (j < Q.S) {
                if (n >= Q.a_lo && n < Q.a_hi) v = x[Q.xoff + (n - Q.a_lo)];
                else if (n >= Q.h_lo && n < Q.a_lo) v = reinterpret_cast<const T *>(hist + Q.hoff)[n - Q.h_lo];
            }
            raw[b] = v;
        }
    };
    // tile w: its row's count to out_len (tile 0), its description (the 64-bit position arithmetic, once),
    // the loads of its first batch; false: the tile lies past the row's outputs
    auto fetch = [&](int64_t w, ResampTile &Q) -> bool {
        const int64_t row = w / A.tiles_per_row, t = w - row * A.tiles_per_row;
        const ResampRow R = rs_row(A, row, off, len, pos0, st);
        if (t == 0 && tid == 0) out_len[row] = R.count;
        const int64_t vis = R.count < A.ld_out ? R.count : A.ld_out;  // outputs of the row that are stored
        const int64_t i0 = t * TM;
        if (i0 >= vis) return false;  // (the whole workgroup)
        Q.row = row, Q.i0 = i0;
        Q.nout = (int)(vis - i0 < TM ? vis - i0 : TM);
        Q.m0 = R.m_lo + i0;
        const int64_t t0 = Q.m0 * M + P.c, n00 = t0 / L;  // (t0 >= 0)
        Q.phi0 = (int)(t0 - n00 * L);
        Q.nb = n00 - (I - 1);
        Q.S = (Q.phi0 + (Q.nout - 1) * M) / L + I;  // up to n0 of the tile's last output
        Q.a_lo = R.a_lo, Q.a_hi = R.a_hi, Q.h_lo = R.h_lo, Q.xoff = R.xoff;
        Q.hoff = R.hoff;
        load_batch(Q, tid);
        return true;
    };

    ResampTile Q;
    bool have = false;
    int64_t w = blockIdx.x;
    for (; w < total && !have; w += have ? 0 : gridDim.x) have = fetch(w, Q);
    if (!have) return;
    while (have) {
        const int nout = Q.nout, S = Q.S;
        const int64_t m0 = Q.m0;
        // ---- stage: sample j = tid, tid + 256, ... of the tile, mixed, into slot j; the first batch's loads
        // went out before the previous tile's filter
        {
            int r = 0;
            if (MIX) {
                int64_t nm = Q.nb % P.q;
                if (nm < 0) nm += P.q;
                r = (int)((((nm + tid) % P.q) * (int64_t)P.p) % P.q);
            }
            for (int jb = tid; jb < S; jb += RS_BATCH_LOADS * RS_THREADS) {
                if (jb != tid) load_batch(Q, jb);
#pragma unroll
                for (int b4 = 0; b4 < RS_BATCH_LOADS; b4 += 4) {
                    double2 wv[4], wh[4];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {  // the four phase factors' loads go out together
                        if (MIX == 1) wv[b] = tw1[r];
                        if (MIX == 2) wv[b] = tw1[r & (ddc::TABLE_MAX - 1)], wh[b] = tw2[r >> ddc::TABLE_BITS];
                        if (MIX) {
                            r += P.step;
                            if (r >= P.q) r -= P.q;
                        }
                    }
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int j = jb + (b4 + b) * RS_THREADS;
                        if (j < S) {
                            double xr, xi;
                            rs_cvt(raw[b4 + b], xr, xi);
                            if (MIX == 0) {
                                pl[j] = xr;
                            } else {
                                double2 f = wv[b];
                                if (MIX == 2) {
                                    f.x = fma(wh[b].x, wv[b].x, -(wh[b].y * wv[b].y));
                                    f.y = fma(wh[b].x, wv[b].y, wh[b].y * wv[b].x);
                                }
                                pl[j] = fma(xr, f.x, -(xi * f.y));
                                pl[P.plane + j] = fma(xr, f.y, xi * f.x);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- the next tile's first loads, in flight while this one is filtered
        ResampTile Qn;
        bool hn = false;
        int64_t wn = w + gridDim.x;
        for (; wn < total && !hn; wn += hn ? 0 : gridDim.x) hn = fetch(wn, Qn);

        // ---- filter: group g of output o, ascending i from +0.0, no further than the branch's own taps
        {
            const int g = tid / TM, t = tid - g * TM;
            const int A_ = TM / P.B;
            const int o = (t % A_) * P.B + t / A_;  // (powers of two)
            if (o < nout) {
                const int tt = Q.phi0 + o * M;
                const int dn = tt / L, phi = tt - dn * L;
                const int Iphi = phi < ntaps ? (ntaps - phi + L - 1) / L : 0;
                const int i0 = g * P.K;
                const int i1 = i0 + P.K < Iphi ? i0 + P.K : Iphi;
                const double *sp = pl + ((MIX && ((m0 + o) & 1)) ? P.plane : 0) + (I - 1) + dn - i0;
                const double *tp = tl + phi + i0 * L;
                double acc = 0.0;
#pragma unroll 4
                for (int i = i0; i < i1; ++i) {
                    acc = fma(*tp, *sp, acc);
                    tp += L;
                    --sp;
                }
                part[g * TM + o] = acc;
            }
        }
        lds_barrier();  // (orders the partial sums; the prefetched samples stay in flight)

        // ---- combine the groups in order, gain, the output mixer's sign, store
        if (tid < nout) {
            double v = part[tid];
            for (int g = 1; g < P.G; ++g) v = v + part[g * TM + tid];
            double o = P.gain * v;
            if (MIX) {
                const int mm = (int)((m0 + tid) & 3);
                if (mm == 1 || mm == 2) o = -o;
            }
            const int64_t at = Q.row * A.ld_out + Q.i0 + tid;
            if (P.out_i16) {
                double rv = rint(o);
                rv = rv < -32768.0 ? -32768.0 : (rv > 32767.0 ? 32767.0 : rv);
                if (!(rv == rv)) rv = 0.0;  // NaN
                static_cast<int16_t *>(y)[at] = (int16_t)(int)rv;
            } else {
                static_cast<double *>(y)[at] = o;
            }
        }
        // (the next tile's staging writes the planes: every filter chain has passed the second barrier;
        // its filter writes part behind the next barrier, which this combine precedes)
        Q = Qn, have = hn, w = wn;
    }
}

// after a push: the stream's last H = I - 1 samples into its other history buffer, then the position.
// One workgroup per stream.
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void resamp_advance_kernel(const T *__restrict__ x,
                                                                    const int64_t *__restrict__ off,
                                                                    const int64_t *__restrict__ len, ResampState *st,
                                                                    unsigned char *hist, int H, int64_t max_len,
                                                                    int64_t stream0) {
    const int64_t s = stream0 + blockIdx.x;
    const ResampState S = st[s];
    int64_t n = len[blockIdx.x] > 0 ? len[blockIdx.x] : 0;
    if (n > max_len) n = max_len;
    const T *old = reinterpret_cast<const T *>(hist + ((s * 2 + S.cur) * (int64_t)H) * RS_HIST_ELEM);
    T *nw = reinterpret_cast<T *>(hist + ((s * 2 + (S.cur ^ 1)) * (int64_t)H) * RS_HIST_ELEM);
    const int64_t xo = off[blockIdx.x];
    for (int i = threadIdx.x; i < H; i += RS_THREADS) {
        // the new history's sample i has global index count + n - H + i
        const int64_t rel = n - H + i;  // relative to the old count
        nw[i] = rel >= 0 ? x[xo + rel] : old[i + n];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        st[s].count = S.count + n;
        st[s].cur = S.cur ^ 1;
    }
}

__global__ void resamp_reset_kernel(ResampState *st, unsigned char *hist, int H, int64_t stream0, int64_t pos0) {
    const int64_t s = stream0 + blockIdx.x;
    const int64_t bytes = 2 * (int64_t)H * RS_HIST_ELEM;
    unsigned char *h = hist + s * bytes;
    for (int64_t i = threadIdx.x; i < bytes; i += blockDim.x) h[i] = 0;
    if (threadIdx.x == 0) st[s] = ResampState{pos0, pos0, 0, 0};
}

template <typename T, int MIX>
int rs_launch_t(msd_resamp_plan *p, const ResampArgs &A, const void *x, const int64_t *off, const int64_t *len,
                const int64_t *pos0, void *y, int64_t *out_len) {
    msd_ctx *ctx = p->ctx;
    auto kern = resamp_kernel<T, MIX>;
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(kern), (int)ddc::LDS_MAX)) return rc;
    const int64_t total = A.nrows * A.tiles_per_row;
    int per_cu = (int)((160 * 1024) / p->P.lds_bytes);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int64_t slots = (int64_t)ctx->num_cu * per_cu;
    const int64_t grid = total < slots ? total : slots;
    if (grid < 1 || grid > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, "msd_resamp: grid too large");
    KernelTimer timer(ctx, K_RESAMP);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RS_THREADS), p->P.lds_bytes, ctx->stream,
                       static_cast<const T *>(x), off, len, pos0, p->d_state.get(), p->d_hist.get(), A, p->d_taps.get(),
                       p->d_tw1.get(), p->d_tw2.get(), y, out_len);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

int rs_launch(msd_resamp_plan *p, int kind, const void *x, int dtype, const int64_t *off, const int64_t *len,
              const int64_t *pos0, int64_t nrows, int64_t stream0, void *y, int64_t ld_out, int64_t *out_len) {
    const resamp::Plan &P = p->P;
    ResampArgs A{};
    A.P = P;
    A.kind = kind;
    A.nrows = nrows;
    A.ld_out = ld_out;
    A.max_len = p->max_push;
    A.stream0 = stream0;
    A.tiles_per_row = ld_out > 0 ? (ld_out + P.TM - 1) / P.TM : 1;
    if (nrows > 0 && A.tiles_per_row > INT64_MAX / nrows) return fail(MSD_ERR_UNSUPPORTED, "msd_resamp: grid too large");
    const int mix = P.mode == MSD_DDC_SSB ? (P.two ? 2 : 1) : 0;
    switch (dtype) {
        case MSD_I16: return rs_launch_t<int16_t, 0>(p, A, x, off, len, pos0, y, out_len);
        case MSD_F32: return rs_launch_t<float, 0>(p, A, x, off, len, pos0, y, out_len);
        case MSD_CI16:
            return mix == 2 ? rs_launch_t<short2, 2>(p, A, x, off, len, pos0, y, out_len)
                            : rs_launch_t<short2, 1>(p, A, x, off, len, pos0, y, out_len);
        case MSD_CF32:
            return mix == 2 ? rs_launch_t<float2, 2>(p, A, x, off, len, pos0, y, out_len)
                            : rs_launch_t<float2, 1>(p, A, x, off, len, pos0, y, out_len);
        default: return fail(MSD_ERR_INVALID, "msd_resamp: unknown dtype");
    }
}

int rs_advance(msd_resamp_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len, int64_t stream0,
               int64_t nstreams) {
    hipStream_t s = p->ctx->stream;
    ResampState *st = p->d_state.get();
    unsigned char *h = p->d_hist.get();
    const int H = p->P.I - 1;
    const dim3 g((unsigned)nstreams), b(RS_THREADS);
    switch (dtype) {
        case MSD_I16:
            hipLaunchKernelGGL(resamp_advance_kernel<int16_t>, g, b, 0, s, static_cast<const int16_t *>(x), off, len, st, h,
                               H, p->max_push, stream0);
            break;
        case MSD_F32:
            hipLaunchKernelGGL(resamp_advance_kernel<float>, g, b, 0, s, static_cast<const float *>(x), off, len, st, h, H,
                               p->max_push, stream0);
            break;
        case MSD_CI16:
            hipLaunchKernelGGL(resamp_advance_kernel<short2>, g, b, 0, s, static_cast<const short2 *>(x), off, len, st, h,
                               H, p->max_push, stream0);
            break;
        default:
            hipLaunchKernelGGL(resamp_advance_kernel<float2>, g, b, 0, s, static_cast<const float2 *>(x), off, len, st, h,
                               H, p->max_push, stream0);
            break;
    }
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

// the dtype check of a push to streams [s0, s0 + n): fits the mode, equals the streams' dtype so far
int rs_claim_dtype(msd_resamp_plan *p, const char *fn, int dtype, int64_t s0, int64_t n) {
    if (!ddc::dtype_fits(p->P.mode, dtype)) return fail(MSD_ERR_INVALID, std::string(fn) + ": dtype does not fit the mode");
    for (int64_t s = s0; s < s0 + n; ++s) {
        if (p->flushed[(size_t)s]) return fail(MSD_ERR_INVALID, std::string(fn) + ": the stream was flushed; reset it first");
        if (p->dtype[(size_t)s] && p->dtype[(size_t)s] != dtype)
            return fail(MSD_ERR_INVALID, std::string(fn) + ": the stream holds samples of another dtype; reset it first");
    }
    for (int64_t s = s0; s < s0 + n; ++s) p->dtype[(size_t)s] = dtype;
    return MSD_OK;
}

size_t rs_out_size(const msd_resamp_plan *p) { return p->P.out_i16 ? 2 : 8; }

// ceil(n L / M) + 1: the most outputs a push of n samples emits
int64_t rs_push_outputs(const msd_resamp_plan *p, int64_t n) { return (n * p->P.L + p->P.M - 1) / p->P.M + 1; }

// the host forms' read-back: the count, MSD_ERR_CAPACITY when it exceeds cap, else the outputs
int rs_read_back(msd_resamp_plan *p, const char *fn, const void *dy, const int64_t *dlen, void *y, int64_t cap,
                 int64_t *out_len) {
    msd_ctx *ctx = p->ctx;
    int64_t n = 0;
    MSD_HIP(hipMemcpyAsync(&n, dlen, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    if (out_len) *out_len = n;
    if (n > cap) return fail(MSD_ERR_CAPACITY, std::string(fn) + ": cap too small");
    if (n > 0) {
        if (!y) return fail(MSD_ERR_INVALID, std::string(fn) + ": null y");
        MSD_HIP(hipMemcpyAsync(y, dy, (size_t)n * rs_out_size(p), hipMemcpyDeviceToHost, ctx->stream));
        MSD_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MSD_OK;
}

// one row's samples and {off = 0, len = n, pos0} on the device
int rs_stage(msd_resamp_plan *p, const void *x, size_t bytes, int64_t n, int64_t pos0, const void **dx) {
    msd_ctx *ctx = p->ctx;
    void *ds = nullptr;
    if (int rc = ctx_scratch(ctx, SCRATCH_SAMPLES, (bytes + 255) / 256 * 256, &ds)) return rc;
    if (bytes) MSD_HIP(hipMemcpyAsync(ds, x, bytes, hipMemcpyHostToDevice, ctx->stream));
    p->h_meta[0] = 0;
    p->h_meta[1] = n;
    p->h_meta[2] = pos0;
    MSD_HIP(hipMemcpyAsync(p->d_meta.get(), p->h_meta, sizeof(p->h_meta), hipMemcpyHostToDevice, ctx->stream));
    *dx = ds;
    return MSD_OK;
}

// the output scratch of a host form: ld outputs and the count behind them
int rs_out_scratch(msd_resamp_plan *p, int64_t ld, void **dout, int64_t **dlen) {
    const size_t ybytes = ((size_t)ld * rs_out_size(p) + 15) / 16 * 16;
    if (int rc = ctx_scratch(p->ctx, SCRATCH_OUTPUT, ybytes + 16, dout)) return rc;
    *dlen = reinterpret_cast<int64_t *>(static_cast<char *>(*dout) + ybytes);
    return MSD_OK;
}

}  // namespace
}  // namespace msd

using namespace msd;

extern "C" {

int msd_resamp_out_len(const msd_resamp_cfg *cfg, int64_t pos0, int64_t n, int64_t *m0, int64_t *count) {
    const char *msg = "";
    if (int rc = resamp::out_len(cfg, pos0, n, m0, count, &msg)) return fail(rc, std::string("msd_resamp_out_len: ") + msg);
    return MSD_OK;
}

int msd_resamp_chain(const msd_resamp_cfg *cfg, double *chain) {
    if (!chain) return fail(MSD_ERR_INVALID, "msd_resamp_chain: null");
    resamp::Plan P;
    const char *msg = "";
    if (int rc = resamp::make_plan(cfg, P, &msg)) return fail(rc, std::string("msd_resamp_chain: ") + msg);
    *chain = resamp::chain(P);
    return MSD_OK;
}

int msd_resamp_plan_create(msd_ctx *ctx, const msd_resamp_cfg *cfg, const double *taps, int64_t nstreams,
                           int64_t max_push, msd_resamp_plan **out) {
    if (!ctx || !cfg || !taps || !out) return fail(MSD_ERR_INVALID, "msd_resamp_plan_create: null");
    if (nstreams < 0 || max_push < 0 || nstreams > (1 << 20) || max_push > ((int64_t)1 << 40))
        return fail(MSD_ERR_INVALID, "msd_resamp_plan_create: nstreams / max_push out of range");
    resamp::Plan P;
    const char *msg = "";
    if (int rc = resamp::make_plan(cfg, P, &msg)) return fail(rc, std::string("msd_resamp_plan_create: ") + msg);
    for (int k = 0; k < cfg->ntaps; ++k)
        if (!std::isfinite(taps[k])) return fail(MSD_ERR_INVALID, "msd_resamp_plan_create: taps must be finite");
    DeviceGuard g(ctx->device);
    std::unique_ptr<msd_resamp_plan> p(new msd_resamp_plan);
    p->ctx = ctx;
    p->cfg = *cfg;
    p->P = P;
    p->nstreams = nstreams;
    p->max_push = max_push;
    int rc;
    if ((rc = p->d_taps.upload(taps, (size_t)cfg->ntaps, "resampler taps"))) return rc;
    std::vector<double> t1, t2;
    if (P.mode == MSD_DDC_SSB) resamp::tables(P, t1, t2);
    if (t1.empty()) t1.assign(2, 0.0);
    if (t2.empty()) t2.assign(2, 0.0);
    static_assert(sizeof(double2) == 2 * sizeof(double), "double2 is two doubles");
    if ((rc = p->d_tw1.upload(reinterpret_cast<const double2 *>(t1.data()), t1.size() / 2, "resampler phase table"))) return rc;
    if ((rc = p->d_tw2.upload(reinterpret_cast<const double2 *>(t2.data()), t2.size() / 2, "resampler phase table"))) return rc;
    if ((rc = p->d_meta.alloc(4, "resampler meta"))) return rc;
    const size_t ns = (size_t)(nstreams > 0 ? nstreams : 1);
    if ((rc = p->d_state.alloc(ns, "resampler state"))) return rc;
    if ((rc = p->d_state.zero())) return rc;
    const size_t hb = ns * 2 * (size_t)(P.I - 1) * RS_HIST_ELEM;
    if ((rc = p->d_hist.alloc(hb > 16 ? hb : 16, "resampler history"))) return rc;
    if ((rc = p->d_hist.zero())) return rc;
    p->dtype.assign(ns, 0);
    p->flushed.assign(ns, 0);
    *out = p.release();
    return MSD_OK;
}

void msd_resamp_plan_destroy(msd_resamp_plan *plan) { destroy_plan(plan); }

int msd_resamp_run_dev(msd_resamp_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                       const int64_t *pos0, int64_t nrows, void *y, int64_t ld_out, int64_t *out_len) {
    if (!plan || nrows < 0 || ld_out < 0 || (nrows > 0 && (!x || !off || !len || !pos0 || !out_len || (!y && ld_out))))
        return fail(MSD_ERR_INVALID, "msd_resamp_run_dev: null or negative argument");
    if (!ddc::dtype_fits(plan->P.mode, dtype)) return fail(MSD_ERR_INVALID, "msd_resamp_run_dev: dtype does not fit the mode");
    if (nrows == 0) return MSD_OK;
    DeviceGuard g(plan->ctx->device);
    return rs_launch(plan, RS_BATCH, x, dtype, off, len, pos0, nrows, 0, y, ld_out, out_len);
}

int msd_resamp_run(msd_resamp_plan *plan, const void *x, int dtype, int64_t n, int64_t pos0, void *y, int64_t cap,
                   int64_t *out_len) {
    if (!plan || (!x && n) || n < 0 || cap < 0) return fail(MSD_ERR_INVALID, "msd_resamp_run: null or negative argument");
    if (!ddc::dtype_fits(plan->P.mode, dtype)) return fail(MSD_ERR_INVALID, "msd_resamp_run: dtype does not fit the mode");
    int64_t m0 = 0, count = 0;
    const char *msg = "";
    if (int rc = resamp::out_len(&plan->cfg, pos0, n, &m0, &count, &msg)) return fail(rc, std::string("msd_resamp_run: ") + msg);
    if (out_len) *out_len = count;
    if (count > cap) return fail(MSD_ERR_CAPACITY, "msd_resamp_run: cap too small");
    if (count == 0) return MSD_OK;
    if (!y) return fail(MSD_ERR_INVALID, "msd_resamp_run: null y");
    DeviceGuard g(plan->ctx->device);
    int rc;
    const void *dx = nullptr;
    if ((rc = rs_stage(plan, x, (size_t)n * ddc::elem_size(dtype), n, pos0, &dx))) return rc;
    void *dout = nullptr;
    int64_t *dlen = nullptr;
    if ((rc = rs_out_scratch(plan, count, &dout, &dlen))) return rc;
    const int64_t *m = plan->d_meta.get();
    if ((rc = rs_launch(plan, RS_BATCH, dx, dtype, m, m + 1, m + 2, 1, 0, dout, count, dlen))) return rc;
    return rs_read_back(plan, "msd_resamp_run", dout, dlen, y, cap, out_len);
}

int msd_resamp_push_dev(msd_resamp_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                        void *y, int64_t ld_out, int64_t *out_len) {
    if (!plan || !off || !len || !out_len || (!x && plan->max_push) || ld_out < 0 || (!y && ld_out))
        return fail(MSD_ERR_INVALID, "msd_resamp_push_dev: null or negative argument");
    if (plan->nstreams < 1) return fail(MSD_ERR_INVALID, "msd_resamp_push_dev: the plan has no streams");
    if (ld_out < rs_push_outputs(plan, plan->max_push))
        return fail(MSD_ERR_INVALID, "msd_resamp_push_dev: ld_out < ceil(max_push up / down) + 1");
    if (int rc = rs_claim_dtype(plan, "msd_resamp_push_dev", dtype, 0, plan->nstreams)) return rc;
    DeviceGuard g(plan->ctx->device);
    if (int rc = rs_launch(plan, RS_PUSH, x, dtype, off, len, nullptr, plan->nstreams, 0, y, ld_out, out_len)) return rc;
    return rs_advance(plan, x, dtype, off, len, 0, plan->nstreams);
}

int msd_resamp_push(msd_resamp_plan *plan, int64_t stream, const void *x, int dtype, int64_t n, void *y, int64_t cap,
                    int64_t *out_len) {
    if (!plan || (!x && n) || n < 0 || cap < 0) return fail(MSD_ERR_INVALID, "msd_resamp_push: null or negative argument");
    if (stream < 0 || stream >= plan->nstreams) return fail(MSD_ERR_INVALID, "msd_resamp_push: no such stream");
    if (n > plan->max_push) return fail(MSD_ERR_INVALID, "msd_resamp_push: n > max_push");
    if (int rc = rs_claim_dtype(plan, "msd_resamp_push", dtype, stream, 1)) return rc;
    DeviceGuard g(plan->ctx->device);
    int rc;
    const void *dx = nullptr;
    if ((rc = rs_stage(plan, x, (size_t)n * ddc::elem_size(dtype), n, 0, &dx))) return rc;
    const int64_t ld = rs_push_outputs(plan, n);
    void *dout = nullptr;
    int64_t *dlen = nullptr;
    if ((rc = rs_out_scratch(plan, ld, &dout, &dlen))) return rc;
    const int64_t *m = plan->d_meta.get();
    if ((rc = rs_launch(plan, RS_PUSH, dx, dtype, m, m + 1, nullptr, 1, stream, dout, ld, dlen))) return rc;
    if ((rc = rs_advance(plan, dx, dtype, m, m + 1, stream, 1))) return rc;
    return rs_read_back(plan, "msd_resamp_push", dout, dlen, y, cap, out_len);
}

int msd_resamp_flush(msd_resamp_plan *plan, int64_t stream, void *y, int64_t cap, int64_t *out_len) {
    if (!plan || cap < 0) return fail(MSD_ERR_INVALID, "msd_resamp_flush: null or negative argument");
    if (stream < 0 || stream >= plan->nstreams) return fail(MSD_ERR_INVALID, "msd_resamp_flush: no such stream");
    if (plan->flushed[(size_t)stream]) return fail(MSD_ERR_INVALID, "msd_resamp_flush: the stream was flushed; reset it first");
    DeviceGuard g(plan->ctx->device);
    int rc;
    int dtype = plan->dtype[(size_t)stream];
    if (!dtype) dtype = plan->P.mode == MSD_DDC_SSB ? MSD_CI16 : MSD_I16;  // nothing pushed: the history is zeros
    const int64_t ld = plan->P.c / plan->P.M + 2;
    void *dout = nullptr;
    int64_t *dlen = nullptr;
    if ((rc = rs_out_scratch(plan, ld, &dout, &dlen))) return rc;
    if ((rc = rs_launch(plan, RS_FLUSH, plan->d_hist.get(), dtype, nullptr, nullptr, nullptr, 1, stream, dout, ld, dlen)))
        return rc;
    plan->flushed[(size_t)stream] = 1;
    return rs_read_back(plan, "msd_resamp_flush", dout, dlen, y, cap, out_len);
}

int msd_resamp_reset(msd_resamp_plan *plan, int64_t stream, int64_t pos0) {
    if (!plan) return fail(MSD_ERR_INVALID, "msd_resamp_reset: null");
    if (stream < -1 || stream >= plan->nstreams || plan->nstreams < 1) return fail(MSD_ERR_INVALID, "msd_resamp_reset: no such stream");
    if (pos0 < 0 || pos0 > resamp::MAX_POS / plan->P.L) return fail(MSD_ERR_INVALID, "msd_resamp_reset: pos0 outside 0 .. 2^62 / up");
    DeviceGuard g(plan->ctx->device);
    const int64_t s0 = stream < 0 ? 0 : stream, n = stream < 0 ? plan->nstreams : 1;
    hipLaunchKernelGGL(resamp_reset_kernel, dim3((unsigned)n), dim3(RS_THREADS), 0, plan->ctx->stream, plan->d_state.get(),
                       plan->d_hist.get(), plan->P.I - 1, s0, pos0);
    MSD_HIP(hipGetLastError());
    for (int64_t s = s0; s < s0 + n; ++s) plan->dtype[(size_t)s] = 0, plan->flushed[(size_t)s] = 0;
    return MSD_OK;
}

}  // extern "C"
