// Two-sided power spectrogram of complex (I/Q) input at any frame length: scipy.signal.spectrogram(z, fs,
// 'hann', nperseg, noverlap, nfft) for complex z, any 1 <= nperseg <= nfft, nfft a power of two in
// [16, 8192], any 1 <= hop <= nperseg (cstft.hip keeps nperseg = nfft = 4096, the C5 shape).  Frame-major
// float32 out[(s * max_frames + t) * nfft + k], bins in FFT order, |X|^2 with sqrt(scale) in the window,
// constant detrend of the complex mean of the nperseg samples BEFORE the zero padding (the padded points
// carry window 0, so they stay 0 whatever the mean).
//
// Mapping.  A thread holds 16 points of a frame, so a frame takes U = nfft / 16 threads and a workgroup
// of max(256, U) threads transforms F = 256 / U frames per trip (256 at nfft 16, 4 at 1024, 1 from 4096
// on); the workgroups are persistent over contiguous ranges of F-frame groups.  Stockham autosort,
// decimation in time: a pass of radix R over an array whose first p outputs-so-far are done reads
// x[i + t N / R] (t < R), multiplies by W_(pR)^(t (i mod p)), transforms and writes y[(i - i mod p) R +
// i mod p + t p].  With thread u holding point u + U c in register c, EVERY pass reads u + U c and the last
// one leaves bin u + U c there, so the loads, the LDS reads and the stores are the same code for every
// shape: consecutive threads touch consecutive elements.  Passes (cstft_chain.h): one radix-2^(L mod 4)
// pass first (p = 1: no twiddles; 16 / R butterflies per thread), then L / 4 radix-16 passes
// (fft_butterfly.h dft16) whose 15 twiddles per pass a thread keeps in registers across frames, like its
// 16 window values.  LDS holds the array between passes only, element a at a + a / 16 (float2): pass q
// writes runs of p consecutive elements R p apart, which the padding spreads over all banks
// (tools/lds_bank_model.py; p = 1 writes 16-element rows at pitch 17).
// Output: from nfft 1024 on a wave's store instruction writes 256 consecutive bytes of one row straight
// from registers; below that the F rows of a trip (16 KB, contiguous in the frame-major output) go
// through an LDS tile so that every store instruction still writes consecutive bytes.
// Detrend: int16 sums are exact integers (float adds of integers below 2^24, then int32), float32 sums
// float64; mean = sum / nperseg in float64, subtracted as (x - hi) - lo with hi = float(mean), lo =
// float(mean - hi): the detrended sample is the float64 difference rounded to float32, so no bin needs
// excluding, and a constant stream (mean = the sample, lo = 0) gives exact zeros.
// Energy: etot != NULL adds each frame's own total power as 16 float32 partials (partial i: the bins of
// threads u with u / (U / 16) = i; U < 16: thread u's sum at partial u, zeros above).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <type_traits>

#include "cstft_chain.h"
#include "fft_butterfly.h"
#include "msd_internal.h"

namespace msd {
namespace {

using bfly::cmul;
using bfly::dft16;
using bfly::dft4;
using bfly::dft8;

template <int L>
struct Csa {
    static constexpr int N = 1 << L;
    static constexpr int U = N / 16;                  // threads per frame
    static constexpr int TPB = U > 256 ? U : 256;     // threads per workgroup
    static constexpr int F = TPB / U;                 // frames per trip
    static constexpr int R0 = csa_first_radix(L);     // leading small pass (1: none)
    static constexpr int N16 = csa_radix16_passes(L);
    static constexpr int TW = N16 - (R0 > 1 ? 0 : 1);  // radix-16 passes with twiddles
    static constexpr int P0 = R0 > 1 ? R0 : 16;        // p of the first of them
    // entries of the LDS twiddle tables: 16 p for every twiddled pass but the last
    static constexpr int TWL = TW >= 3 ? 16 * P0 * 17 : TW == 2 ? 16 * P0 : 0;
    static constexpr int PADN = N + N / 16;           // float2 per frame in LDS
    static constexpr bool EXCH = N > 16;              // any LDS exchange at all
    static constexpr bool TILE = U < 64;              // output through an LDS tile
    static constexpr int BUF_BYTES = EXCH ? F * PADN * 8 : 0;
    static constexpr int TILE_BYTES = TILE ? (F * N + F * N / 16) * 4 : 0;
    static constexpr int LDS_BYTES = BUF_BYTES + TILE_BYTES;
    static constexpr int LP = U >= 16 ? U / 16 : 1;   // lanes per energy partial
    // waves per SIMD the register budget is set for: 3 (168 VGPRs: 32 data, ~24 butterfly temporaries, 16
    // window, 16-32 prefetched samples, 30 per twiddled pass); 8192 (three twiddled passes; 8 waves per
    // workgroup) 2
    static constexpr int WAVES = L <= 12 ? 3 : 2;
};

__device__ __forceinline__ int pad16(int a) { return a + (a >> 4); }

template <typename T>
struct AnyIQ;
template <>
struct AnyIQ<int16_t> {
    using raw_t = uint32_t;
    using sum_t = int;
    __device__ static raw_t load(const int16_t *p) {
        return __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
    }
    __device__ static raw_t zero() { return 0u; }
    __device__ static float2 f(raw_t r) { return make_float2(cvt_i16_lo(r), cvt_i16_hi(r)); }
    // the thread's 16 integers summed as floats (exact: below 2^19)
    __device__ static void sums(const float2 *v, int &sr, int &si) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            a += v[c].x;
            b += v[c].y;
        }
        sr = (int)a;
        si = (int)b;
    }
};
template <>
struct AnyIQ<float> {
    using raw_t = float2;
    using sum_t = double;
    __device__ static raw_t load(const float *p) { return *reinterpret_cast<const float2 *>(p); }
    __device__ static raw_t zero() { return make_float2(0.f, 0.f); }
    __device__ static float2 f(raw_t r) { return r; }
    __device__ static void sums(const float2 *v, double &sr, double &si) {
        sr = 0.0;
        si = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            sr += (double)v[c].x;
            si += (double)v[c].y;
        }
    }
};

template <int CTRL>
__device__ __forceinline__ int dpp_v(int x) { return __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ float dpp_v(float x) { return dpp_f<CTRL>(x); }
template <int CTRL>
__device__ __forceinline__ double dpp_v(double x) { return dpp64<CTRL>(x); }
__device__ __forceinline__ int lane_v(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ double lane_v(double x, int l) {
    const long long v = __builtin_bit_cast(long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
    return __builtin_bit_cast(double, ((long long)hi << 32) | lo);
}

// sum over the aligned group of W consecutive lanes (W a power of two <= 64), in every lane of it; every
// lane of the wave takes part.  Up to a row of 16 by DPP (quad swaps, mirrored half rows, mirrored rows),
// the rows of a half or whole wave by readlane: no LDS round trip
template <int W, typename V>
__device__ __forceinline__ V lanes_sum(V v) {
    if constexpr (W >= 2) v += dpp_v<0xB1>(v);   // quad_perm [1,0,3,2]
    if constexpr (W >= 4) v += dpp_v<0x4E>(v);   // quad_perm [2,3,0,1]
    if constexpr (W >= 8) v += dpp_v<0x141>(v);  // row_half_mirror
    if constexpr (W >= 16) v += dpp_v<0x140>(v);  // row_mirror
    if constexpr (W >= 32) {  // (the sample sums: int or double)
        const V a = lane_v(v, 0) + lane_v(v, 16), b = lane_v(v, 32) + lane_v(v, 48);
        v = W == 64 ? a + b : (threadIdx.x & 32) ? b : a;
    }
    return v;
}

template <typename T, int L>
__global__ __launch_bounds__(Csa<L>::TPB, Csa<L>::WAVES) void cstft_any_kernel(
    const T *__restrict__ x, const int64_t *__restrict__ off, const int64_t *__restrict__ len, int64_t max_frames,
    int64_t total, int64_t ngroups, int64_t per, int nperseg, int hop, int detrend, const float *__restrict__ g_win,
    const float2 *__restrict__ g_tw, float *__restrict__ out, float *__restrict__ etot, int64_t estride) {
    using S = Csa<L>;
    using io = AnyIQ<T>;
    using sum_t = typename io::sum_t;
    constexpr int N = S::N, U = S::U, F = S::F, TPB = S::TPB, R0 = S::R0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *const buf = reinterpret_cast<float2 *>(smem);
    float *const tile = reinterpret_cast<float *>(smem + S::BUF_BYTES);
    __shared__ sum_t red[2][TPB / 64];  // U > 64: the waves' sums of a frame
    __shared__ float ered[TPB / 16];    // U = 512: the rows' energies
    const int tid = threadIdx.x;
    const int f = tid / U, u = tid % U;
    float2 *const fb = buf + f * S::PADN;  // this frame's array

    // per-thread constants, kept across frames: the window (x sqrt(scale); 0 past nperseg) of points
    // u + U c and the twiddles W_(16 p)^(t (u mod p)) of the radix-16 passes with p > 1
    float wr[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int n = u + U * c;
        wr[c] = n < nperseg ? g_win[n] : 0.f;
    }
    // ... the last pass's (p = N / 16: a different set per thread) in registers, the earlier passes'
    // (p <= 32: 16 p entries, [t][k]) in LDS tables; t k < 16 p, so the index into g_tw stays below N
    float2 tw[16];
    __shared__ float2 twl[S::TWL > 0 ? S::TWL : 1];
    {
        int p = S::P0, base = 0;
#pragma unroll
        for (int q = 0; q < S::TW; ++q, p *= 16) {
            const int step = N / (16 * p);
            if (q == S::TW - 1) {
#pragma unroll
                for (int t = 1; t < 16; ++t) tw[t] = g_tw[(t * (u & (p - 1))) * step];
            } else {
                for (int i = tid; i < 16 * p; i += TPB) twl[base + i] = g_tw[((i / p) * (i % p)) * step];
                base += 16 * p;
            }
        }
    }
    __syncthreads();
    const float rh = vgpr_f(0.70710678118654752440f);
    // LDS addresses as one per-thread base plus compile-time offsets (the padding is linear wherever the
    // stride is a multiple of 16, and a run of p | 16 elements never crosses a 16-element row):
    //   reads   pad16(u + U c)   = pad16(u) + c (U + U / 16)             (U a multiple of 16)
    //   writes  pad16(j + t p)   = pad16(j) + t p + (t p >> 4)           (j = (u - k) 16 + k, k < p)
    constexpr bool RLIN = U % 16 == 0;
    const int rd0 = pad16(u);
    auto rd = [&](int c) { return RLIN ? rd0 + c * (U + U / 16) : pad16(u + U * c); };

    typename io::raw_t raw[16];
    // the samples of this thread's frame of group `grp` into raw; whether that frame exists, and which
    const int64_t g_begin = (int64_t)blockIdx.x * per;
    const int64_t g_end = g_begin + per < ngroups ? g_begin + per : ngroups;
    // where the frame load_group loads next lies: frame ct of a stream of cnfr frames whose samples start
    // at cbase.  The two divisions and the two table reads run when a thread's frames enter a new stream,
    // not per trip (a trip advances a thread by F frames)
    int64_t ct = 0, cnfr = 0, cbase = 0;
    auto locate = [&](int64_t g) {
        const int64_t s = g / max_frames;
        const int64_t n = len[s];
        ct = g - s * max_frames;
        cnfr = n >= nperseg ? (n - nperseg) / hop + 1 : 0;
        cbase = off[s];
    };
    if (g_begin * F + f < total) locate(g_begin * F + f);
    auto load_group = [&](int64_t grp, bool &valid) {
        const int64_t g = grp * F + f;
        valid = g < total && ct < cnfr;
        const int64_t base = cbase + ct * (int64_t)hop;
        ct += F;
        if (ct >= max_frames && g + F < total) locate(g + F);
        // one address per thread plus compile-time offsets; points past nperseg (and a frame that does not
        // exist) are not read
        const T *p = x + 2 * (F == 1 ? uniform_i64(base) : base) + 2 * u;
        const int lim = valid ? nperseg - u : 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) raw[c] = U * c < lim ? io::load(p + 2 * U * c) : io::zero();
    };

    bool vnext = false;
    if (g_begin < g_end) load_group(g_begin, vnext);
    for (int64_t grp = g_begin; grp < g_end; ++grp) {
        const bool valid = vnext;
        const int64_t g = grp * F + f;
        float2 v[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = io::f(raw[c]);
        // ---- the frame's complex sample sum: per thread, over the frame's lanes of a wave, over its waves
        sum_t sr, si;
        io::sums(v, sr, si);
        if (grp + 1 < g_end) load_group(grp + 1, vnext);  // prefetch: raw is consumed
        sr = lanes_sum<(U < 64 ? U : 64)>(sr);
        si = lanes_sum<(U < 64 ? U : 64)>(si);
        if constexpr (U > 64) {
            const int wave = tid >> 6, lane = tid & 63;
            if (lane == 0) {
                red[0][wave] = sr;
                red[1][wave] = si;
            }
            lds_barrier();
            const int w0 = f * (U / 64);
            sr = 0;
            si = 0;
#pragma unroll
            for (int w = 0; w < U / 64; ++w) {
                sr += red[0][w0 + w];
                si += red[1][w0 + w];
            }
            // (red is written again only after this trip's exchange barriers)
        }
        float hr = 0.f, lr = 0.f, hi = 0.f, li = 0.f;
        if (detrend) {
            const double mr = (double)sr / (double)nperseg, mi = (double)si / (double)nperseg;
            hr = (float)mr;
            lr = (float)(mr - (double)hr);
            hi = (float)mi;
            li = (float)(mi - (double)hi);
        }
        // lo is zero whenever the mean is a float32 (a power-of-two nperseg and an int16 sum below 2^24; any
        // constant stream): one subtraction then.  The branch is the wave's, and (x - hi) - 0 = x - hi, so
        // either side gives the same bits
        if (__builtin_amdgcn_ballot_w64(lr != 0.f || li != 0.f) != 0) {
#pragma unroll
            for (int c = 0; c < 16; ++c)
                v[c] = make_float2(((v[c].x - hr) - lr) * wr[c], ((v[c].y - hi) - li) * wr[c]);
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) v[c] = make_float2((v[c].x - hr) * wr[c], (v[c].y - hi) * wr[c]);
        }

        // ---- the leading small pass: butterfly b of the thread is i = u + U b, its points v[b + t nb]
        if constexpr (R0 > 1) {
            constexpr int nb = 16 / R0;
            if constexpr (R0 == 2) {
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const float2 a = v[b], c = v[b + 8];
                    v[b] = bfly::cadd(a, c);
                    v[b + 8] = bfly::csub(a, c);
                }
            } else if constexpr (R0 == 4) {
#pragma unroll
                for (int b = 0; b < 4; ++b) dft4(v[b], v[b + 4], v[b + 8], v[b + 12]);
            } else {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float2 w8[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) w8[t] = v[b + 2 * t];
                    dft8(w8, rh);
#pragma unroll
                    for (int t = 0; t < 8; ++t) v[b + 2 * t] = w8[t];
                }
            }
            lds_barrier();  // everyone has read the previous trip's array
#pragma unroll
            for (int b = 0; b < nb; ++b)
#pragma unroll
                for (int t = 0; t < R0; ++t) {
                    // (U R0 a multiple of 16: linear in b; t < R0 stays inside the row)
                    const int a = (U * R0) % 16 == 0 ? pad16(u * R0) + t + b * (U * R0 + U * R0 / 16)
                                                     : pad16((u + U * b) * R0 + t);
                    fb[a] = v[b + t * nb];
                }
            lds_barrier();
#pragma unroll
            for (int c = 0; c < 16; ++c) v[c] = fb[rd(c)];
        }
        // ---- the radix-16 passes
        {
            int p = R0 > 1 ? R0 : 1;
#pragma unroll
            for (int q = 0; q < S::N16; ++q, p *= 16) {
                if (p > 1) {
                    if (q == S::N16 - 1) {
#pragma unroll
                        for (int t = 1; t < 16; ++t) v[t] = cmul(v[t], tw[t]);
                    } else {  // (the tables in pass order: p = P0 at 0, 16 P0 at 16 P0)
                        const float2 *tb = twl + (p == S::P0 ? 0 : 16 * S::P0) + (u & (p - 1));
#pragma unroll
                        for (int t = 1; t < 16; ++t) v[t] = cmul(v[t], tb[t * p]);
                    }
                }
                dft16(v);
                if (q + 1 < S::N16) {
                    const int k = u & (p - 1), j = (u - k) * 16 + k, w0 = pad16(j);
                    lds_barrier();  // everyone has read the array
#pragma unroll
                    for (int t = 0; t < 16; ++t) fb[w0 + t * p + ((t * p) >> 4)] = v[t];
                    lds_barrier();
#pragma unroll
                    for (int c = 0; c < 16; ++c) v[c] = fb[rd(c)];
                }
            }
        }
        // ---- powers: v[c] is bin u + U c (a frame that does not exist loaded zeros and carries zeros here)
        float pw[16], esum = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            pw[c] = v[c].x * v[c].x + v[c].y * v[c].y;
            esum += pw[c];
        }
        if constexpr (S::TILE) {
            // the trip's F rows are F N consecutive floats of the output: through the tile (padded like
            // the array), then TPB consecutive floats per store instruction
            lds_barrier();  // the previous trip's tile has been read
#pragma unroll
            for (int c = 0; c < 16; ++c) tile[f * (N + N / 16) + rd(c)] = pw[c];
            lds_barrier();
            const int64_t o0 = grp * (int64_t)(F * N);
            const int64_t lim = (total - grp * F) * (int64_t)N;  // floats of existing frames from o0 on
#pragma unroll
            for (int m = 0; m < F * N / TPB; ++m) {
                const int a = tid + TPB * m;
                if (a < lim) __builtin_nontemporal_store(tile[pad16(tid) + m * (TPB + TPB / 16)], out + o0 + a);
            }
        } else {
            if (g < total) {
                float *const of = out + (F == 1 ? uniform_i64(g * (int64_t)N) : g * (int64_t)N) + u;
#pragma unroll
                for (int c = 0; c < 16; ++c) __builtin_nontemporal_store(pw[c], of + U * c);
            }
        }
        // ---- the frame's own energy in 16 partials
        if (etot) {
            if constexpr (U < 16) {
                if (valid) {
#pragma unroll
                    for (int m = 0; m < 16 / U; ++m) etot[(int64_t)(u + U * m) * estride + g] = m == 0 ? esum : 0.f;
                }
            } else if constexpr (S::LP <= 16) {
                const float e = lanes_sum<S::LP>(esum);
                if (valid && u % S::LP == 0) etot[(int64_t)(u / S::LP) * estride + g] = e;
            } else {  // U = 512, one frame: partial i = rows 2 i and 2 i + 1
                const float e = lanes_sum<16>(esum);
                if ((tid & 15) == 0) ered[tid >> 4] = e;
                lds_barrier();
                if (valid && tid < 16) etot[(int64_t)tid * estride + g] = ered[2 * tid] + ered[2 * tid + 1];
                // (ered is written again only after the next trip's exchange barriers)
            }
        }
    }
}

template <typename T, int L>
int launch_l(msd_cstft_plan *p, const T *x, const int64_t *off, const int64_t *len, int64_t nstreams,
             int64_t max_frames, float *out, float *etot) {
    using S = Csa<L>;
    auto kern = cstft_any_kernel<T, L>;
    if (S::LDS_BYTES > 0)
        if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(kern), S::LDS_BYTES)) return rc;
    const int64_t total = nstreams * max_frames;
    const int64_t ngroups = (total + S::F - 1) / S::F;
    // persistent: as many workgroups as stay resident, each a contiguous range of groups
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, S::TPB, S::LDS_BYTES) != hipSuccess || per_cu < 1)
        per_cu = 1;
    int64_t wgs = (int64_t)p->ctx->num_cu * per_cu - p->ctx->cstft_reserve;
    if (wgs < 1) wgs = 1;
    if (wgs > ngroups) wgs = ngroups;
    const int64_t per = (ngroups + wgs - 1) / wgs;
    wgs = (ngroups + per - 1) / per;
    KernelTimer timer(p->ctx, K_CSTFT);
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(S::TPB), S::LDS_BYTES, p->ctx->stream, x, off, len, max_frames,
                       total, ngroups, per, p->nperseg, p->hop, p->detrend, p->d_win.get(), p->d_tw.get(), out, etot,
                       msd_cstft_energy_stride(nstreams, max_frames));
    return MSD_OK;
}

template <typename T>
int launch_t(msd_cstft_plan *p, const T *x, const int64_t *off, const int64_t *len, int64_t nstreams,
             int64_t max_frames, float *out, float *etot) {
    switch (csa_log2(p->nfft)) {
        case 4: return launch_l<T, 4>(p, x, off, len, nstreams, max_frames, out, etot);
        case 5: return launch_l<T, 5>(p, x, off, len, nstreams, max_frames, out, etot);
        case 6: return launch_l<T, 6>(p, x, off, len, nstreams, max_frames, out, etot);
        case 7: return launch_l<T, 7>(p, x, off, len, nstreams, max_frames, out, etot);
        case 8: return launch_l<T, 8>(p, x, off, len, nstreams, max_frames, out, etot);
        case 9: return launch_l<T, 9>(p, x, off, len, nstreams, max_frames, out, etot);
        case 10: return launch_l<T, 10>(p, x, off, len, nstreams, max_frames, out, etot);
        case 11: return launch_l<T, 11>(p, x, off, len, nstreams, max_frames, out, etot);
        case 12: return launch_l<T, 12>(p, x, off, len, nstreams, max_frames, out, etot);
        case 13: return launch_l<T, 13>(p, x, off, len, nstreams, max_frames, out, etot);
        default: return fail(MSD_ERR_UNSUPPORTED, "cstft: nfft must be a power of two in [16, 8192]");
    }
}

}  // namespace

int launch_cstft_any(msd_cstft_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len,
                     int64_t nstreams, int64_t max_frames, float *out, float *etot) {
    const int rc = dtype == MSD_CI16
                       ? launch_t(p, static_cast<const int16_t *>(x), off, len, nstreams, max_frames, out, etot)
                       : launch_t(p, static_cast<const float *>(x), off, len, nstreams, max_frames, out, etot);
    if (rc) return rc;
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

}  // namespace msd

extern "C" int msd_cstft_chain(int32_t nperseg, int32_t nfft, double *chain) {
    using namespace msd;
    if (!chain) return fail(MSD_ERR_INVALID, "msd_cstft_chain: null");
    *chain = 0.0;
    const int L = csa_log2(nfft);
    if (L < 0) return fail(MSD_ERR_UNSUPPORTED, "msd_cstft_chain: nfft must be a power of two in [16, 8192]");
    if (nperseg < 1 || nperseg > nfft) return fail(MSD_ERR_INVALID, "msd_cstft_chain: need 1 <= nperseg <= nfft");
    *chain = nperseg == 4096 && nfft == 4096 ? CSTFT4096_CHAIN : cstft_any_chain(L);
    return MSD_OK;
}
