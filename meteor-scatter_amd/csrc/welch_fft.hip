// The whole one-sided Welch PSD of every processing block, float64: scipy.signal.welch(block, fs,
// nperseg=, noverlap=, nfft=) -- periodic Hann, constant detrend, density scaling, mean over the
// segments -- for all K = nfft/2 + 1 bins, and np.mean(10 log10(row)) per block (the reference's
// local_wf_db_data rows and block_current_psd_db_mean, processor.py:206-229, :448).
// welch_bands_kernel (live.hip) runs one Goertzel recurrence per bin: right for the detector's 309
// band bins, 2049 x 256 x 5 recurrence steps per block for the whole band.  Here each segment goes
// through a pruned FFT.
//
// Factorisation (welch_fft_plan.h): the segment's nperseg values are followed by zeros up to nfft.
// With Lp = min(nperseg rounded up to a power of two, nfft / 2) and R = nfft / Lp, bin r + R q is bin q
// of the Lp-point complex transform of y_r[n] = v[n] W_nfft^{n r} (plus the folded second half where
// nperseg > nfft / 2), and the real input needs r = 0 .. R/2 only: R/2 + 1 transforms of Lp points, no
// pass over the padding.  Chosen over packing two real points into one complex point of a full
// nfft / 2-point transform (stft_any.hip): that one runs log2(nfft / 2) levels over nfft / 2 points whatever
// nperseg is, 11 x 2048 at the live default against 8 x 9 x 256 here, and its real split is one more
// rounded twiddle product per bin; the modulation costs one real-by-complex product per point.
//
// Arithmetic per segment, in this order: sample (float64) times sample_scale; minus the segment mean,
// taken in two parts as stft_any.hip does (mean, then the mean of the residual: exact for a
// constant, and no residue of a large offset under a small variation); times the window; the
// transform; |X|^2 scale, doubled on bins 1 .. nfft/2 - 1; segment powers summed in segment order, then
// divided by nseg (scipy's mean(axis=-1), as welch_bands_kernel does it).
//
// Mapping: one workgroup per block, in two kernels chosen by the plan's shape alone (so a block's row
// never depends on the launch).  Short shapes, the live default among them: welch_fft_wave_kernel, one
// wave per sub-transform (described at the kernel).  Every other shape: welch_fft_kernel, 256 threads
// over rounds of sub-transforms.  Its LDS: the row's K accumulators (8 K bytes), and two
// ping-pong buffers of G sub-transforms (32 G Lp bytes), G chosen so that a round's butterflies fill
// the workgroup: G Lp <= 1024 points, 4 x 256 at the live default -- 48 KB, three workgroups per CU.
// Per segment: the two detrend sums (samples read from global memory, L2 hits after the first
// segment), then rounds of G sub-transforms: modulated points into LDS (the samples and the window
// are read again from the caches and centred again: the same arithmetic, so the same values), the
// Stockham passes with a barrier each, then every owned output's power into its accumulator -- each
// bin has one owner, and the barriers order the segments.  Lp >= 2048 has one sub-transform per round;
// where two buffers and the accumulators exceed the LDS the passes run in place (read to registers,
// barrier, write), and at Lp = 8192 (128 KB) the accumulators are the output row itself in global
// memory.  A block's row depends on its samples and the plan alone: one workgroup, a fixed order.
// Bytes per block: 2 block_size in (int16), 8 K + 8 out.
#include <cmath>

#include "msd_internal.h"
#include "welch_fft_plan.h"

#pragma clang fp contract(off)

namespace msd {
namespace {

using wfft::cd;

constexpr int WF_THREADS = 256;
constexpr int WF_ROUND_POINTS = 1024;       // G Lp of a round (at least one sub-transform)
constexpr int WF_LDS_MAX = 150 * 1024;      // dynamic LDS a workgroup may ask for
constexpr int WF_INPLACE_MAX = 32;          // points per thread of an in-place pass (Lp 8192)

struct WfArgs {
    int64_t nfiles, max_blocks, ld;
    int block_size, step, nseg, G;
    double sample_scale, scale;
    wfft::Plan P;
};

// the workgroup's sum of v in a fixed order, the same value in every thread
__device__ __forceinline__ double wf_block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double tot = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();  // red is free again
    return tot;
}

template <int RDX>
__device__ __forceinline__ void wf_pass(const cd *src, cd *dst, const cd *__restrict__ W, const wfft::Plan &P, int G,
                                        int Ns) {
    const int lg = P.logLp - (RDX == 4 ? 2 : 1), nbf = 1 << lg;  // butterflies per sub-transform
    for (int i = threadIdx.x; i < G * nbf; i += WF_THREADS) {
        const int g = i >> lg, j = i & (nbf - 1);
        wfft::butterfly<RDX>(src + g * P.Lp, dst + g * P.Lp, W, P.Lp, P.nfft, Ns, j);
    }
}

// the same pass of one sub-transform in place: every thread reads its butterflies' inputs, the
// workgroup synchronises, then writes
template <int RDX>
__device__ __forceinline__ void wf_pass_inplace(cd *buf, const cd *__restrict__ W, const wfft::Plan &P, int Ns) {
    constexpr int NB = WF_INPLACE_MAX / RDX;
    const int nbf = P.Lp / RDX;
    cd v[NB][RDX];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = threadIdx.x + b * WF_THREADS;
        if (j < nbf) wfft::bf_read<RDX>(buf, P.Lp, j, v[b]);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = threadIdx.x + b * WF_THREADS;
        if (j >= nbf) continue;
        wfft::bf_compute<RDX>(v[b], W, P.nfft, Ns, j);
        wfft::bf_write<RDX>(buf, Ns, j, v[b]);
    }
}

// INPLACE: one buffer of one sub-transform; ACCG: the accumulators are the output row
template <typename T, bool INPLACE, bool ACCG>
__global__ __launch_bounds__(WF_THREADS) void welch_fft_kernel(const T *__restrict__ x,
                                                               const int64_t *__restrict__ off,
                                                               const int64_t *__restrict__ len, WfArgs A,
                                                               const double *__restrict__ g_win,
                                                               const cd *__restrict__ W, double *__restrict__ psd,
                                                               double *__restrict__ db_mean) {
    extern __shared__ __attribute__((aligned(16))) char wf_smem[];
    __shared__ double red[WF_THREADS / 64];
    const wfft::Plan &P = A.P;
    const int64_t gb = blockIdx.x;
    const int64_t f = gb / A.max_blocks, b = gb - f * A.max_blocks;
    if (f >= A.nfiles) return;
    const int64_t n = len[f];
    const int64_t nb = n >= A.block_size ? (n - A.block_size) / A.block_size + 1 : 0;
    if (b >= nb) return;  // whole workgroup
    const int G = INPLACE ? 1 : A.G;
    cd *bufA = reinterpret_cast<cd *>(wf_smem);
    cd *bufB = INPLACE ? bufA : bufA + G * P.Lp;
    const int64_t ri = f * A.ld + b;  // the block's row
    double *row = psd + ri * (int64_t)P.K;
    double *acc = ACCG ? row : reinterpret_cast<double *>(bufA + (INPLACE ? 1 : 2) * G * P.Lp);
    const T *xb = x + off[f] + b * (int64_t)A.block_size;
    const int L = P.nperseg;
    const double dL = (double)L;

    for (int s = 0; s < A.nseg; ++s) {
        const T *xs = xb + (int64_t)s * A.step;
        double t = 0.0;
        for (int i = threadIdx.x; i < L; i += WF_THREADS) t += (double)xs[i] * A.sample_scale;
        const double mean = wf_block_sum(t, red) / dL;
        t = 0.0;
        for (int i = threadIdx.x; i < L; i += WF_THREADS) t += (double)xs[i] * A.sample_scale - mean;
        const double mlo = wf_block_sum(t, red) / dL;
        auto v = [&](int i) -> double {  // window times the detrended sample; 0 past the segment
            return i < L ? g_win[i] * (((double)xs[i] * A.sample_scale - mean) - mlo) : 0.0;
        };
        for (int r0 = 0; r0 < P.nsub; r0 += G) {
            for (int i = threadIdx.x; i < G * P.Lp; i += WF_THREADS) {
                const int g = i >> P.logLp, m = i & (P.Lp - 1), r = r0 + g;
                cd y{0.0, 0.0};
                if (r < P.nsub) y = wfft::modulated(P, r, v(m), P.fold ? v(m + P.Lp) : 0.0, W[wfft::mod_index(P, r, m)]);
                bufA[i] = y;
            }
            __syncthreads();
            cd *src = bufA, *dst = bufB;
            for (int p = 0; p < P.npass; ++p) {
                const int Ns = wfft::pass_ns(P, p);
                if constexpr (INPLACE) {
                    if (wfft::pass_radix(P, p) == 2) wf_pass_inplace<2>(bufA, W, P, Ns);
                    else wf_pass_inplace<4>(bufA, W, P, Ns);
                } else {
                    if (wfft::pass_radix(P, p) == 2) wf_pass<2>(src, dst, W, P, G, Ns);
                    else wf_pass<4>(src, dst, W, P, G, Ns);
                    cd *tmp = src;
                    src = dst;
                    dst = tmp;
                }
                __syncthreads();
            }
            for (int i = threadIdx.x; i < G * P.Lp; i += WF_THREADS) {
                const int g = i >> P.logLp, q = i & (P.Lp - 1), r = r0 + g;
                if (r >= P.nsub) continue;
                const int bin = wfft::owned_bin(P, r, q);
                if (bin < 0) continue;
                const double pw = wfft::bin_power(P, bin, src[i], A.scale);
                acc[bin] = s == 0 ? pw : acc[bin] + pw;  // Pxy.mean(axis=-1): segments in order
            }
            __syncthreads();  // the next round refills bufA; the next segment adds to acc
        }
    }
    double lsum = 0.0;
    for (int k = threadIdx.x; k < P.K; k += WF_THREADS) {
        const double pv = acc[k] / (double)A.nseg;
        row[k] = pv;
        lsum += 10.0 * log10(pv);  // log10(0) = -inf, as numpy's
    }
    if (db_mean) {  // (uniform)
        const double tot = wf_block_sum(lsum, red);
        if (threadIdx.x == 0) db_mean[ri] = tot / (double)P.K;
    }
}

// The short shapes (Lp <= 256, the block, its window and the row's accumulators within WFW_LDS_MAX of
// LDS, at most WFW_MAX_SEG segments: the live default among them): one wave per sub-transform, so that
// nothing but the wave's own LDS traffic lies between two steps of a transform.  The block's samples
// (float64, scaled), the window and the Lp roots W_Lp^j are staged once, the segments' two-part means
// are taken wave by wave (shuffles), then wave w runs sub-transforms r = w, w + NW, ...: its
// modulation factors stay in registers over the segments, each lane owns at most one butterfly of
// every pass (read, wave barrier, write: in place in the wave's Lp points) and the same outputs in
// every segment, whose powers it adds to the accumulators in segment order.  The accumulators are laid
// out by (sub-transform, output), [R/2 + 1][Lp + 1], not by bin: a wave's 64 outputs q, q + 1, ... are
// the bins r + R q, 8 R bytes apart, which by bin would fall into one or two LDS banks (32-way conflicts
// at R = 16); the odd row length keeps the final pass over the bins, which walks r fastest, off a
// single bank too.  No workgroup barrier
// between the staging and the final division.  NW = blockDim.x / 64 is 1 .. 4, chosen to waste the
// fewest wave slots over the R/2 + 1 sub-transforms (3 for the live default's 9).
constexpr int WFW_MAX_LP = 256, WFW_MAX_SEG = 64, WFW_LDS_MAX = 52 * 1024;

template <int RDX>
__device__ __forceinline__ void wfw_pass(cd *buf, const cd *tw, int Lp, int Ns, int lane) {
    const bool mine = lane < Lp / RDX;
    cd v[RDX];
    if (mine) {
        wfft::bf_read<RDX>(buf, Lp, lane, v);
        wfft::bf_compute<RDX>(v, tw, Lp, Ns, lane);  // W_Lp^j = W_nfft^{R j}: the general kernel's twiddles
    }
    wave_sync();  // every lane has read its inputs
    if (mine) wfft::bf_write<RDX>(buf, Ns, lane, v);
    wave_sync();
}

template <typename T>
__global__ __launch_bounds__(WF_THREADS) void welch_fft_wave_kernel(const T *__restrict__ x,
                                                                    const int64_t *__restrict__ off,
                                                                    const int64_t *__restrict__ len, WfArgs A,
                                                                    const double *__restrict__ g_win,
                                                                    const cd *__restrict__ W, double *__restrict__ psd,
                                                                    double *__restrict__ db_mean) {
    extern __shared__ __attribute__((aligned(16))) char wf_smem[];
    __shared__ double red[WF_THREADS / 64];
    const wfft::Plan &P = A.P;
    const int64_t gb = blockIdx.x;
    const int64_t f = gb / A.max_blocks, b = gb - f * A.max_blocks;
    if (f >= A.nfiles) return;
    const int64_t n = len[f];
    const int64_t nb = n >= A.block_size ? (n - A.block_size) / A.block_size + 1 : 0;
    if (b >= nb) return;  // whole workgroup
    const int NW = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = P.nperseg, Lp = P.Lp;
    cd *tw = reinterpret_cast<cd *>(wf_smem);          // [Lp] W_Lp^j
    cd *buf = tw + Lp + wave * Lp;                     // [NW][Lp] the waves' transforms
    double *acc = reinterpret_cast<double *>(tw + (1 + NW) * Lp);  // [nsub][Lp + 1] by (sub-transform, output)
    const int ars = Lp + 1;
    double *xs = acc + P.nsub * ars;                   // [block_size] samples times sample_scale
    double *win = xs + A.block_size;                   // [nperseg]
    double *smean = win + L;                           // [nseg][2] mean, mean of the residual
    const int64_t ri = f * A.ld + b;  // the block's row
    double *row = psd + ri * (int64_t)P.K;
    const T *xb = x + off[f] + b * (int64_t)A.block_size;
    for (int i = threadIdx.x; i < A.block_size; i += blockDim.x) xs[i] = (double)xb[i] * A.sample_scale;
    for (int i = threadIdx.x; i < L; i += blockDim.x) win[i] = g_win[i];
    for (int i = threadIdx.x; i < Lp; i += blockDim.x) tw[i] = W[i * P.R];
    __syncthreads();
    const double dL = (double)L;
    for (int s = wave; s < A.nseg; s += NW) {
        const double *sx = xs + s * A.step;
        double t = 0.0;
        for (int i = lane; i < L; i += 64) t += sx[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
        const double mean = t / dL;
        t = 0.0;
        for (int i = lane; i < L; i += 64) t += sx[i] - mean;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
        if (lane == 0) smean[2 * s] = mean, smean[2 * s + 1] = t / dL;
    }
    __syncthreads();
    constexpr int PT = WFW_MAX_LP / 64;  // points per lane
    for (int r = wave; r < P.nsub; r += NW) {
        cd wm[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int m = lane + 64 * j;
            wm[j] = W[wfft::mod_index(P, r, m < Lp ? m : 0)];
        }
        for (int s = 0; s < A.nseg; ++s) {
            const double *sx = xs + s * A.step;
            const double mean = smean[2 * s], mlo = smean[2 * s + 1];
            auto v = [&](int i) -> double { return i < L ? win[i] * ((sx[i] - mean) - mlo) : 0.0; };
            cd y[PT];  // every read before the first write: the LDS reads go out together
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int m = lane + 64 * j;
                y[j] = wfft::modulated(P, r, v(m), P.fold ? v(m + Lp) : 0.0, wm[j]);
            }
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int m = lane + 64 * j;
                if (m < Lp) buf[m] = y[j];
            }
            wave_sync();
            for (int p = 0; p < P.npass; ++p) {
                const int Ns = wfft::pass_ns(P, p);
                if (wfft::pass_radix(P, p) == 2) wfw_pass<2>(buf, tw, Lp, Ns, lane);
                else wfw_pass<4>(buf, tw, Lp, Ns, lane);
            }
            double pw[PT];
            bool own[PT];
            double *ar = acc + r * ars;
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int q = lane + 64 * j;
                const int bin = q < Lp ? wfft::owned_bin(P, r, q) : -1;
                own[j] = bin >= 0;
                pw[j] = 0.0;
                if (own[j]) {
                    pw[j] = wfft::bin_power(P, bin, buf[q], A.scale);
                    if (s > 0) pw[j] = ar[q] + pw[j];  // this lane's bin in every segment, in order
                }
            }
#pragma unroll
            for (int j = 0; j < PT; ++j)
                if (own[j]) ar[lane + 64 * j] = pw[j];
            wave_sync();  // the next segment refills buf
        }
    }
    __syncthreads();
    double lsum = 0.0;
    for (int k = threadIdx.x; k < P.K; k += blockDim.x) {
        int r, q;
        wfft::bin_source(P, k, r, q);
        const double pv = acc[r * ars + q] / (double)A.nseg;
        row[k] = pv;
        lsum += 10.0 * log10(pv);
    }
    if (db_mean) {  // (uniform)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
        if (lane == 0) red[wave] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = red[0];
            for (int w = 1; w < NW; ++w) tot += red[w];
            db_mean[ri] = tot / (double)P.K;
        }
    }
}

// the wave kernel's workgroup: waves (0: the shape does not take it) and dynamic LDS
int wfw_shape(const wfft::Plan &P, int block_size, int nseg, size_t *lds) {
    if (P.Lp > WFW_MAX_LP || nseg > WFW_MAX_SEG) return 0;
    int best = 0, waste = 1 << 30;
    for (int nw = 4; nw >= 1; --nw) {
        const int w = (P.nsub + nw - 1) / nw * nw - P.nsub;
        if (w < waste) best = nw, waste = w;
    }
    *lds = sizeof(cd) * (size_t)P.Lp * (size_t)(1 + best) +
           sizeof(double) * ((size_t)P.nsub * (size_t)(P.Lp + 1) + (size_t)block_size + (size_t)P.nperseg + 2 * (size_t)nseg);
    return *lds <= (size_t)WFW_LDS_MAX ? best : 0;
}

template <typename T>
int launch_spectrum_t(msd_welch_plan *p, const void *x, const int64_t *off, const int64_t *len, int64_t nfiles,
                      int64_t max_blocks, double *psd, int64_t ld, double *db_mean) {
    const msd_welch_cfg &c = p->cfg;
    WfArgs A{};
    A.nfiles = nfiles;
    A.max_blocks = max_blocks;
    A.ld = ld;
    A.block_size = c.block_size;
    A.step = p->step;
    A.nseg = p->nseg;
    A.sample_scale = c.sample_scale;
    A.scale = c.scale;
    A.P = p->fft;
    const wfft::Plan &P = A.P;
    const int64_t grid = nfiles * max_blocks;
    if (grid > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, "welch spectrum: grid too large");
    size_t wlds = 0;
    if (const int nw = wfw_shape(P, c.block_size, p->nseg, &wlds)) {  // by the plan's shape alone
        if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(welch_fft_wave_kernel<T>), WFW_LDS_MAX)) return rc;
        KernelTimer timer(p->ctx, K_WSPEC);
        hipLaunchKernelGGL(welch_fft_wave_kernel<T>, dim3((unsigned)grid), dim3(64 * nw), wlds, p->ctx->stream,
                           static_cast<const T *>(x), off, len, A, p->d_window.get(),
                           reinterpret_cast<const cd *>(p->d_roots.get()), psd, db_mean);
        MSD_HIP(hipGetLastError());
        return MSD_OK;
    }
    int G = WF_ROUND_POINTS / P.Lp;
    G = G < 1 ? 1 : (G > P.nsub ? P.nsub : G);
    const size_t acc_bytes = sizeof(double) * (size_t)P.K, tr = sizeof(cd) * (size_t)P.Lp;
    const bool inplace = 2 * G * tr + acc_bytes > (size_t)WF_LDS_MAX;
    if (inplace && (G != 1 || P.Lp > WF_INPLACE_MAX * WF_THREADS))
        return fail(MSD_ERR_UNSUPPORTED, "welch spectrum: sub-transform too long for one workgroup");
    const bool accg = inplace && tr + acc_bytes > (size_t)WF_LDS_MAX;
    A.G = G;
    const size_t lds = (inplace ? tr : 2 * G * tr) + (accg ? 0 : acc_bytes);
    if (lds > (size_t)WF_LDS_MAX) return fail(MSD_ERR_UNSUPPORTED, "welch spectrum: LDS budget exceeded");
    auto kern = !inplace ? welch_fft_kernel<T, false, false>
                         : (accg ? welch_fft_kernel<T, true, true> : welch_fft_kernel<T, true, false>);
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(kern), WF_LDS_MAX)) return rc;
    KernelTimer timer(p->ctx, K_WSPEC);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WF_THREADS), lds, p->ctx->stream, static_cast<const T *>(x), off,
                       len, A, p->d_window.get(), reinterpret_cast<const cd *>(p->d_roots.get()), psd, db_mean);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

}  // namespace

int welch_spectrum_prepare(msd_welch_plan *p) {
    if (p->fft_state > 0) return MSD_OK;
    if (p->fft_state < 0 || !wfft::make_plan(p->cfg.nperseg, p->cfg.nfft, p->fft)) {
        p->fft_state = -1;
        return fail(MSD_ERR_UNSUPPORTED, "welch spectrum: nfft must be a power of two in [16, 16384], nperseg <= nfft");
    }
    std::vector<cd> roots((size_t)p->cfg.nfft);
    wfft::unit_roots(p->cfg.nfft, roots.data());
    static_assert(sizeof(cd) == sizeof(double2), "cd is a double2");
    if (int rc = p->d_roots.upload(reinterpret_cast<const double2 *>(roots.data()), roots.size(), "welch spectrum"))
        return rc;
    p->fft_state = 1;
    return MSD_OK;
}

int launch_welch_spectrum(msd_welch_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len,
                          int64_t nfiles, int64_t max_blocks, double *psd, int64_t ld, double *db_mean) {
    if (int rc = welch_spectrum_prepare(p)) return rc;
    if (nfiles == 0 || max_blocks == 0) return MSD_OK;
    switch (dtype) {
        case MSD_U8: return launch_spectrum_t<uint8_t>(p, x, off, len, nfiles, max_blocks, psd, ld, db_mean);
        case MSD_I16: return launch_spectrum_t<int16_t>(p, x, off, len, nfiles, max_blocks, psd, ld, db_mean);
        case MSD_I32: return launch_spectrum_t<int32_t>(p, x, off, len, nfiles, max_blocks, psd, ld, db_mean);
        case MSD_F32: return launch_spectrum_t<float>(p, x, off, len, nfiles, max_blocks, psd, ld, db_mean);
        case MSD_F64: return launch_spectrum_t<double>(p, x, off, len, nfiles, max_blocks, psd, ld, db_mean);
        default: return fail(MSD_ERR_INVALID, "welch spectrum: unknown dtype");
    }
}

}  // namespace msd

using namespace msd;

extern "C" {

int msd_welch_spectrum_dev(msd_welch_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len,
                           int64_t nfiles, int64_t max_blocks, double *psd, int64_t ld, double *db_mean) {
    if (!p || (nfiles > 0 && max_blocks > 0 && (!x || !off || !len || !psd)))
        return fail(MSD_ERR_INVALID, "msd_welch_spectrum_dev: null");
    if (nfiles < 0 || max_blocks < 0 || ld < max_blocks) return fail(MSD_ERR_INVALID, "msd_welch_spectrum_dev: ld < max_blocks");
    DeviceGuard g(p->ctx->device);
    return launch_welch_spectrum(p, x, dtype, off, len, nfiles, max_blocks, psd, ld, db_mean);
}

int msd_welch_spectrum(msd_welch_plan *p, const void *x, int dtype, int64_t n, double *psd, double *db_mean,
                       int64_t *blocks) {
    if (!p || (!x && n) || n < 0) return fail(MSD_ERR_INVALID, "msd_welch_spectrum: null");
    const size_t es = dtype_size(dtype);
    if (!es) return fail(MSD_ERR_INVALID, "msd_welch_spectrum: unknown dtype");
    msd_ctx *ctx = p->ctx;
    DeviceGuard g(ctx->device);
    int rc;
    if ((rc = welch_spectrum_prepare(p))) return rc;  // an unsupported shape, whatever n is
    const int64_t B = p->cfg.block_size;
    const int64_t nb = n >= B ? (n - B) / B + 1 : 0;
    if (blocks) *blocks = nb;
    if (nb == 0) return MSD_OK;
    if (!psd) return fail(MSD_ERR_INVALID, "msd_welch_spectrum: null psd");
    const void *dx;
    const int64_t *doff;
    void *dout;
    const size_t K = (size_t)p->fft.K, psd_bytes = sizeof(double) * K * (size_t)nb, db_bytes = sizeof(double) * (size_t)nb;
    if ((rc = stage_one_file(ctx, x, (size_t)n * es, n, &dx, &doff))) return rc;
    if ((rc = ctx_scratch(ctx, SCRATCH_OUTPUT, psd_bytes + db_bytes, &dout))) return rc;
    double *dpsd = static_cast<double *>(dout), *ddb = dpsd + K * (size_t)nb;
    if ((rc = launch_welch_spectrum(p, dx, dtype, doff, doff + 1, 1, nb, dpsd, nb, ddb))) return rc;
    MSD_HIP(hipMemcpyAsync(psd, dpsd, psd_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (db_mean) MSD_HIP(hipMemcpyAsync(db_mean, ddb, db_bytes, hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    return MSD_OK;
}

}  // extern "C"
