// Time-frequency burst clustering of the legacy spectrogram (meteor_detect_class/detector_and_classification.py:7-91):
//   spec_peaks_kernel  the points, in ORB's place (:12-16): the cells of the window above the colour floor, the
//                      max_points largest by (value descending, cell ascending) when there are more, in cell order;
//   cluster_kernel     DBSCAN(eps, min_samples).fit(points).labels_ (:20-21), the clusters' boxes (:44-46) and the
//                      critical rule (:48-50), exactly.
// One workgroup of 256 threads per image in both.  The contract, the LDS layout and a plain C++ restatement are in
// cluster_plan.h.  Built with -ffp-contract=off: dx dx + dy dy is two rounded products and one rounded sum.
//
// cluster_kernel.  A wave takes row i of the adjacency and its lanes 64 columns: one __ballot is a 64-bit word of the
// bitmask (512 x 512 bits in LDS), its popcount the neighbour count.  Components: every core point holds a label,
// initially its own index; a round lowers each label to the minimum over the point's core neighbours, hooks the old
// label's point to it as well, and then shortens label -> label[label] chains; labels only fall, never below the
// component's lowest index, and after k rounds a label is at most the lowest index within k hops, so at most n rounds
// run (a workgroup-wide "changed" flag in LDS ends them earlier).  A root is
// a core point that kept its own index; cluster ids are the roots' ranks, a prefix popcount of the root mask.
//
// spec_peaks_kernel.  A counting pass; where the count exceeds max_points, a radix select (8 passes of 8 bits, most
// significant first) on the order-preserving 64-bit key of the float64 finds the key V of the max_points-th largest
// and how many cells equal to V stay; an ordered compaction over the cells in index order (ballot + prefix popcount,
// two barriers per 256 cells) then keeps key > V, and the first of key == V.  The counting passes read along the
// frames (coalesced); the compaction reads in cell order, which is frame-major.
#include <cstring>

#include "cluster_plan.h"
#include "msd_internal.h"

namespace msd {
namespace {

using namespace cluster;

constexpr int NWAVES = THREADS / 64;
constexpr int NO_LABEL = 0x7fffffff;
static_assert(THREADS == PEAK_BINS, "one histogram bin per thread");
static_assert(MAX_POINTS % THREADS == 0, "whole passes over the points");

__global__ __launch_bounds__(THREADS) void cluster_kernel(const double *__restrict__ xy, const int32_t *__restrict__ npts,
                                                          int32_t n_one, int32_t max_points, double eps2,
                                                          int32_t min_samples, double min_extent,
                                                          int32_t *__restrict__ labels, double *__restrict__ boxes,
                                                          msd_cluster_summary *__restrict__ summary) {
    __shared__ double s_x[MAX_POINTS], s_y[MAX_POINTS];
    __shared__ unsigned long long s_adj[MAX_POINTS * ROW_WORDS];
    __shared__ int s_label[MAX_POINTS], s_id[MAX_POINTS];
    __shared__ unsigned long long s_core[WORDS], s_root[WORDS];
    __shared__ int s_changed[2], s_cnt[3];  // s_cnt: critical, non-critical, noise

    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = npts ? npts[m] : n_one;
    if (n < 0 || n > max_points) {  // uniform: nothing is clamped, the image is reported and left alone
        if (tid == 0) summary[m] = msd_cluster_summary{0, 0, 0, 0, MSD_CLUSTER_STATUS_NPTS, 0, {0, 0}};
        return;
    }
    const int nw = (n + 63) >> 6;
    const double *p = xy + m * max_points * 2;
    for (int i = tid; i < n; i += THREADS) {
        s_x[i] = p[2 * i];
        s_y[i] = p[2 * i + 1];
    }
    if (tid < 3) s_cnt[tid] = 0;
    if (tid < 2) s_changed[tid] = 0;
    __syncthreads();

    // adjacency rows and neighbour counts (the count waits in s_label)
    for (int i = wave; i < n; i += NWAVES) {
        const double xi = s_x[i], yi = s_y[i];
        unsigned long long mine = 0;
        int cnt = 0;
        for (int c = 0; c < nw; ++c) {
            const int j = c * 64 + lane;
            bool a = false;
            if (j < n) {
                const double dx = xi - s_x[j], dy = yi - s_y[j];
                a = (dx * dx + dy * dy) <= eps2;
            }
            const unsigned long long w = __ballot(a);
            cnt += __popcll(w);
            if (lane == c) mine = w;
        }
        if (lane < WORDS) s_adj[i * ROW_WORDS + lane] = mine;
        if (lane == 0) s_label[i] = cnt;
    }
    __syncthreads();
    for (int i = tid; i < MAX_POINTS; i += THREADS) {
        const bool c = i < n && s_label[i] >= min_samples;
        const unsigned long long w = __ballot(c);
        if (lane == 0) s_core[i >> 6] = w;
        if (i < n) s_label[i] = c ? i : NO_LABEL;
    }
    __syncthreads();

    // connected components of the core points
    // (relaxed atomic accesses on the arrays themselves: another thread lowers a label while this one reads it)
#define LDS_LOAD(a) __atomic_load_n(&(a), __ATOMIC_RELAXED)
#define LDS_STORE(a, v) __atomic_store_n(&(a), (v), __ATOMIC_RELAXED)
    for (int round = 0; round < n; ++round) {
        if (tid == 0) LDS_STORE(s_changed[(round + 1) & 1], 0);
        for (int i = tid; i < n; i += THREADS) {
            if (!((s_core[i >> 6] >> (i & 63)) & 1)) continue;
            const int old = LDS_LOAD(s_label[i]);
            int mn = old;
            for (int c = 0; c < nw; ++c) {
                unsigned long long w = s_adj[i * ROW_WORDS + c] & s_core[c];
                while (w) {
                    const int j = c * 64 + __builtin_ctzll(w);
                    w &= w - 1;
                    const int l = LDS_LOAD(s_label[j]);
                    mn = l < mn ? l : mn;
                }
            }
            if (mn < old) {
                atomicMin(&s_label[i], mn);
                atomicMin(&s_label[old], mn);
                LDS_STORE(s_changed[round & 1], 1);
            }
        }
        __syncthreads();
        if (!LDS_LOAD(s_changed[round & 1])) break;  // uniform
        for (int i = tid; i < n; i += THREADS) {
            if (!((s_core[i >> 6] >> (i & 63)) & 1)) continue;
            int l = LDS_LOAD(s_label[i]);
            for (;;) {
                const int ll = LDS_LOAD(s_label[l]);
                if (ll >= l) break;
                l = ll;
            }
            LDS_STORE(s_label[i], l);
        }
        __syncthreads();
    }

#undef LDS_LOAD
#undef LDS_STORE

    // roots, their ranks, and the core points' cluster ids
    for (int i = tid; i < MAX_POINTS; i += THREADS) {
        const bool r = i < n && s_label[i] == i;
        const unsigned long long w = __ballot(r);
        if (lane == 0) s_root[i >> 6] = w;
    }
    __syncthreads();
    int nclusters = 0;
    for (int c = 0; c < WORDS; ++c) nclusters += __popcll(s_root[c]);
    for (int i = tid; i < n; i += THREADS) {
        const int r = s_label[i];
        int id = -1;
        if (r != NO_LABEL) {
            id = __popcll(s_root[r >> 6] & ((1ull << (r & 63)) - 1));
            for (int c = 0; c < (r >> 6); ++c) id += __popcll(s_root[c]);
        }
        s_id[i] = id;
    }
    __syncthreads();
    // border points: the lowest id among the core neighbours (only core entries of s_id are read)
    for (int i = tid; i < n; i += THREADS) {
        if ((s_core[i >> 6] >> (i & 63)) & 1) continue;
        int best = NO_LABEL;
        for (int c = 0; c < nw; ++c) {
            unsigned long long w = s_adj[i * ROW_WORDS + c] & s_core[c];
            while (w) {
                const int j = c * 64 + __builtin_ctzll(w);
                w &= w - 1;
                const int l = s_id[j];
                best = l < best ? l : best;
            }
        }
        if (best != NO_LABEL) s_id[i] = best;
    }
    __syncthreads();

    for (int i = tid; i < MAX_POINTS; i += THREADS) {
        const bool noise = i < n && s_id[i] < 0;
        if (i < n) labels[m * max_points + i] = s_id[i];
        const unsigned long long w = __ballot(noise);
        if (lane == 0 && w) atomicAdd(&s_cnt[2], __popcll(w));
    }
    // boxes: a wave per cluster
    for (int k = wave; k < nclusters; k += NWAVES) {
        double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
        for (int c = 0; c < nw; ++c) {
            const int j = c * 64 + lane;
            if (j < n && s_id[j] == k) {
                const double x = s_x[j], y = s_y[j];
                x0 = x < x0 ? x : x0;
                y0 = y < y0 ? y : y0;
                x1 = x > x1 ? x : x1;
                y1 = y > y1 ? y : y1;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double a = __shfl_xor(x0, off), b = __shfl_xor(y0, off), c = __shfl_xor(x1, off),
                         d = __shfl_xor(y1, off);
            x0 = a < x0 ? a : x0;
            y0 = b < y0 ? b : y0;
            x1 = c > x1 ? c : x1;
            y1 = d > y1 ? d : y1;
        }
        if (lane == 0) {
            if (boxes) {
                double *b = boxes + (m * max_points + k) * 4;
                b[0] = x0, b[1] = y0, b[2] = x1, b[3] = y1;
            }
            atomicAdd(&s_cnt[(x1 - x0) >= min_extent ? 0 : 1], 1);
        }
    }
    __syncthreads();
    if (tid == 0) summary[m] = msd_cluster_summary{nclusters, s_cnt[0], s_cnt[1], s_cnt[2], 0, n, {0, 0}};
}

__device__ __forceinline__ unsigned long long peak_key_dev(double p) {
    if (p == 0.0) p = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(p);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(THREADS) void spec_peaks_kernel(const double *__restrict__ spec, int32_t K, int32_t frames,
                                                             int64_t ld, int32_t k_lo, int32_t nk,
                                                             const double *__restrict__ thr, double thr_one, double sx,
                                                             double sy, int32_t max_points, double *__restrict__ xy,
                                                             int32_t *__restrict__ cell, int32_t *__restrict__ npts,
                                                             int32_t *__restrict__ ncand) {
    __shared__ int s_hist[PEAK_BINS];
    __shared__ int s_wc[2][2][NWAVES];
    __shared__ int s_tot, s_remaining;
    __shared__ unsigned long long s_prefix;

    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *s = spec + (m * K + k_lo) * ld;
    const double th = thr ? thr[m] : thr_one;
    const int ncells = nk * frames;  // <= 2^31 - 1 (validated)
    if (tid == 0) s_tot = 0;
    __syncthreads();

    // candidates, read along the frames
    int cnt = 0;
    for (int64_t idx = tid; idx < ncells; idx += THREADS) {
        const int kk = (int)(idx / frames), t = (int)(idx - (int64_t)kk * frames);
        cnt += s[kk * ld + t] > th;
    }
    cnt = wave_sum_i(cnt);
    if (lane == 0 && cnt) atomicAdd(&s_tot, cnt);
    __syncthreads();
    const int total = s_tot;
    const bool cut = total > max_points;

    // the key of the max_points-th largest candidate and how many of its equals stay
    unsigned long long prefix = 0;
    int remaining = max_points;
    if (cut) {  // uniform
        for (int shift = 64 - PEAK_DIGIT_BITS; shift >= 0; shift -= PEAK_DIGIT_BITS) {
            s_hist[tid] = 0;
            __syncthreads();
            for (int64_t idx = tid; idx < ncells; idx += THREADS) {
                const int kk = (int)(idx / frames), t = (int)(idx - (int64_t)kk * frames);
                const double v = s[kk * ld + t];
                if (v > th) {
                    const unsigned long long key = peak_key_dev(v);
                    const int hi = shift + PEAK_DIGIT_BITS;
                    if (hi >= 64 || (key >> hi) == (prefix >> hi)) atomicAdd(&s_hist[(key >> shift) & (PEAK_BINS - 1)], 1);
                }
            }
            __syncthreads();
            if (wave == 0) {  // lane l holds digits 4 l .. 4 l + 3; suffix sums from the top digit down
                const int h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2],
                          h3 = s_hist[4 * lane + 3];
                const int sl = h0 + h1 + h2 + h3;
                int incl = sl;
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_down(incl, off);
                    if (lane + off < 64) incl += o;
                }
                const int above = incl - sl;
                if (above < remaining && remaining <= incl) {  // one lane
                    int cum = above, d = 3;
                    if (cum + h3 < remaining) {
                        cum += h3, d = 2;
                        if (cum + h2 < remaining) {
                            cum += h2, d = 1;
                            if (cum + h1 < remaining) cum += h1, d = 0;
                        }
                    }
                    s_prefix = prefix | ((unsigned long long)(4 * lane + d) << shift);
                    s_remaining = remaining - cum;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            remaining = s_remaining;
        }
    }

    // ordered compaction in cell order
    int run_eq = 0, run_keep = 0, par = 0;
    const unsigned long long below = (1ull << lane) - 1;
    double *oxy = xy + m * max_points * 2;
    int32_t *ocell = cell + m * max_points;
    for (int64_t base = 0; base < ncells; base += THREADS, par ^= 1) {
        const int64_t c = base + tid;
        bool gt = false, eq = false;
        int t = 0, kk = 0;
        if (c < ncells) {
            t = (int)(c / nk), kk = (int)(c - (int64_t)t * nk);
            const double v = s[kk * ld + t];
            if (v > th) {
                if (cut) {
                    const unsigned long long key = peak_key_dev(v);
                    gt = key > prefix, eq = key == prefix;
                } else {
                    gt = true;
                }
            }
        }
        const unsigned long long beq = __ballot(eq);
        if (lane == 0) s_wc[par][0][wave] = __popcll(beq);
        __syncthreads();
        int eq_before = run_eq + __popcll(beq & below), eq_all = 0;
        for (int w = 0; w < NWAVES; ++w) {
            const int v = s_wc[par][0][w];
            eq_before += w < wave ? v : 0;
            eq_all += v;
        }
        const bool keep = gt || (eq && eq_before < remaining);
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) s_wc[par][1][wave] = __popcll(bk);
        __syncthreads();
        int pos = run_keep + __popcll(bk & below), keep_all = 0;
        for (int w = 0; w < NWAVES; ++w) {
            const int v = s_wc[par][1][w];
            pos += w < wave ? v : 0;
            keep_all += v;
        }
        if (keep && pos < max_points) {
            oxy[2 * pos] = (double)t * sx;
            oxy[2 * pos + 1] = (double)kk * sy;
            ocell[pos] = (int32_t)c;
        }
        run_eq += eq_all;
        run_keep += keep_all;
    }
    if (tid == 0) {
        npts[m] = run_keep;
        ncand[m] = total;
    }
}

int launch_cluster(msd_ctx *ctx, const msd_cluster_cfg *cfg, const double *xy, const int32_t *npts, int32_t n_one,
                   int64_t nimg, int32_t *labels, double *boxes, msd_cluster_summary *summary) {
    KernelTimer timer(ctx, K_CLUSTER);
    hipLaunchKernelGGL(cluster_kernel, dim3((unsigned)nimg), dim3(THREADS), 0, ctx->stream, xy, npts, n_one,
                       cfg->max_points, cfg->eps * cfg->eps, cfg->min_samples, cfg->critical_min_extent, labels, boxes,
                       summary);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

int launch_peaks(msd_ctx *ctx, const double *spec, int64_t nimg, int32_t K, int64_t frames, int64_t ld, int32_t k_lo,
                 int32_t k_hi, const double *thr, double thr_one, double sx, double sy, int32_t max_points, double *xy,
                 int32_t *cell, int32_t *npts, int32_t *ncand) {
    KernelTimer timer(ctx, K_CLUSTER);
    hipLaunchKernelGGL(spec_peaks_kernel, dim3((unsigned)nimg), dim3(THREADS), 0, ctx->stream, spec, K, (int32_t)frames,
                       ld, k_lo, k_hi - k_lo + 1, thr, thr_one, sx, sy, max_points, xy, cell, npts, ncand);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

}  // namespace
}  // namespace msd

using namespace msd;

extern "C" {

int msd_spec_peaks_f64_dev(msd_ctx *ctx, const double *spec, int64_t nimg, int32_t K, int64_t frames, int64_t ld,
                           int32_t k_lo, int32_t k_hi, const double *thr, double sx, double sy, int32_t max_points,
                           double *xy, int32_t *cell, int32_t *npts, int32_t *ncand) {
    const char *msg = "";
    if (int rc = cluster::validate_peaks(K, frames, ld, k_lo, k_hi, sx, sy, max_points, &msg))
        return fail(rc, std::string("msd_spec_peaks_f64_dev: ") + msg);
    if (!ctx || nimg < 0 || (nimg > 0 && (!spec || !thr || !xy || !cell || !npts || !ncand)))
        return fail(MSD_ERR_INVALID, "msd_spec_peaks_f64_dev: null or negative argument");
    if (nimg == 0) return MSD_OK;
    if (nimg > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, "msd_spec_peaks_f64_dev: too many images");
    DeviceGuard g(ctx->device);
    return launch_peaks(ctx, spec, nimg, K, frames, ld, k_lo, k_hi, thr, 0.0, sx, sy, max_points, xy, cell, npts, ncand);
}

int msd_cluster_dev(msd_ctx *ctx, const msd_cluster_cfg *cfg, const double *xy, const int32_t *npts, int64_t nimg,
                    int32_t *labels, double *boxes, msd_cluster_summary *summary) {
    const char *msg = "";
    if (int rc = cluster::validate(cfg, &msg)) return fail(rc, std::string("msd_cluster_dev: ") + msg);
    if (!ctx || nimg < 0 || (nimg > 0 && (!xy || !npts || !labels || !summary)))
        return fail(MSD_ERR_INVALID, "msd_cluster_dev: null or negative argument");
    if (nimg == 0) return MSD_OK;
    if (nimg > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, "msd_cluster_dev: too many images");
    DeviceGuard g(ctx->device);
    return launch_cluster(ctx, cfg, xy, npts, 0, nimg, labels, boxes, summary);
}

int msd_spec_peaks_f64(msd_ctx *ctx, const double *spec, int32_t K, int64_t frames, int32_t k_lo, int32_t k_hi,
                       double thr, double sx, double sy, int32_t max_points, double *xy, int32_t *cell, int32_t *npts,
                       int32_t *ncand) {
    const char *msg = "";
    if (int rc = cluster::validate_peaks(K, frames, frames, k_lo, k_hi, sx, sy, max_points, &msg))
        return fail(rc, std::string("msd_spec_peaks_f64: ") + msg);
    if (!ctx || (!spec && frames) || !xy || !cell || !npts)
        return fail(MSD_ERR_INVALID, "msd_spec_peaks_f64: null argument");
    DeviceGuard g(ctx->device);
    const size_t in_bytes = (size_t)K * (size_t)frames * sizeof(double);
    void *din = nullptr, *dout = nullptr;
    if (int rc = ctx_scratch(ctx, SCRATCH_SAMPLES, (in_bytes + 255) / 256 * 256, &din)) return rc;
    const size_t xy_bytes = (size_t)max_points * 2 * sizeof(double), cell_bytes = (size_t)max_points * sizeof(int32_t);
    if (int rc = ctx_scratch(ctx, SCRATCH_OUTPUT, xy_bytes + cell_bytes + 16, &dout)) return rc;
    double *dxy = static_cast<double *>(dout);
    int32_t *dcell = reinterpret_cast<int32_t *>(static_cast<char *>(dout) + xy_bytes);
    int32_t *dcnt = dcell + max_points;
    if (in_bytes) MSD_HIP(hipMemcpyAsync(din, spec, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_peaks(ctx, static_cast<const double *>(din), 1, K, frames, frames, k_lo, k_hi, nullptr, thr, sx,
                              sy, max_points, dxy, dcell, dcnt, dcnt + 1))
        return rc;
    std::vector<char> host(xy_bytes + cell_bytes + 8);
    MSD_HIP(hipMemcpyAsync(host.data(), dout, host.size(), hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    int32_t cnt[2];
    std::memcpy(cnt, host.data() + xy_bytes + cell_bytes, sizeof cnt);
    if (cnt[0] < 0 || cnt[0] > max_points) return fail(MSD_ERR_HIP, "msd_spec_peaks_f64: bad point count");
    std::memcpy(xy, host.data(), (size_t)cnt[0] * 2 * sizeof(double));
    std::memcpy(cell, host.data() + xy_bytes, (size_t)cnt[0] * sizeof(int32_t));
    *npts = cnt[0];
    if (ncand) *ncand = cnt[1];
    return MSD_OK;
}

int msd_cluster(msd_ctx *ctx, const msd_cluster_cfg *cfg, const double *xy, int32_t n, int32_t *labels, double *boxes,
                msd_cluster_summary *summary) {
    const char *msg = "";
    if (int rc = cluster::validate(cfg, &msg)) return fail(rc, std::string("msd_cluster: ") + msg);
    if (n > cfg->max_points) return fail(MSD_ERR_UNSUPPORTED, "msd_cluster: n above max_points");
    if (!ctx || n < 0 || (n > 0 && (!xy || !labels)) || !summary)
        return fail(MSD_ERR_INVALID, "msd_cluster: null or negative argument");
    for (int64_t i = 0; i < 2 * (int64_t)n; ++i)
        if (!std::isfinite(xy[i])) return fail(MSD_ERR_INVALID, "msd_cluster: points must be finite");
    DeviceGuard g(ctx->device);
    const int32_t mp = cfg->max_points;
    const size_t xy_bytes = (size_t)mp * 2 * sizeof(double), box_bytes = (size_t)mp * 4 * sizeof(double),
                 lab_bytes = ((size_t)mp * sizeof(int32_t) + 7) / 8 * 8;
    void *din = nullptr, *dout = nullptr;
    if (int rc = ctx_scratch(ctx, SCRATCH_SAMPLES, xy_bytes, &din)) return rc;
    if (int rc = ctx_scratch(ctx, SCRATCH_OUTPUT, box_bytes + lab_bytes + sizeof(msd_cluster_summary), &dout)) return rc;
    double *dbox = static_cast<double *>(dout);
    int32_t *dlab = reinterpret_cast<int32_t *>(static_cast<char *>(dout) + box_bytes);
    msd_cluster_summary *dsum = reinterpret_cast<msd_cluster_summary *>(static_cast<char *>(dout) + box_bytes + lab_bytes);
    if (n) MSD_HIP(hipMemcpyAsync(din, xy, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_cluster(ctx, cfg, static_cast<const double *>(din), nullptr, n, 1, dlab, dbox, dsum)) return rc;
    std::vector<char> host(box_bytes + lab_bytes + sizeof(msd_cluster_summary));
    MSD_HIP(hipMemcpyAsync(host.data(), dout, host.size(), hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(summary, host.data() + box_bytes + lab_bytes, sizeof *summary);
    if (summary->status != 0 || summary->n_clusters < 0 || summary->n_clusters > n)
        return fail(MSD_ERR_HIP, "msd_cluster: bad summary");
    if (n) std::memcpy(labels, host.data() + box_bytes, (size_t)n * sizeof(int32_t));
    if (boxes && summary->n_clusters) std::memcpy(boxes, host.data(), (size_t)summary->n_clusters * 4 * sizeof(double));
    return MSD_OK;
}

}  // extern "C"
