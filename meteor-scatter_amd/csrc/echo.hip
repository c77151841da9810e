// Echo measurement (include/msdsp.h a12): one 128-byte record per detection from the device-resident
// one-sided spectrogram and the detector's device-resident detections, no host round trip.
//
// Mapping.  One wave per detection, lanes along frames: a spectrogram row is contiguous in t, so the 64
// lanes of a wave read 64 consecutive cells of each band row (coalesced), and each lane walks its column's
// few band rows in ascending k exactly as the contract states the sums.  A workgroup holds WAVES waves;
// blockIdx.x is the file and the waves of its up to MAX_GRID_Y workgroups stride over the file's stored
// detections, so the grid depends on nfiles and cap alone and a file with few detections costs a few idle
// waves, not cap of them.  Pass 1 gives each lane its frames' S, N, k*, delta: the lane keeps its best frame
// and its share of the six sums, and 64-lane shuffle reductions finish them, the peak on (value descending,
// frame ascending).  Pass 2 needs the peak: it recomputes S_t with the same ascending-k sum (the same bits)
// from cells that are in L2 by then, and reduces the three threshold frames by min / max.  No LDS, no
// scratch, no atomics; the only stores are the records.
#include <cstring>
#include <vector>

#include "echo_plan.h"
#include "msd_internal.h"

namespace msd {
namespace {

using namespace echo;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min64(v, (int64_t)__shfl_xor((long long)v, o, 64));
    return v;
}
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max64(v, (int64_t)__shfl_xor((long long)v, o, 64));
    return v;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void echo_kernel(const T *__restrict__ spec, int32_t K,
                                                       const int64_t *__restrict__ frames, int64_t ld,
                                                       const msd_det *__restrict__ dets, int64_t cap,
                                                       const int64_t *__restrict__ counts, msd_echo_cfg c,
                                                       msd_echo *__restrict__ out) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = min64(max64(counts[f], 0), cap);           // stored detections of the file
    const int64_t nT = min64(max64(frames[f], 0), ld);           // never past a row, whatever frames[] says
    const T *fspec = spec + f * (int64_t)K * ld;
    const msd_det *fdets = dets + f * cap;
    const int64_t inf_t = 0x7fffffffffffffffLL;
    for (int64_t i = (int64_t)blockIdx.y * WAVES + wave; i < m; i += (int64_t)gridDim.y * WAVES) {
        const Span s = span_of(fdets, i, m, c, nT);
        msd_echo e = empty_record(s);
        if (s.t1 > s.t0) {
            // pass 1: the lane's frames t0 + lane, t0 + lane + 64, ...
            double bS = 0.0, bN = 0.0, bD = 0.0;
            int64_t bt = inf_t;
            int32_t bk = -1;
            double eS = 0.0, eN = 0.0, wr = 0.0, wu = 0.0, wuu = 0.0, wur = 0.0;
            for (int64_t t = s.t0 + lane; t < s.t1; t += 64) {
                const Column col = column_of(fspec + t, ld, K, c);
                if (bt == inf_t || col.S > bS) bS = col.S, bN = col.N, bD = col.delta, bk = col.k, bt = t;
                const double u = (double)(t - s.t0), r = (double)(col.k - c.k_lo) + col.delta, su = col.S * u;
                eS = eS + col.S;
                eN = eN + col.N;
                wr = wr + col.S * r;
                wu = wu + su;
                wuu = wuu + su * u;
                wur = wur + su * r;
            }
            // the peak over the wave: value descending, frame ascending; lanes without a frame lose
            double pS = bS;
            int64_t pt = bt;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double oS = __shfl_xor(pS, o, 64);
                const int64_t ot = (int64_t)__shfl_xor((long long)pt, o, 64);
                const bool take = ot != inf_t && (pt == inf_t || oS > pS || (oS == pS && ot < pt));
                if (take) pS = oS, pt = ot;
            }
            const int owner = (int)((pt - s.t0) & 63);  // the lane that computed frame t_peak
            e.p_peak = pS, e.t_peak = pt;
            e.k_peak = __shfl(bk, owner, 64);
            e.d_peak = __shfl(bD, owner, 64);
            e.n_peak = __shfl(bN, owner, 64);
            e.e_sig = wave_sum_d(eS), e.e_noise = wave_sum_d(eN);
            e.w_r = wave_sum_d(wr), e.w_u = wave_sum_d(wu), e.w_uu = wave_sum_d(wuu), e.w_ur = wave_sum_d(wur);
            // pass 2: the frames at half power and the e-fold frame
            const double half = 0.5 * pS, fold = pS * INV_E;
            int64_t first = inf_t, last = -1, ef = inf_t;
            for (int64_t t = s.t0 + lane; t < s.t1; t += 64) {
                const double S = band_sum(fspec + t, ld, c.k_lo, c.k_hi);
                if (S >= half) {
                    if (first == inf_t) first = t;
                    last = t;
                }
                if (t > pt && S <= fold && ef == inf_t) ef = t;
            }
            first = wave_min_i64(first), last = wave_max_i64(last), ef = wave_min_i64(ef);
            e.t_half_first = first == inf_t ? pt : first;
            e.t_half_last = last < 0 ? pt : last;
            e.t_efold = ef == inf_t ? s.t1 : ef;
            e.flags = s.flags | (e.t_efold == s.t1 ? 4 : 0) | (pt == s.t0 || pt == s.t1 - 1 ? 8 : 0);
        }
        if (lane == 0) out[f * cap + i] = e;
    }
}

template <typename T>
int launch_echo(msd_ctx *ctx, const T *spec, int64_t nfiles, int32_t K, const int64_t *frames, int64_t ld,
                const msd_det *dets, int64_t cap, const int64_t *counts, const msd_echo_cfg *cfg, msd_echo *out) {
    const int64_t gy = min64((cap + WAVES - 1) / WAVES, MAX_GRID_Y);
    KernelTimer timer(ctx, K_ECHO);
    hipLaunchKernelGGL(echo_kernel<T>, dim3((unsigned)nfiles, (unsigned)gy), dim3(THREADS), 0, ctx->stream, spec, K,
                       frames, ld, dets, cap, counts, *cfg, out);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

template <typename T>
int measure_dev(const char *who, msd_ctx *ctx, const T *spec, int64_t nfiles, int32_t K, const int64_t *frames,
                int64_t ld, const msd_det *dets, int64_t cap, const int64_t *counts, const msd_echo_cfg *cfg,
                msd_echo *out) {
    const char *msg = "";
    if (int rc = validate(cfg, K, &msg)) return fail(rc, std::string(who) + ": " + msg);
    if (!ctx || nfiles < 0 || cap < 0 || ld < 0)
        return fail(MSD_ERR_INVALID, std::string(who) + ": null context or negative size");
    if (nfiles > 0 && cap > 0 && (!spec || !frames || !dets || !counts || !out))
        return fail(MSD_ERR_INVALID, std::string(who) + ": null argument");
    if (nfiles == 0 || cap == 0) return MSD_OK;
    if (nfiles > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, std::string(who) + ": too many files");
    DeviceGuard g(ctx->device);
    return launch_echo(ctx, spec, nfiles, K, frames, ld, dets, cap, counts, cfg, out);
}

// one file from host buffers: the spectrogram into the samples slot, {frames, n} and the detections into the
// detections slot, the records through the output slot
template <typename T>
int measure_host(const char *who, msd_ctx *ctx, const T *spec, int32_t K, int64_t frames, int64_t ld,
                 const msd_det *dets, int64_t n, const msd_echo_cfg *cfg, msd_echo *out) {
    const char *msg = "";
    if (int rc = validate(cfg, K, &msg)) return fail(rc, std::string(who) + ": " + msg);
    if (!ctx || n < 0 || frames < 0) return fail(MSD_ERR_INVALID, std::string(who) + ": null context or negative size");
    if (ld < frames) return fail(MSD_ERR_INVALID, std::string(who) + ": ld smaller than frames");
    if (n > 0 && (!dets || !out || (!spec && frames > 0))) return fail(MSD_ERR_INVALID, std::string(who) + ": null argument");
    if (n == 0) return MSD_OK;
    DeviceGuard g(ctx->device);
    const size_t spec_bytes = (size_t)K * (size_t)ld * sizeof(T), det_bytes = (size_t)n * sizeof(msd_det);
    void *dspec = nullptr, *dmeta = nullptr, *dout = nullptr;
    if (int rc = ctx_scratch(ctx, SCRATCH_SAMPLES, spec_bytes, &dspec)) return rc;
    if (int rc = ctx_scratch(ctx, SCRATCH_DETECTIONS, 16 + det_bytes, &dmeta)) return rc;
    if (int rc = ctx_scratch(ctx, SCRATCH_OUTPUT, (size_t)n * sizeof(msd_echo), &dout)) return rc;
    std::vector<char> meta(16 + det_bytes);
    const int64_t head[2] = {frames, n};
    std::memcpy(meta.data(), head, 16);
    std::memcpy(meta.data() + 16, dets, det_bytes);
    // `meta` is the source of an asynchronous copy: whatever happens, the stream is drained before it goes
    auto enqueue = [&]() -> int {
        if (spec_bytes && frames > 0) MSD_HIP(hipMemcpyAsync(dspec, spec, spec_bytes, hipMemcpyHostToDevice, ctx->stream));
        MSD_HIP(hipMemcpyAsync(dmeta, meta.data(), meta.size(), hipMemcpyHostToDevice, ctx->stream));
        const int64_t *dhead = static_cast<const int64_t *>(dmeta);
        if (int rc = launch_echo(ctx, static_cast<const T *>(dspec), 1, K, dhead, ld,
                                 reinterpret_cast<const msd_det *>(dhead + 2), n, dhead + 1, cfg,
                                 static_cast<msd_echo *>(dout)))
            return rc;
        MSD_HIP(hipMemcpyAsync(out, dout, (size_t)n * sizeof(msd_echo), hipMemcpyDeviceToHost, ctx->stream));
        return MSD_OK;
    };
    const int rc = enqueue();
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    return e == hipSuccess ? MSD_OK : hip_fail(e, "hipStreamSynchronize");
}

}  // namespace
}  // namespace msd

using namespace msd;

extern "C" {

int msd_echo_measure_dev(msd_ctx *ctx, const float *spec, int64_t nfiles, int32_t K, const int64_t *frames, int64_t ld,
                         const msd_det *dets, int64_t cap, const int64_t *counts, const msd_echo_cfg *cfg,
                         msd_echo *out) {
    return measure_dev("msd_echo_measure_dev", ctx, spec, nfiles, K, frames, ld, dets, cap, counts, cfg, out);
}

int msd_echo_measure_f64_dev(msd_ctx *ctx, const double *spec, int64_t nfiles, int32_t K, const int64_t *frames,
                             int64_t ld, const msd_det *dets, int64_t cap, const int64_t *counts,
                             const msd_echo_cfg *cfg, msd_echo *out) {
    return measure_dev("msd_echo_measure_f64_dev", ctx, spec, nfiles, K, frames, ld, dets, cap, counts, cfg, out);
}

int msd_echo_measure(msd_ctx *ctx, const float *spec, int32_t K, int64_t frames, int64_t ld, const msd_det *dets,
                     int64_t n, const msd_echo_cfg *cfg, msd_echo *out) {
    return measure_host("msd_echo_measure", ctx, spec, K, frames, ld, dets, n, cfg, out);
}

int msd_echo_measure_f64(msd_ctx *ctx, const double *spec, int32_t K, int64_t frames, int64_t ld, const msd_det *dets,
                         int64_t n, const msd_echo_cfg *cfg, msd_echo *out) {
    return measure_host("msd_echo_measure_f64", ctx, spec, K, frames, ld, dets, n, cfg, out);
}

}  // extern "C"
