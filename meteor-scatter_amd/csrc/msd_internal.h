// Internal declarations shared by the libmsdsp translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/msdsp.h"
#include "dev_mem.h"
#include "welch_fft_plan.h"

namespace msd {

void set_error(const std::string &msg);
int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);
// hipFuncAttributeMaxDynamicSharedMemorySize = bytes for `kernel` on the CURRENT device, once
// per (kernel, device); thread-safe (several contexts may launch from several threads)
int ensure_dyn_lds(const void *kernel, int bytes);

#define MSD_HIP(call)                                   \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

enum KernelId { K_STFT = 0, K_BLOCK = 1, K_DSTAT = 2, K_DSCAN = 3, K_WELCH = 4, K_LIVE = 5, K_CSTFT = 6, K_IQDELTA = 7, K_FRESH = 8, K_SSCAN = 9,
               K_REFINE = 10, K_CSTFT_DC = 11, K_WSPEC = 12, K_DDC = 13, K_RESAMP = 14, K_CLUSTER = 15, K_ECHO = 16, K_COUNT = 17 };

struct EventPair {
    hipEvent_t a, b;
    int kernel;
};

// the context's scratch buffers, one per use (a call may hold several at once)
enum ScratchSlot {
    SCRATCH_SAMPLES = 0,    // the one file's samples (stage_one_file)
    SCRATCH_META,           // its {offset, length}
    SCRATCH_OUTPUT,         // the launcher's output before the read-back
    SCRATCH_DETECTIONS,     // detector inputs, counters and detections / meteors
    SCRATCH_WELCH_PSD,      // launch_welch_i8's PSD when the caller passes none
    SCRATCH_LIVE_SEGMENTS,  // the live detector's per-segment scan states
    SCRATCH_COUNT
};

// msd_iq_delta64_dev's caches, kept on the context
struct RefineCache {
    DevBuf<double2> w;  // twiddle table W^m (m < w_n), built once per frame length
    int w_n = 0;
    // the per-call tables staged in pinned memory (no stream sync), reusable once ev has passed
    PinBuf pin;
    hipEvent_t ev = nullptr;
    // the tables of the last call as uploaded to `tables` (last_dev): a call with the same tables
    // (every step of a stream of the same length) skips the two copies
    std::vector<char> last;
    const void *last_dev = nullptr;
    DevBuf<char> tables;  // block table, rotations and ranges; last_dev is dropped where it grows
    ~RefineCache() {
        if (ev) (void)hipEventSynchronize(ev), (void)hipEventDestroy(ev);
    }
};

// the int8-MFMA block step's tables: B fragments, column starts, lane twiddles, built once per
// (frame length, bins)
struct RefineI8Cache {
    DevBuf<char> i8_tab;
    uint64_t i8_key = 0;
    // the exact (N, bins) they were built for: the hash only picks the candidate, a match needs
    // these equal (a hash collision must not reuse another geometry's tables)
    int i8_n = 0, i8_nk = 0;
    int i8_km[16] = {};
};

// a guided chunk schedule on the device (guided_sched.h) for `total` items over `wgs` workgroups,
// and the ticket the workgroups draw chunks by
struct GuidedSched {
    DevBuf<int64_t> bounds;
    DevBuf<unsigned long long> ticket;
    int64_t total = -1, wgs = -1, n = 0;  // n chunks: bounds[0 .. n]
};
// rebuilds and uploads the schedule when (total, wgs) differ from the last call's (the stream is
// drained first), and always enqueues the ticket's reset on the stream
int guided_sched_prepare(GuidedSched &s, hipStream_t stream, int64_t total, int64_t wgs, int64_t div, int64_t cmin,
                         int64_t multiple, bool merge_short_tail);

}  // namespace msd

struct msd_ctx {
    int device = 0;
    int num_cu = 256;  // compute units (persistent-grid sizing)
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host → HBM uploads (msd_memcpy_h2d_async), created on first use
    hipEvent_t fence_ev = nullptr;      // cross-stream ordering (msd_fence)
    hipEvent_t join_ev = nullptr;       // cross-context ordering (msd_stream_wait), this ctx signalling
    bool timing = false;
    uint32_t timing_mask = 0xffffffffu;  // msd_timing_select: kernel ids timed while timing is on
    bool force_generic = false;  // MSD_OPT_GENERIC_STFT
    bool force_generic_cstft = false;  // MSD_OPT_GENERIC_CSTFT
    bool fresh_all = false;      // MSD_OPT_FRESH_ALL
    std::vector<msd::EventPair> pending;  // recorded, not yet folded into totals
    std::vector<hipEvent_t> pool;         // reusable events
    double total_ms[msd::K_COUNT] = {};
    int64_t launches[msd::K_COUNT] = {};
    // scratch device buffers of the host-pointer convenience entry points (ctx_scratch)
    msd::DevBuf<char> scratch[msd::SCRATCH_COUNT];
    int64_t file_meta[2] = {0, 0};  // stage_one_file's {offset, length}: the source of its async copy
    msd::RefineCache refine;       // msd_iq_delta64_dev (refine.hip)
    msd::RefineI8Cache refine_i8;  // its int8-MFMA block step (refine_i8.hip)
    bool refine_goertzel = false;  // MSD_OPT_REFINE_GOERTZEL: int16 refinement on the float64 Goertzel
    bool block_goertzel = false;   // MSD_OPT_BLOCK_GOERTZEL: int16 block energies on the float64 Goertzel
    bool welch_goertzel = false;   // MSD_OPT_WELCH_GOERTZEL: int16 Welch band powers on the float64 Goertzel
    int cstft_reserve = 0;         // MSD_OPT_CSTFT_RESERVE: workgroup slots the C5 spectrogram leaves free
    int cstft_sched = 0;           // MSD_OPT_CSTFT_SCHED: 0 / 2 chunks from a guided schedule, 1 fixed ranges
    int stft_sched = 0;            // MSD_OPT_STFT_SCHED: the same for stft1024_kernel (tiles)
    int num_cu_dev = 0;            // the device's CUs (num_cu: those the stream may use, MSD_OPT_STREAM_CUS)
    int stream_cus = 0;            // MSD_OPT_STREAM_CUS value in force
    int welch_i8_form = 0;         // MSD_OPT_WELCH_I8_FORM (test hook): bit 0 no int32 pairs, bit 1 generic instantiation
    int stream_eps_log2 = 0;       // MSD_OPT_STREAM_EPS_LOG2 (test hook): the stream's near-tie bound times 2^n
};

struct msd_stft_plan {
    msd_ctx *ctx = nullptr;
    int nperseg = 0, nfft = 0, hop = 0, M = 0;  // M = nfft/2 complex points, K = M + 1 bins
    int detrend = 1;                             // 1 constant (scipy), 0 none (matplotlib mlab)
    int precision = MSD_F32;                     // arithmetic and output type: MSD_F32 or MSD_F64
    double scale = 0;
    msd::DevBuf<float> d_window;   // [nperseg]  (MSD_F32 plans)
    msd::DevBuf<float2> d_tw;      // [M]    exp(-2*pi*i*m/M)
    msd::DevBuf<float2> d_post;    // [M+1]  exp(-2*pi*i*k/(2M))
    msd::DevBuf<double> d_window64;  // the same three in float64 (MSD_F64 plans)
    msd::DevBuf<double2> d_tw64;
    msd::DevBuf<double2> d_post64;
    msd::GuidedSched sched;  // stft1024_kernel's guided tile schedule (chunked, MSD_OPT_STFT_SCHED)
    // stft1024_kernel, integer samples: the frame mean m = tot / 1024 = a + b / 1024 (a = floor) comes
    // off as the exact integer a before the FFT and as b / 1024 times the window's DFT after it, which
    // is exact when that DFT vanishes past bin 1 (periodic Hann: W_0 = N/2, W_1 = -N/4).  win_dft01:
    // W_0, W_1 of the float32 window in float64; win_dft_compact: max |W_k|, 2 <= k <= M, below
    // 1e-6 |W_0| (else integer input takes the generic kernel's exact two-part mean)
    double2 win_dft01[2] = {};
    int win_dft_compact = 0;
};

struct msd_cstft_plan {
    msd_ctx *ctx = nullptr;
    int nperseg = 0, nfft = 0, hop = 0, detrend = 1;
    msd::DevBuf<float> d_win;   // [nperseg] window x sqrt(scale)
    msd::DevBuf<float2> d_tw;   // [nfft] W_nfft^m
    msd::GuidedSched sched;     // cstft4096_kernel, DYN: the guided schedule of frame chunks
};

struct msd_block_plan {
    msd_ctx *ctx = nullptr;
    int64_t block_size = 0;
    int nfft = 0, L = 0;                  // L = min(B, nfft) samples used per block
    int band_lo = 0, band_hi = -1, noise_lo = 0, noise_hi = -1;
    int nbins = 0;                        // band bins + noise bins
    msd::DevBuf<double> d_window;         // [L]
    msd::DevBuf<double2> d_tw;            // [nfft] exp(-2*pi*i*m/nfft)
    msd::DevBuf<int> d_bins;              // [nbins] bin indices, band first
    // fast path (nbins <= 64): per bin {2cos th, cos th, -sin th}, then per (bin, 16-lane
    // segment) the rotation exp(-i th (seg*SPL + SPL - 1)) — host-computed in float64
    // long blocks (L > 4096, block_long_kernel): the per-bin constants alone; a lane's rotation comes
    // from d_tw
    msd::DevBuf<double> d_bconst;
    int spl = 0;                          // samples per lane segment of the fast path / the long kernel
    msd::DevBuf<double2> d_energy;        // fast path: per block (band, noise) energy + 1e-12, grown
    msd::DevBuf<char> d_i8;               // int16 blocks on the matrix cores (block_i8.hip): B fragments
                                          // + column constants, when block_i8_shape(L, nbins)
};

struct msd_welch_plan {
    msd_ctx *ctx = nullptr;
    msd_welch_cfg cfg{};
    int nseg = 0, step = 0;       // segments per block, nperseg - noverlap
    int nslots = 0;               // bins computed per block (band ranges concatenated)
    msd::DevBuf<double> d_window;   // [nperseg]
    msd::DevBuf<double> d_bins;     // [nslots][4]: cos w, sin w, 2 cos w, doubling factor (1 or 2)
    // int16 samples on the matrix cores (welch_i8.hip): B fragments and doubling factors of the
    // nct column tiles; empty when the plan's shape does not take that path
    msd::DevBuf<char> d_i8;
    int i8_nct = 0;
    bool i8_pairs = false;  // the accumulators' digit sums fit int32 pairs (welch_i8_build)
    // the whole-band row (welch_fft.hip), built by the first call that needs it (welch_spectrum_prepare)
    msd::wfft::Plan fft{};
    int fft_state = 0;             // 0 not built, 1 built, -1 a shape the transform does not take
    msd::DevBuf<double2> d_roots;  // [nfft] W_nfft^j
};

namespace msd {

// workgroup barrier that orders LDS only: waits for this wave's LDS accesses, not for its
// global loads (prefetches) or stores still in flight.  __syncthreads() on gfx9 also waits
// vmcnt(0), which drains every outstanding prefetch and store at each barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// a wave-uniform 64-bit value the compiler can keep in SGPRs (a load through x + uniform_i64(off) +
// lane offset then uses the scalar-base + 32-bit lane offset form, no per-lane 64-bit arithmetic)
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// wave-level barrier that also orders the wave's LDS accesses across it (one wave's lanes exchanging
// values through LDS)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a float64 from the lane DPP control CTRL selects (two 32-bit DPP moves)
template <int CTRL>
__device__ __forceinline__ double dpp64(double x) {
    const long long v = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_mov_dpp((int)(v & 0xffffffffll), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(v >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// DPP: v + v[lane ^ 1], v[lane ^ 2], mirrored half rows, mirrored rows → each lane
// holds the sum of its row of 16
__device__ __forceinline__ int row_sum_i(int v) {
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true);  // row_half_mirror
    v += __builtin_amdgcn_mov_dpp(v, 0x140, 0xf, 0xf, true);  // row_mirror
    return v;
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum_f(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return v;
}
// sum over the wave (uniform, in SGPRs): row sums by DPP, then the four rows by readlane
__device__ __forceinline__ int wave_sum_i(int v) {
    v = row_sum_i(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ float lane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float wave_sum_f(float v) {
    v = row_sum_f(v);
    return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}

// int16 pairs packed in a 32-bit word (PCM16 samples, int16 I/Q): SDWA conversion of either half
// straight to float (no separate shift / bit-field extract), and integer sums by v_dot2 (one
// instruction adds both halves, or one of them, to an accumulator)
#ifndef MSD_NO_SDWA
__device__ __forceinline__ float cvt_i16_lo(uint32_t r) {
    float f;
    asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(f) : "v"(r));
    return f;
}
__device__ __forceinline__ float cvt_i16_hi(uint32_t r) {
    float f;
    asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(f) : "v"(r));
    return f;
}
typedef short msd_short2 __attribute__((ext_vector_type(2)));
template <int WLO, int WHI>
__device__ __forceinline__ int dot2_i16(uint32_t r, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(msd_short2, r), msd_short2{WLO, WHI}, acc, false);
}
#else
__device__ __forceinline__ float cvt_i16_lo(uint32_t r) { return (float)(int16_t)(r & 0xffffu); }
__device__ __forceinline__ float cvt_i16_hi(uint32_t r) { return (float)(int16_t)(r >> 16); }
template <int WLO, int WHI>
__device__ __forceinline__ int dot2_i16(uint32_t r, int acc) {
    return acc + WLO * (int)(int16_t)(r & 0xffffu) + WHI * (int)(int16_t)(r >> 16);
}
#endif

// makes `dev` current for the scope
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// the destroy entry point of a plan or session: its work on the context's stream ends, then its
// members free their memory
template <typename P>
void destroy_plan(P *p) {
    if (!p) return;
    DeviceGuard g(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
}

// scoped timing of one kernel launch on ctx->stream
struct KernelTimer {
    msd_ctx *ctx;
    int kernel;
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimer(msd_ctx *c, int k);
    ~KernelTimer();
};

// a float constant held in a VGPR for the rest of the kernel: on gfx950 a VALU operand read from
// an SGPR issues at ~4.4 cycles per wave-instruction and a 32-bit literal at 2.65, a VGPR operand
// at 2.3 (VOP2) / 2.65 (VOP3) (tools/ubench/operand_rate.hip); the compiler hoists uniform constants
// into SGPRs or literals, the opaque move keeps this one in a VGPR
__device__ __forceinline__ float vgpr_f(float c) {
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(c));
    return r;
}

// the context's scratch buffer `slot` grown to at least `bytes`
int ctx_scratch(msd_ctx *ctx, ScratchSlot slot, size_t bytes, void **out);
// one file of a host-pointer entry point on the device: the n samples (`bytes` of them) into the
// samples slot and {0, n} into the meta slot, both copies enqueued on the context's stream;
// *doff, *doff + 1 are the launchers' off and len
int stage_one_file(msd_ctx *ctx, const void *x, size_t bytes, int64_t n, const void **dx, const int64_t **doff);

// launchers (defined in the kernel translation units)
// out: float32 or float64 [nfiles][K][ld] by the plan's precision
int launch_stft(msd_stft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len, int64_t nfiles,
                int64_t max_frames, void *out, int64_t ld);
int launch_stft_any(msd_stft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                    int64_t nfiles, void *out, int64_t ld);
int launch_stft1024(msd_stft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                    int64_t nfiles, float *out, int64_t ld);
// every I/Q spectrogram shape but nperseg = nfft = 4096 (cstft_any.hip); frame_sums are not used
int launch_cstft_any(msd_cstft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                     int64_t nstreams, int64_t max_frames, float *out, float *etot);
// block plans: L = min(block_size, n_fft) up to BLOCK_MAX_L; above BLOCK_FAST_MAX_L one 256-thread
// workgroup per block (block_long_kernel), each lane a segment of block_long_spl(L) samples: L / 256
// rounded up to a multiple of 8, so that a lane's segment starts on a 16-B boundary of an aligned
// int16 block and is read in whole 8-sample chunks
constexpr int BLOCK_FAST_MAX_L = 4096;
constexpr int BLOCK_MAX_L = 65536;
constexpr int block_long_spl(int L) { return ((L + 255) / 256 + 7) / 8 * 8; }
bool block_i8_shape(int64_t L, int nbins);
bool block_i8_window(const double *window, int64_t L);
bool welch_i8_shape(const msd_welch_cfg &c, int nseg, int nslots, const double *window);
int welch_i8_build(msd_welch_plan *p, const double *window);
int launch_welch_i8(msd_welch_plan *p, const int16_t *x, const int64_t *off, const int64_t *len, int64_t nfiles,
                    int64_t max_blocks, double *band_db, int64_t ld, double *psd);
// the whole-band Welch row of every block (welch_fft.hip): psd[(f*ld + b)*K + k], db_mean[f*ld + b] (may be
// null); prepare builds the plan's transform tables (a blocking upload, once)
int welch_spectrum_prepare(msd_welch_plan *p);
int launch_welch_spectrum(msd_welch_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len,
                          int64_t nfiles, int64_t max_blocks, double *psd, int64_t ld, double *db_mean);
int block_i8_build(msd_block_plan *p, const double *window, const int *bins, int nbins);
int launch_block_i8(msd_block_plan *p, const int16_t *x, const int64_t *off, const int64_t *len, int64_t nfiles,
                    int64_t max_blocks);
int launch_block_delta(msd_block_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                       int64_t nfiles, int64_t max_blocks, double *band_db, double *noise_db, double *delta,
                       int64_t ld);
int launch_detect(msd_ctx *ctx, const double *delta, const int64_t *nblocks, int64_t nfiles, int64_t ld,
                  const msd_det_cfg *cfg, msd_det *dets, int64_t cap, int64_t *counts, double *thresholds,
                  double *margin, int32_t *status, const msd_hist_cfg *hist);

inline size_t dtype_size(int dtype) {
    switch (dtype) {
        case MSD_U8: return 1;
        case MSD_I16: return 2;
        case MSD_I32: return 4;
        case MSD_F32: return 4;
        case MSD_F64: return 8;
        default: return 0;
    }
}

}  // namespace msd
