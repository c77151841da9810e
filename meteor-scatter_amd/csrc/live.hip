// Phase-2 live detector of the reference (dsp/src/live/backend/processor.py), float64:
//   welch_bands_kernel  a8  per processing block: scipy.signal.welch(block, fs, nfft=n_fft)
//                           (processor.py:206) restricted to the bins of the three bands, and
//                           the band sums → dB (processor.py:349-369)
//   live_seg_*_kernel   a9  the over-noise value, its history threshold and the
//                           Init / Detection / Tracking state machine (processor.py:391-507)
//
// (int16 audio takes welch_i8.hip's exact integer GEMM instead of welch_bands_kernel by default.)
// welch_bands_kernel: one wave per block.  Each Welch segment's samples are staged in the
// wave's LDS as float64 (times the soundfile scale), detrended with the numpy-order mean and
// windowed; then every band bin (one lane each) runs a float64 Goertzel recurrence over the
// nperseg samples — the band bins only, not the whole nfft-point rFFT (the zero padding to
// nfft only sets the bin spacing).  Segment powers are averaged in scipy's order (sequential
// over segments, / nseg) and the band sums use numpy's pairwise order.
//
// live_over_kernel, live_history_kernel: the over-noise values, then the history thresholds
// mean + k*std of the previous W of them -- state-free, one thread per block of every file
// (the whole GPU, not one workgroup per file);
// live_seg_{init,scan,link,emit}_kernel: the state machine in 256-block time segments, one wave
// each over the whole GPU (ballots), rounds of scan + link to a fixed point over their entry states,
// then one emitting pass.
// live_session_*_kernel: the same detector fed in pushes (msdsp.h, live session): the state, the
// over-noise tail and the samples short of a block stay on the device; one wave per stream scans a
// push's blocks in order from the carried state (no rounds, no host synchronisation).
#include <cmath>

#include "msd_internal.h"
#include "np_reduce.h"

#pragma clang fp contract(off)

namespace msd {
namespace {

constexpr int WL_THREADS = 256;

// np.sum over LDS in numpy's exact order: one pairwise leaf inline up to 128 elements (the
// default 100 Hz bands: 103 bins at nfft 4096), numpy's full recursion beyond (bands wider
// than 128 bins, nperseg above 128)
__device__ __forceinline__ double lds_band_sum(const double *p, int64_t base, int64_t n) {
    return n <= 128 ? np_sum_small(ArrRef{p}, base, n) : np_sum(ArrRef{p}, base, n);
}

template <typename T>
__device__ __forceinline__ double to_f64(T v) {
    return (double)v;
}

struct WelchArgs {
    int64_t nfiles, max_blocks, ld;
    int block_size, nperseg, step, nseg, nfft, nslots, nbands;
    int wave_lds;  // doubles of LDS per wave: segment [nperseg, padded] + psd [nslots, padded]
    double sample_scale, scale;
    int band_lo[MSD_WELCH_MAX_BANDS], band_hi[MSD_WELCH_MAX_BANDS];
    int band_slot0[MSD_WELCH_MAX_BANDS];  // first slot of each band
};

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const int2 v = __builtin_bit_cast(int2, x);
    int2 r;
    r.x = __builtin_amdgcn_readlane(v.x, lane);
    r.y = __builtin_amdgcn_readlane(v.y, lane);
    return __builtin_bit_cast(double, r);
}

// np.sum(seg[0:n]) by one wave, numpy's pairwise order.  n = 256 (scipy's default
// nperseg): two 128-element leaves, their 8 interleaved partial sums on lanes 0-7 / 8-15,
// combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) by DPP; other n: lane 0 (lds_band_sum).
__device__ __forceinline__ double wave_np_sum(const double *seg, int n, int lane) {
    if (n == 256) {
        double r = 0.0;
        if (lane < 16) {
            const double *a = seg + (lane >> 3) * 128 + (lane & 7);
            r = a[0];
            for (int k = 1; k < 16; ++k) r += a[8 * k];
        }
        r += dpp64<0xB1>(r);   // lane ^ 1
        r += dpp64<0x4E>(r);   // lane ^ 2
        r += dpp64<0x141>(r);  // half-row mirror: lanes 0-3 meet 4-7 (8-11 meet 12-15)
        return 0.0 + (readlane_f64(r, 0) + readlane_f64(r, 8));
    }
    double v = 0.0;
    if (lane == 0) v = lds_band_sum(seg, 0, n);
    return readlane_f64(v, 0);
}

// Goertzel power of NB band bins per lane (bins j, j + 64, ...) over the staged, windowed
// segment, added into the wave's psd in segment order.  The arithmetic per bin is the same
// for any NB (bit-identical results).
template <int NB>
__device__ __forceinline__ void goertzel_bins(const double *seg, int L, const double *__restrict__ g_bins, int j,
                                              int nslots, double scale, double *psd, int s) {
    double cw[NB], sw[NB], c2[NB], dbl[NB], s1[NB], s2[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int jb = j + 64 * b;
        const double *bc = g_bins + 4 * (jb < nslots ? jb : 0);
        cw[b] = bc[0], sw[b] = bc[1], c2[b] = bc[2], dbl[b] = bc[3];
        s1[b] = 0.0, s2[b] = 0.0;
    }
    const double2 *y2 = reinterpret_cast<const double2 *>(seg);
    int m = 0;
#pragma unroll 4
    for (; m + 2 <= L; m += 2) {
        const double2 y = y2[m >> 1];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            double s0 = __builtin_fma(c2[b], s1[b], y.x - s2[b]);
            s2[b] = s1[b];
            s1[b] = s0;
            s0 = __builtin_fma(c2[b], s1[b], y.y - s2[b]);
            s2[b] = s1[b];
            s1[b] = s0;
        }
    }
    if (m < L) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const double s0 = __builtin_fma(c2[b], s1[b], seg[m] - s2[b]);
            s2[b] = s1[b];
            s1[b] = s0;
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int jb = j + 64 * b;
        // X e^{i w (L-1)} = s1 - e^{-i w} s2: |X|^2 = re^2 + im^2
        const double re = s1[b] - cw[b] * s2[b], im = sw[b] * s2[b];
        double p = re * re + im * im;  // conj(X) * X (real part)
        p = p * scale;                 // result *= scale
        p = p * dbl[b];                // result[..., 1:-1] *= 2 (onesided psd)
        if (jb < nslots) psd[jb] = s == 0 ? p : psd[jb] + p;  // Pxy.mean(axis=-1): segments in order
    }
}

// One wave per processing block: per Welch segment, stage + detrend + window the samples in
// the wave's LDS, then Goertzel over the segment for every band bin (lane = bin, broadcast
// LDS reads of the samples, two per ds_read_b128), accumulating the segment powers in the
// wave's LDS psd in segment order.  No workgroup barriers: the 4 waves of a workgroup work
// on independent blocks.
template <typename T>
__global__ __launch_bounds__(WL_THREADS) void welch_bands_kernel(const T *__restrict__ x,
                                                                 const int64_t *__restrict__ off,
                                                                 const int64_t *__restrict__ len, WelchArgs A,
                                                                 const double *__restrict__ g_win,
                                                                 const double *__restrict__ g_bins,
                                                                 double *__restrict__ band_db,
                                                                 double *__restrict__ psd_out) {
    extern __shared__ double sm[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t gb = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;  // 1-4 waves per workgroup
    const int64_t f = gb / A.max_blocks;
    const int64_t b = gb - f * A.max_blocks;
    if (f >= A.nfiles) return;
    const int64_t n = len[f];
    const int64_t nb = n >= A.block_size ? (n - A.block_size) / A.block_size + 1 : 0;
    if (b >= nb) return;  // whole wave
    double *seg = sm + wave * A.wave_lds;                 // [nperseg (+pad)]
    double *psd = seg + ((A.nperseg + 1) & ~1);           // [nslots]
    const T *xb = x + off[f] + b * (int64_t)A.block_size;
    const int L = A.nperseg;

    for (int s = 0; s < A.nseg; ++s) {
        const T *xs = xb + s * A.step;
        for (int i = lane; i < L; i += 64) seg[i] = to_f64(xs[i]) * A.sample_scale;
        wave_sync();
        // detrend='constant': d - np.mean(d, axis=-1) (numpy pairwise order)
        const double mean = wave_np_sum(seg, L, lane) / (double)L;
        wave_sync();
        for (int i = lane; i < L; i += 64) seg[i] = g_win[i] * (seg[i] - mean);  // win * detrended
        wave_sync();
        // two bins per lane while 128 remain (one broadcast LDS read feeds both recurrences:
        // half the LDS reads per flop, two independent FMA chains), then one per lane
        int j0 = 0;
        for (; j0 + 128 <= A.nslots; j0 += 128) goertzel_bins<2>(seg, L, g_bins, j0 + lane, A.nslots, A.scale, psd, s);
        for (; j0 < A.nslots; j0 += 64) goertzel_bins<1>(seg, L, g_bins, j0 + lane, A.nslots, A.scale, psd, s);
        wave_sync();
    }
    for (int j = lane; j < A.nslots; j += 64) {
        const double v = psd[j] / (double)A.nseg;
        psd[j] = v;
        if (psd_out) psd_out[(f * A.ld + b) * (int64_t)A.nslots + j] = v;
    }
    wave_sync();
    if (lane < A.nbands) {
        const int w = A.band_hi[lane] - A.band_lo[lane] + 1;
        const double P = w > 0 ? lds_band_sum(psd, A.band_slot0[lane], w) : 0.0;  // np.sum(psd[mask])
        band_db[(f * A.nbands + lane) * A.ld + b] = P > 0.0 ? 10.0 * log10(P) : -INFINITY;
    }
}

struct LiveArgs {
    msd_live_cfg cfg;
    int64_t nfiles, ld, cap;
};

// Python's builtin min/max over a list (first element kept unless a later one compares
// strictly less / greater — NaN behaves as CPython's does)
__device__ __forceinline__ void py_minmax(gdouble_t *v, int64_t a, int64_t e, double &mn, double &mx) {
    mn = v[a];
    mx = v[a];
    for (int64_t i = a + 1; i < e; ++i) {
        if (v[i] < mn) mn = v[i];
        if (v[i] > mx) mx = v[i];
    }
}

struct LiveScan {
    int state = 0;  // 0 init, 1 detection, 2 tracking
    double lock = -1.0, until = -1.0, t_start = 0.0;
    int64_t trig = 0, cnt = 0;
};

// numpy mean/std of over[b, b+n), read from global memory as such (global loads: the event handlers
// are out of line, and a generic pointer there would be read with flat instructions, np_reduce.h)
__device__ __forceinline__ void hist_stats(const double *ov, int64_t b, int64_t n, double &mean, double &sd,
                                           double *mn, double *mx) {
    np_mean_std_global(ov, b, n, mean, sd);
    if (mn) py_minmax(as_global(ov), b, b + n, *mn, *mx);
}

// The two event handlers are out of line (they run once per meteor; inlined, their numpy sums
// would be copied into every scan).  The scan state travels by value and the history is read
// through global loads: no generic pointer -- to the caller's scratch, to LDS or to global memory --
// reaches them, so they hold no flat instruction (np_reduce.h, tests/test_build_check.py).

// Detection → Tracking (processor.py:462-472): locked_threshold = thr + 0 * history_std
__device__ __forceinline__ LiveScan live_trigger_body(LiveScan sc, const double *ov, int64_t i, double t, double t0,
                                                      int64_t W) {
    const int64_t h0 = W > 0 ? (i - W > 0 ? i - W : 0) : 0;
    double hm = NAN, hs = NAN;
    if (i - h0 > 0) hist_stats(ov, h0, i - h0, hm, hs, nullptr, nullptr);
    sc.lock = t + 0.0 * hs;
    sc.t_start = t0;
    sc.trig = i;
    sc.state = 2;
    return sc;
}
__device__ __noinline__ LiveScan live_trigger(LiveScan sc, const double *ov, int64_t i, double t, double t0,
                                              int64_t W) {
    return live_trigger_body(sc, ov, i, t, t0, W);
}

// Tracking ends (processor.py:474-504): history = over[trig+1 .. i]
__device__ __forceinline__ LiveScan live_close_body(LiveScan sc, const double *ov, int64_t i, double t0,
                                                    double min_db_mean, double min_dur_sec, double wait_sec,
                                                    msd_meteor *out, int64_t cap, bool writer) {
    const double dur = t0 - sc.t_start;
    double hm, hs, mn, mx;
    hist_stats(ov, sc.trig + 1, i - sc.trig, hm, hs, &mn, &mx);
    if (hm >= min_db_mean && dur >= min_dur_sec) {
        if (writer && sc.cnt < cap) {
            typedef __attribute__((address_space(1))) int64_t gi64;
            typedef __attribute__((address_space(1))) double gf64;
            msd_meteor *m = out + sc.cnt;  // fields stored through global pointers (global_store)
            *(gi64 *)&m->start_block = sc.trig;
            *(gi64 *)&m->stop_block = i;
            *(gf64 *)&m->time_start = sc.t_start;
            *(gf64 *)&m->time_stop = t0;
            *(gf64 *)&m->duration = dur;
            *(gf64 *)&m->db_min = mn;
            *(gf64 *)&m->db_max = mx;
            *(gf64 *)&m->db_mean = hm;
            *(gf64 *)&m->db_std = hs;
        }
        ++sc.cnt;
    }
    sc.state = 1;
    sc.until = t0 + wait_sec;
    return sc;
}
__device__ __noinline__ LiveScan live_close(LiveScan sc, const double *ov, int64_t i, double t0, double min_db_mean,
                                            double min_dur_sec, double wait_sec, msd_meteor *out, int64_t cap,
                                            bool writer) {
    return live_close_body(sc, ov, i, t0, min_db_mean, min_dur_sec, wait_sec, out, cap, writer);
}

// processor.py:391: block_db_2_ms = block_db_ms - np.mean([n1, n2])
__global__ __launch_bounds__(WL_THREADS) void live_over_kernel(const double *__restrict__ band_db,
                                                                const int64_t *__restrict__ nblocks, LiveArgs A,
                                                                double *__restrict__ over) {
    const int64_t f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * WL_THREADS + threadIdx.x;
    if (i >= A.ld || i >= nblocks[f]) return;
    const double *sig = band_db + (f * 3 + 0) * A.ld;
    const double *n1 = band_db + (f * 3 + 1) * A.ld;
    const double *n2 = band_db + (f * 3 + 2) * A.ld;
    const double m = (0.0 + (-0.0 + n1[i] + n2[i])) / 2.0;  // np.add.reduce starts at +0.0 (np_reduce.h)
    over[f * A.ld + i] = sig[i] - m;
}

// processor.py:392-402: history = the previous min(W, b) values (W = 0 → all of them)
__global__ __launch_bounds__(WL_THREADS) void live_history_kernel(const int64_t *__restrict__ nblocks, LiveArgs A,
                                                                   const double *__restrict__ over,
                                                                   double *__restrict__ thr) {
    const int64_t f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * WL_THREADS + threadIdx.x;
    if (i >= A.ld || i >= nblocks[f]) return;
    const int64_t W = A.cfg.avg_win_blocks;
    const int64_t h0 = W > 0 ? (i - W > 0 ? i - W : 0) : 0;
    const int64_t hn = i - h0;
    double mean = NAN, sd = NAN;
    if (hn > 0) np_mean_std(over + f * A.ld, h0, hn, mean, sd);
    thr[f * A.ld + i] = mean + A.cfg.k_std * sd;
}

// the state machine of one file, time-segmented: segment s scans blocks [s L, (s + 1) L) of its file
// (L = LV_SEGLEN; one wave per segment, every file's segments over the whole GPU).  Segment 0 starts
// from the true initial state (Init); the others from the memoryless Detection state (no lock),
// which is where a file spends most of its time.  After each round every segment whose entry
// differs from its predecessor's exit re-scans from that exit, until no entry changes (normally 2-3
// rounds); the final entries are then exact, and a last pass per segment writes the thresholds used
// and the meteors at offsets from the earlier segments' meteor counts.  A segment's scan: at position
// k lane j evaluates block k + j under the current state; the first block whose event condition holds
// (ballot) is where the state changes, so a 64-block span without events is one step.
// (Rounds 1-5 ran one 16-wave workgroup per file with the rounds inside it: 24 files used 24 CUs,
// 0.65-0.70 ms per day.)
// blocks per segment: 256 against 64 / 128 / 512 / 1024 measured 0.26-0.31 vs 0.55 / 0.34-0.35 /
// 0.31-0.32 / 0.42-0.47 ms per day for the state machine (profiles/r6_live_seglen_ab.txt)
constexpr int LV_SEGLEN = 256;
constexpr int LV_ROUNDS = 4;  // rounds launched before the convergence flag is read

__device__ __forceinline__ bool live_same_entry(const LiveScan &x, const LiveScan &y, double t1_first) {
    if (x.state != y.state) return false;
    if (x.state == 2)
        return __builtin_bit_cast(long long, x.lock) == __builtin_bit_cast(long long, y.lock) &&
               __builtin_bit_cast(long long, x.t_start) == __builtin_bit_cast(long long, y.t_start) && x.trig == y.trig;
    if (x.state == 1) {  // a lock that has run out before the first block's end is no lock
        const bool lx = x.until > t1_first, ly = y.until > t1_first;
        if (lx != ly) return false;
        return !lx || (__builtin_bit_cast(long long, x.lock) == __builtin_bit_cast(long long, y.lock) &&
                       __builtin_bit_cast(long long, x.until) == __builtin_bit_cast(long long, y.until));
    }
    return true;
}

struct LiveSegArgs {
    LiveArgs L;
    int64_t smax;  // segments per file slot: ceil(ld / LV_SEGLEN)
};

__device__ __forceinline__ double live_tblk(const msd_live_cfg &C, int64_t i) {
    return (double)(i * (int64_t)C.block_size) / C.fs;
}

// one wave's pass over blocks [a, b) of one file from sc; emit: write the thresholds used and the meteors.
// INL: the event handlers inlined (the live session's kernel, which may not call: tests/test_build_check.py)
template <bool INL>
__device__ __forceinline__ void live_scan(LiveScan &sc, int64_t a, int64_t b, bool emit, const double *ov, double *th,
                                          const msd_live_cfg &C, msd_meteor *outf, int64_t cap, int lane) {
    int64_t k = a;
    while (k < b) {
        const int64_t kk = k + lane;
        const bool valid = kk < b;
        const int64_t kc = valid ? kk : b - 1;
        const double v = ov[kc], fresh = th[kc], t0 = live_tblk(C, kc), t1 = live_tblk(C, kc + 1);
        double t;
        bool cand;
        if (sc.state == 0) {
            t = fresh;
            cand = t0 >= C.init_wait_sec;
        } else if (sc.state == 1) {
            t = sc.until > t1 ? sc.lock : fresh;
            cand = v > t;
        } else {
            t = sc.lock;
            cand = v < t;
        }
        const uint64_t mask = __ballot(valid && cand);
        const int first = mask ? __builtin_ctzll(mask) : 64;
        if (emit && valid && lane <= first) th[kk] = t;  // thresholds used (processor.py:395-412)
        if (!mask) {
            k += 64;
            continue;
        }
        const int64_t e = k + first;  // event block
        const double te = __shfl(t, first), t0e = __shfl(t0, first);
        if (sc.state == 0) {
            sc.state = 1;
            sc.lock = -1.0;
            sc.until = -1.0;
        } else if (sc.state == 1) {
            sc = INL ? live_trigger_body(sc, ov, e, te, t0e, C.avg_win_blocks)
                     : live_trigger(sc, ov, e, te, t0e, C.avg_win_blocks);
        } else {
            sc = INL ? live_close_body(sc, ov, e, t0e, C.min_db_mean, C.min_dur_sec, C.after_tracking_wait_sec, outf,
                                       cap, emit && lane == 0)
                     : live_close(sc, ov, e, t0e, C.min_db_mean, C.min_dur_sec, C.after_tracking_wait_sec, outf, cap,
                                  emit && lane == 0);
        }
        k = e + 1;
    }
}

// the segments' states: in / out [nfiles][smax] (entry, exit), cnt (meteors), active
struct LiveSegState {
    LiveScan *in, *out;
    int64_t *cnt;
    int32_t *active;
    int32_t *changed;  // [1]: some entry changed in the last link
};

// entries of round 1: Init at each file's start, Detection elsewhere; counts / status of empty files
__global__ __launch_bounds__(256) void live_seg_init_kernel(const int64_t *__restrict__ nblocks, LiveSegArgs A,
                                                            LiveSegState S, int64_t *__restrict__ counts,
                                                            int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.L.nfiles * A.smax) return;
    const int64_t f = i / A.smax, s = i - f * A.smax;
    const int64_t nb = nblocks[f];
    LiveScan e0;
    if (s > 0) {
        e0.state = 1;
        e0.lock = -1.0;
        e0.until = -1.0;
    }
    S.in[i] = e0;
    S.active[i] = s * LV_SEGLEN < nb;
    if (s == 0 && nb <= 0) {  // no segment: no meteors
        counts[f] = 0;
        if (status) status[f] = 0;
    }
}

// one wave per active segment: scan from its entry, record its exit and meteor count
__global__ __launch_bounds__(256) void live_seg_scan_kernel(const int64_t *__restrict__ nblocks, LiveSegArgs A,
                                                            LiveSegState S, const double *__restrict__ over,
                                                            double *__restrict__ thr) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.L.nfiles * A.smax || !S.active[i]) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t f = i / A.smax, s = i - f * A.smax;
    const int64_t nb = nblocks[f];
    const int64_t a = s * LV_SEGLEN, b = a + LV_SEGLEN < nb ? a + LV_SEGLEN : nb;
    LiveScan sc = S.in[i];
    sc.cnt = 0;
    live_scan<false>(sc, a, b, false, over + f * A.L.ld, thr + f * A.L.ld, A.L.cfg, nullptr, 0, lane);
    if (lane == 0) {
        S.out[i] = sc;
        S.cnt[i] = sc.cnt;
    }
}

// a segment whose entry differs from its predecessor's exit re-scans from that exit next round
__global__ __launch_bounds__(256) void live_seg_link_kernel(const int64_t *__restrict__ nblocks, LiveSegArgs A,
                                                            LiveSegState S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.L.nfiles * A.smax) return;
    const int64_t f = i / A.smax, s = i - f * A.smax;
    const int64_t a = s * LV_SEGLEN;
    int act = 0;
    if (s > 0 && a < nblocks[f]) {  // (an empty segment's exit is its entry: its scan does nothing)
        const LiveScan nw = S.out[i - 1];
        if (!live_same_entry(nw, S.in[i], live_tblk(A.L.cfg, a + 1))) {
            S.in[i] = nw;
            act = 1;
            *S.changed = 1;
        }
    }
    S.active[i] = act;
}

// final pass from the exact entries: the thresholds used and the meteors at the offsets of the
// earlier segments' counts; the file's last segment writes its count and status
__global__ __launch_bounds__(256) void live_seg_emit_kernel(const int64_t *__restrict__ nblocks, LiveSegArgs A,
                                                            LiveSegState S, const double *__restrict__ over,
                                                            double *__restrict__ thr, msd_meteor *__restrict__ out,
                                                            int64_t *__restrict__ counts,
                                                            int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.L.nfiles * A.smax) return;
    const int lane = threadIdx.x & 63;
    const int64_t f = i / A.smax, s = i - f * A.smax;
    const int64_t nb = nblocks[f];
    const int64_t a = s * LV_SEGLEN;
    if (a >= nb) return;  // wave-uniform
    const int64_t b = a + LV_SEGLEN < nb ? a + LV_SEGLEN : nb;
    int64_t off = 0;  // meteors of the file's earlier segments
    for (int64_t j = lane; j < s; j += 64) off += S.cnt[i - s + j];
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    LiveScan sc = S.in[i];
    sc.cnt = off;
    live_scan<false>(sc, a, b, true, over + f * A.L.ld, thr + f * A.L.ld, A.L.cfg, out + f * A.L.cap, A.L.cap, lane);
    if (lane == 0 && b == nb) {
        counts[f] = sc.cnt;
        if (status) status[f] = sc.cnt > A.L.cap ? 3 : 0;
    }
}

template <typename T>
int launch_welch_t(msd_welch_plan *p, const void *x, const int64_t *off, const int64_t *len, int64_t nfiles,
                   int64_t max_blocks, double *band_db, int64_t ld, double *psd) {
    const msd_welch_cfg &c = p->cfg;
    WelchArgs A{};
    A.nfiles = nfiles;
    A.max_blocks = max_blocks;
    A.ld = ld;
    A.block_size = c.block_size;
    A.nperseg = c.nperseg;
    A.step = p->step;
    A.nseg = p->nseg;
    A.nfft = c.nfft;
    A.nslots = p->nslots;
    A.nbands = c.nbands;
    A.wave_lds = ((c.nperseg + 1) & ~1) + ((p->nslots + 1) & ~1);
    A.sample_scale = c.sample_scale;
    A.scale = c.scale;
    int slot = 0;
    for (int j = 0; j < c.nbands; ++j) {
        A.band_lo[j] = c.band_lo[j];
        A.band_hi[j] = c.band_hi[j];
        A.band_slot0[j] = slot;
        if (c.band_hi[j] >= c.band_lo[j]) slot += c.band_hi[j] - c.band_lo[j] + 1;
    }
    // waves per workgroup: 4 unless one wave's segment + PSD buffer needs more of the LDS
    // (e.g. nperseg 4096 with a full 2049-bin PSD: 3)
    const size_t wave_bytes = sizeof(double) * (size_t)A.wave_lds;
    const int nw = (int)std::min<size_t>(WL_THREADS / 64, (160 * 1024) / wave_bytes);
    if (nw < 1) return fail(MSD_ERR_UNSUPPORTED, "welch: nperseg + band bins exceed the LDS budget");
    const size_t lds = wave_bytes * nw;
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(welch_bands_kernel<T>), 160 * 1024)) return rc;
    const int64_t grid = (nfiles * max_blocks + nw - 1) / nw;  // a wave per block
    if (grid > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, "welch: grid too large");
    KernelTimer timer(p->ctx, K_WELCH);
    hipLaunchKernelGGL(welch_bands_kernel<T>, dim3((unsigned)grid), dim3(64 * nw), lds, p->ctx->stream,
                       static_cast<const T *>(x), off, len, A, p->d_window.get(), p->d_bins.get(), band_db, psd);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

int launch_welch(msd_welch_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len, int64_t nfiles,
                 int64_t max_blocks, double *band_db, int64_t ld, double *psd) {
    if (nfiles == 0 || max_blocks == 0) return MSD_OK;
    if (dtype == MSD_I16 && p->d_i8.get() && !p->ctx->welch_goertzel)  // the exact integer DFT (welch_i8.hip)
        return launch_welch_i8(p, static_cast<const int16_t *>(x), off, len, nfiles, max_blocks, band_db, ld, psd);
    switch (dtype) {
        case MSD_U8: return launch_welch_t<uint8_t>(p, x, off, len, nfiles, max_blocks, band_db, ld, psd);
        case MSD_I16: return launch_welch_t<int16_t>(p, x, off, len, nfiles, max_blocks, band_db, ld, psd);
        case MSD_I32: return launch_welch_t<int32_t>(p, x, off, len, nfiles, max_blocks, band_db, ld, psd);
        case MSD_F32: return launch_welch_t<float>(p, x, off, len, nfiles, max_blocks, band_db, ld, psd);
        case MSD_F64: return launch_welch_t<double>(p, x, off, len, nfiles, max_blocks, band_db, ld, psd);
        default: return fail(MSD_ERR_INVALID, "welch: unknown dtype");
    }
}

int launch_live(msd_ctx *ctx, const double *band_db, const int64_t *nblocks, int64_t nfiles, int64_t ld,
                const msd_live_cfg *cfg, msd_meteor *out, int64_t cap, int64_t *counts, double *thr, double *over,
                int32_t *status) {
    if (nfiles == 0) return MSD_OK;
    LiveArgs A{};
    A.cfg = *cfg;
    A.nfiles = nfiles;
    A.ld = ld;
    A.cap = cap;
    KernelTimer timer(ctx, K_LIVE);
    if (ld > 0) {  // grid width: the leading dimension bounds every file's block count
        const dim3 grid((unsigned)((ld + WL_THREADS - 1) / WL_THREADS), (unsigned)nfiles);
        hipLaunchKernelGGL(live_over_kernel, grid, dim3(WL_THREADS), 0, ctx->stream, band_db, nblocks, A, over);
        hipLaunchKernelGGL(live_history_kernel, grid, dim3(WL_THREADS), 0, ctx->stream, nblocks, A, over, thr);
    }
    LiveSegArgs G{};
    G.L = A;
    G.smax = ld > 0 ? (ld + LV_SEGLEN - 1) / LV_SEGLEN : 1;
    const int64_t nseg = nfiles * G.smax;
    const size_t b_state = sizeof(LiveScan) * (size_t)nseg, b_cnt = sizeof(int64_t) * (size_t)nseg,
                 b_act = sizeof(int32_t) * (size_t)nseg;
    void *sp = nullptr;
    if (int rc = ctx_scratch(ctx, SCRATCH_LIVE_SEGMENTS, 2 * b_state + b_cnt + b_act + 64, &sp)) return rc;
    char *base = static_cast<char *>(sp);
    LiveSegState S;
    S.in = reinterpret_cast<LiveScan *>(base);
    S.out = reinterpret_cast<LiveScan *>(base + b_state);
    S.cnt = reinterpret_cast<int64_t *>(base + 2 * b_state);
    S.active = reinterpret_cast<int32_t *>(base + 2 * b_state + b_cnt);
    S.changed = reinterpret_cast<int32_t *>(base + 2 * b_state + b_cnt + b_act);
    if (nseg > 0x7fffffffLL) return fail(MSD_ERR_UNSUPPORTED, "live: too many segments");
    const unsigned g_thr = (unsigned)((nseg + 255) / 256), g_wave = (unsigned)((nseg + 3) / 4);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(live_seg_init_kernel, dim3(g_thr), dim3(256), 0, st, nblocks, G, S, counts, status);
    // rounds: scan the active segments, then link every segment to its predecessor's exit.  The
    // first LV_ROUNDS go out unchecked (segments with nothing to do exit at once); then the flag of
    // the last link is read, and more rounds follow while it is set
    for (int64_t r = 0;; ++r) {
        hipLaunchKernelGGL(live_seg_scan_kernel, dim3(g_wave), dim3(256), 0, st, nblocks, G, S, over, thr);
        MSD_HIP(hipMemsetAsync(S.changed, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(live_seg_link_kernel, dim3(g_thr), dim3(256), 0, st, nblocks, G, S);
        if (r + 1 < LV_ROUNDS) continue;
        int32_t changed = 0;
        MSD_HIP(hipMemcpyAsync(&changed, S.changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        MSD_HIP(hipStreamSynchronize(st));
        if (!changed) break;
        if (r > G.smax + LV_ROUNDS) return fail(MSD_ERR_HIP, "live: segment states did not converge");
    }
    hipLaunchKernelGGL(live_seg_emit_kernel, dim3(g_wave), dim3(256), 0, st, nblocks, G, S, over, thr, out, counts,
                       status);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

// ---------------------------------------------------------------- live session (msdsp.h)
// Per stream f the device keeps an msd_live_stream_state and hist[f][0 .. retained): the over-noise
// values of the global blocks [base, blocks), base = blocks - retained.  A push appends its n new
// values behind them, computes the fresh thresholds with the look-back running into the tail, scans
// the new blocks from the carried state (one wave per stream, live_scan over global block indices)
// and shifts the tail down to the new keep.  The history and threshold pointers handed to live_scan
// are displaced so that the global block index addresses them (hist - base, thr - blocks); every
// index the scan and its event handlers form lies in [keep, blocks + n).
struct LsArgs {
    msd_live_cfg cfg;
    int64_t nstreams, max_blocks;  // max_blocks: this push's bound on the new blocks per stream
    int64_t H, hcap;               // hist_blocks, hcap = H + max_push_blocks doubles per stream
    int64_t cap;
};

__device__ __forceinline__ int64_t ls_new_blocks(const int64_t *nblocks, int64_t f, const LsArgs &A) {
    const int64_t n = nblocks[f];
    return n < 0 ? 0 : (n < A.max_blocks ? n : A.max_blocks);
}

// processor.py:391 for the push's new blocks, appended behind the retained tail
__global__ __launch_bounds__(WL_THREADS) void live_session_over_kernel(const double *__restrict__ band_db, int64_t ld,
                                                                        const int64_t *__restrict__ nblocks, LsArgs A,
                                                                        const msd_live_stream_state *__restrict__ st,
                                                                        double *__restrict__ hist,
                                                                        double *__restrict__ over, int64_t ld_over) {
    const int64_t f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * WL_THREADS + threadIdx.x;
    if (st[f].status == 4 || i >= ls_new_blocks(nblocks, f, A)) return;
    const double *sig = band_db + (f * 3 + 0) * ld;
    const double *n1 = band_db + (f * 3 + 1) * ld;
    const double *n2 = band_db + (f * 3 + 2) * ld;
    const double m = (0.0 + (-0.0 + n1[i] + n2[i])) / 2.0;  // np.add.reduce starts at +0.0 (np_reduce.h)
    const double v = sig[i] - m;
    hist[f * A.hcap + st[f].retained + i] = v;  // retained <= H, i < P
    over[f * ld_over + i] = v;
}

// processor.py:392-402 for the new blocks: the look-back runs into the tail (local index l of global
// block blocks + i; the tail starts at or before global block - W, or at block 0)
__global__ __launch_bounds__(WL_THREADS) void live_session_history_kernel(const int64_t *__restrict__ nblocks, LsArgs A,
                                                                           const msd_live_stream_state *__restrict__ st,
                                                                           const double *__restrict__ hist,
                                                                           double *__restrict__ thr, int64_t ld_thr) {
    const int64_t f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * WL_THREADS + threadIdx.x;
    if (st[f].status == 4 || i >= ls_new_blocks(nblocks, f, A)) return;
    const int64_t W = A.cfg.avg_win_blocks;
    const int64_t l = st[f].retained + i;
    const int64_t h0 = W > 0 ? (l - W > 0 ? l - W : 0) : 0;
    const int64_t hn = l - h0;
    double mean = NAN, sd = NAN;
    if (hn > 0) np_mean_std(hist + f * A.hcap, h0, hn, mean, sd);
    thr[f * ld_thr + i] = mean + A.cfg.k_std * sd;
}

// one wave per stream: the state machine over the new blocks from the carried state (thresholds used
// and meteors written), the exit state, and the tail shifted down to the new keep.  The shift is in
// place: this wave alone touches the stream's history, it moves 64 values per step downwards by
// shift >= 1, and step k's stores [64 k, 64 k + 64) lie below every later load (>= shift + 64 (k + 1)),
// so no load can see a moved value.
__global__ __launch_bounds__(256) void live_session_scan_kernel(const int64_t *__restrict__ nblocks, LsArgs A,
                                                                msd_live_stream_state *__restrict__ st,
                                                                double *__restrict__ hist, double *__restrict__ thr,
                                                                int64_t ld_thr, msd_meteor *__restrict__ out,
                                                                int64_t *__restrict__ counts,
                                                                int32_t *__restrict__ status,
                                                                int64_t *__restrict__ new_blocks,
                                                                const int64_t *__restrict__ new_rem) {
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= A.nstreams) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const msd_live_stream_state S = st[f];
    if (S.status == 4) {  // frozen: nothing consumed, nothing emitted
        if (lane == 0) {
            if (counts) counts[f] = 0;
            if (status) status[f] = 4;
            if (new_blocks) new_blocks[f] = 0;
        }
        return;
    }
    const int64_t n = ls_new_blocks(nblocks, f, A);
    const int64_t base = S.blocks - S.retained, nb2 = S.blocks + n;
    double *hf = hist + f * A.hcap;
    LiveScan sc;
    sc.state = S.state;
    sc.lock = S.lock;
    sc.until = S.until;
    sc.t_start = S.t_start;
    sc.trig = S.trig;
    sc.cnt = 0;  // meteors closed in this push
    live_scan<true>(sc, S.blocks, nb2, true, hf - base, thr + f * ld_thr - S.blocks, A.cfg, out + f * A.cap, A.cap,
                    lane);
    const int64_t W = A.cfg.avg_win_blocks;
    int64_t keep = W > 0 ? nb2 - W : 0;
    if (sc.state == 2 && sc.trig < keep) keep = sc.trig;
    if (keep < base) keep = base;
    const int64_t shift = keep - base, kept = nb2 - keep;
    if (shift > 0) {
        for (int64_t j0 = 0; j0 < kept; j0 += 64) {
            const int64_t j = j0 + lane;
            if (j < kept) {
                const double v = hf[shift + j];
                hf[j] = v;
            }
        }
    }
    if (lane == 0) {
        const bool overflow = kept > A.H;  // the next push's P values would no longer fit behind it
        msd_live_stream_state E;
        E.state = sc.state;
        E.status = overflow ? 4 : 0;
        E.blocks = nb2;
        E.trig = sc.trig;
        E.lock = sc.lock;
        E.until = sc.until;
        E.t_start = sc.t_start;
        E.meteors = S.meteors + sc.cnt;
        E.retained = kept;
        E.remainder = new_rem ? new_rem[f] : S.remainder;
        st[f] = E;
        if (counts) counts[f] = sc.cnt;
        if (status) status[f] = overflow ? 4 : (sc.cnt > A.cap ? 3 : 0);
        if (new_blocks) new_blocks[f] = n;
    }
}

// [carried remainder | new samples] of every stream into the staging buffer, and the Welch launch's
// offsets / lengths (whole blocks only), block counts and new remainder counts into meta [4][nstreams]
template <typename E>
__global__ __launch_bounds__(256) void live_session_gather_kernel(const E *__restrict__ x,
                                                                  const int64_t *__restrict__ off,
                                                                  const int64_t *__restrict__ len, int64_t max_len,
                                                                  int64_t nstreams, int64_t B,
                                                                  const msd_live_stream_state *__restrict__ st,
                                                                  const E *__restrict__ rem, E *__restrict__ stage,
                                                                  int64_t stride, int64_t *__restrict__ meta) {
    const int64_t f = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool frozen = st[f].status == 4;
    const int64_t r = st[f].remainder;  // < B
    int64_t L = len[f];
    L = L < 0 ? 0 : (L < max_len ? L : max_len);
    const int64_t total = r + L, nb = total / B;  // total < (P + 1) B <= stride
    if (j == 0) {
        meta[f] = f * stride;
        meta[nstreams + f] = frozen ? 0 : nb * B;
        meta[2 * nstreams + f] = frozen ? 0 : nb;
        meta[3 * nstreams + f] = frozen ? r : total - nb * B;
    }
    if (frozen || j >= total) return;
    stage[f * stride + j] = j < r ? rem[f * B + j] : x[off[f] + (j - r)];
}

// the samples behind the last whole block become the stream's remainder
template <typename E>
__global__ __launch_bounds__(256) void live_session_carry_kernel(int64_t nstreams, int64_t B,
                                                                 const msd_live_stream_state *__restrict__ st,
                                                                 const E *__restrict__ stage, int64_t stride,
                                                                 const int64_t *__restrict__ meta,
                                                                 E *__restrict__ rem) {
    const int64_t f = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (st[f].status == 4 || j >= meta[3 * nstreams + f]) return;
    rem[f * B + j] = stage[f * stride + meta[nstreams + f] + j];
}

__global__ __launch_bounds__(256) void live_session_reset_kernel(msd_live_stream_state *__restrict__ st, int64_t first,
                                                                 int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    msd_live_stream_state E;
    E.state = 0;
    E.status = 0;
    E.blocks = 0;
    E.trig = 0;
    E.lock = -1.0;
    E.until = -1.0;
    E.t_start = 0.0;
    E.meteors = 0;
    E.retained = 0;
    E.remainder = 0;
    st[first + i] = E;
}

}  // namespace
}  // namespace msd

using namespace msd;

struct msd_live_session {
    msd_ctx *ctx = nullptr;
    msd_live_cfg cfg{};
    msd_welch_plan *plan = nullptr;  // null: rows only
    int dtype = 0;
    int64_t F = 0, P = 0, H = 0, stride = 0;  // stride: samples per stream of the staging buffer
    DevBuf<msd_live_stream_state> d_state;
    DevBuf<double> d_hist;   // [F][H + P]
    DevBuf<double> d_thr;    // [F][P]      thresholds / over / band rows of a push whose caller
    DevBuf<double> d_over;   // [F][P]      passes no buffer of its own
    DevBuf<double> d_band;   // [F][3][P]
    DevBuf<char> d_stage;    // [F][stride] samples
    DevBuf<char> d_rem;      // [F][block_size] samples
    DevBuf<int64_t> d_meta;  // [4][F] gather's Welch offsets / lengths, block counts, remainders
    DevBuf<int64_t> d_aux;   // [4][F] the host forms' nblocks / off / len, counts, new blocks
    DevBuf<int32_t> d_status;
    ~msd_live_session() { msd_welch_plan_destroy(plan); }
};

namespace {

int ls_reset(msd_live_session *s, int64_t first, int64_t n) {
    hipLaunchKernelGGL(live_session_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->ctx->stream,
                       s->d_state.get(), first, n);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

// over, fresh thresholds, scan + exit state + compaction for the push's rows (ld: their stride)
int ls_detect(msd_live_session *s, const double *band_db, const int64_t *nblocks, int64_t max_blocks, int64_t ld,
              msd_meteor *out, int64_t cap, int64_t *counts, double *thr, int64_t ld_thr, double *over,
              int64_t ld_over, int32_t *status, int64_t *new_blocks, const int64_t *new_rem) {
    LsArgs A{};
    A.cfg = s->cfg;
    A.nstreams = s->F;
    A.max_blocks = max_blocks;
    A.H = s->H;
    A.hcap = s->H + s->P;
    A.cap = cap;
    hipStream_t st = s->ctx->stream;
    KernelTimer timer(s->ctx, K_LIVE);
    if (max_blocks > 0) {
        const dim3 grid((unsigned)((max_blocks + WL_THREADS - 1) / WL_THREADS), (unsigned)s->F);
        hipLaunchKernelGGL(live_session_over_kernel, grid, dim3(WL_THREADS), 0, st, band_db, ld, nblocks, A, s->d_state.get(),
                           s->d_hist.get(), over, ld_over);
        hipLaunchKernelGGL(live_session_history_kernel, grid, dim3(WL_THREADS), 0, st, nblocks, A, s->d_state.get(),
                           s->d_hist.get(), thr, ld_thr);
    }
    hipLaunchKernelGGL(live_session_scan_kernel, dim3((unsigned)((s->F + 3) / 4)), dim3(256), 0, st, nblocks, A,
                       s->d_state.get(), s->d_hist.get(), thr, ld_thr, out, counts, status, new_blocks, new_rem);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

template <typename E>
int ls_gather(msd_live_session *s, const void *x, const int64_t *off, const int64_t *len, int64_t max_len) {
    const int64_t B = s->cfg.block_size;
    hipStream_t st = s->ctx->stream;
    const dim3 grid((unsigned)((B + max_len + 255) / 256), (unsigned)s->F);
    KernelTimer timer(s->ctx, K_WELCH);  // the Welch launch's ingest
    E *stage = reinterpret_cast<E *>(s->d_stage.get()), *rem = reinterpret_cast<E *>(s->d_rem.get());
    hipLaunchKernelGGL(live_session_gather_kernel<E>, grid, dim3(256), 0, st, static_cast<const E *>(x), off, len,
                       max_len, s->F, B, s->d_state.get(), static_cast<const E *>(rem), stage, s->stride,
                       s->d_meta.get());
    hipLaunchKernelGGL(live_session_carry_kernel<E>, dim3((unsigned)((B + 255) / 256), (unsigned)s->F), dim3(256), 0,
                       st, s->F, B, s->d_state.get(), static_cast<const E *>(stage), s->stride, s->d_meta.get(), rem);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

}  // namespace

extern "C" {

int msd_welch_plan_create(msd_ctx *ctx, const msd_welch_cfg *cfg, const double *window, msd_welch_plan **out) {
    if (!ctx || !cfg || !window || !out) return fail(MSD_ERR_INVALID, "msd_welch_plan_create: null");
    *out = nullptr;
    const msd_welch_cfg &c = *cfg;
    if (c.block_size <= 0 || c.nperseg <= 0 || c.nperseg > c.block_size || c.noverlap < 0 ||
        c.noverlap >= c.nperseg || c.nfft < c.nperseg)
        return fail(MSD_ERR_INVALID, "msd_welch_plan_create: need 0 <= noverlap < nperseg <= block_size, nfft >= nperseg");
    if (c.nbands < 1 || c.nbands > MSD_WELCH_MAX_BANDS)
        return fail(MSD_ERR_INVALID, "msd_welch_plan_create: nbands out of range");
    std::vector<double> bins;
    int nslots = 0;
    for (int j = 0; j < c.nbands; ++j) {
        if (c.band_hi[j] < c.band_lo[j]) continue;
        if (c.band_lo[j] < 0 || c.band_hi[j] > c.nfft / 2)
            return fail(MSD_ERR_INVALID, "msd_welch_plan_create: band bins outside 0..nfft/2");
        for (int k = c.band_lo[j]; k <= c.band_hi[j]; ++k) {
            const double w = 2.0 * M_PI * (double)k / (double)c.nfft;
            const bool edge = k == 0 || (c.nfft % 2 == 0 && k == c.nfft / 2);
            bins.push_back(std::cos(w));
            bins.push_back(std::sin(w));
            bins.push_back(2.0 * std::cos(w));
            bins.push_back(edge ? 1.0 : 2.0);
            ++nslots;
        }
    }
    DeviceGuard g(ctx->device);
    auto p = std::make_unique<msd_welch_plan>();
    p->ctx = ctx;
    p->cfg = c;
    p->step = c.nperseg - c.noverlap;
    p->nseg = (c.block_size - c.nperseg) / p->step + 1;
    p->nslots = nslots;
    if (!nslots) bins.resize(4, 0.0);  // d_bins is never empty
    int rc;
    (rc = p->d_window.upload(window, c.nperseg, "msd_welch_plan_create")) ||
        (rc = p->d_bins.upload(bins.data(), bins.size(), "msd_welch_plan_create"));
    if (!rc && welch_i8_shape(c, p->nseg, nslots, window)) rc = welch_i8_build(p.get(), window);  // int16 on the matrix cores
    if (rc) return rc;
    *out = p.release();
    return MSD_OK;
}

void msd_welch_plan_destroy(msd_welch_plan *p) { destroy_plan(p); }

int msd_welch_bands_dev(msd_welch_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len,
                        int64_t nfiles, int64_t max_blocks, double *band_db, int64_t ld, double *psd) {
    if (!p || (nfiles > 0 && (!x || !off || !len || !band_db))) return fail(MSD_ERR_INVALID, "msd_welch_bands_dev: null");
    if (ld < max_blocks) return fail(MSD_ERR_INVALID, "msd_welch_bands_dev: ld < max_blocks");
    DeviceGuard g(p->ctx->device);
    return launch_welch(p, x, dtype, off, len, nfiles, max_blocks, band_db, ld, psd);
}

int msd_welch_bands(msd_welch_plan *p, const void *x, int dtype, int64_t n, double *band_db, int64_t *blocks) {
    if (!p || (!x && n) || !band_db) return fail(MSD_ERR_INVALID, "msd_welch_bands: null");
    const size_t es = dtype_size(dtype);
    if (!es) return fail(MSD_ERR_INVALID, "msd_welch_bands: unknown dtype");
    const int64_t B = p->cfg.block_size;
    const int64_t nb = n >= B ? (n - B) / B + 1 : 0;
    if (blocks) *blocks = nb;
    if (nb == 0) return MSD_OK;
    msd_ctx *ctx = p->ctx;
    DeviceGuard g(ctx->device);
    const void *dx;
    const int64_t *doff;
    void *dout;
    int rc;
    const int nbands = p->cfg.nbands;
    if ((rc = stage_one_file(ctx, x, (size_t)n * es, n, &dx, &doff))) return rc;
    if ((rc = ctx_scratch(ctx, SCRATCH_OUTPUT, sizeof(double) * nbands * nb, &dout))) return rc;
    rc = launch_welch(p, dx, dtype, doff, doff + 1, 1, nb, static_cast<double *>(dout), nb, nullptr);
    if (rc) return rc;
    MSD_HIP(hipMemcpyAsync(band_db, dout, sizeof(double) * nbands * nb, hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    return MSD_OK;
}

int msd_welch_psd(msd_welch_plan *p, const void *x, int dtype, int64_t n, double *psd, int64_t *blocks) {
    if (!p || (!x && n) || !psd) return fail(MSD_ERR_INVALID, "msd_welch_psd: null");
    const size_t es = dtype_size(dtype);
    if (!es) return fail(MSD_ERR_INVALID, "msd_welch_psd: unknown dtype");
    const int64_t B = p->cfg.block_size;
    const int64_t nb = n >= B ? (n - B) / B + 1 : 0;
    if (blocks) *blocks = nb;
    if (nb == 0) return MSD_OK;
    msd_ctx *ctx = p->ctx;
    DeviceGuard g(ctx->device);
    const void *dx;
    const int64_t *doff;
    void *dout;
    int rc;
    const int nbands = p->cfg.nbands;
    const size_t band_bytes = sizeof(double) * nbands * nb, psd_bytes = sizeof(double) * (size_t)p->nslots * nb;
    if ((rc = stage_one_file(ctx, x, (size_t)n * es, n, &dx, &doff))) return rc;
    if ((rc = ctx_scratch(ctx, SCRATCH_OUTPUT, band_bytes + psd_bytes, &dout))) return rc;
    double *dband = static_cast<double *>(dout);
    double *dpsd = reinterpret_cast<double *>(static_cast<char *>(dout) + band_bytes);
    rc = launch_welch(p, dx, dtype, doff, doff + 1, 1, nb, dband, nb, dpsd);
    if (rc) return rc;
    MSD_HIP(hipMemcpyAsync(psd, dpsd, psd_bytes, hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    return MSD_OK;
}

static int check_live_cfg(const msd_live_cfg *c) {
    if (!c) return fail(MSD_ERR_INVALID, "live: null cfg");
    if (c->block_size <= 0 || !(c->fs > 0) || c->avg_win_blocks < 0)
        return fail(MSD_ERR_INVALID, "live: block_size, fs must be > 0 and avg_win_blocks >= 0");
    return MSD_OK;
}

int msd_live_detect_dev(msd_ctx *ctx, const double *band_db, const int64_t *nblocks, int64_t nfiles, int64_t ld,
                        const msd_live_cfg *cfg, msd_meteor *out, int64_t cap, int64_t *counts, double *thresholds,
                        double *over, int32_t *status) {
    if (!ctx || (nfiles > 0 && (!band_db || !nblocks || !counts || !thresholds || !over || (!out && cap))))
        return fail(MSD_ERR_INVALID, "msd_live_detect_dev: null (thresholds and over are required scratch here)");
    int rc = check_live_cfg(cfg);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    return launch_live(ctx, band_db, nblocks, nfiles, ld, cfg, out, cap, counts, thresholds, over, status);
}

int msd_live_detect(msd_ctx *ctx, const double *band_db, int64_t nb, const msd_live_cfg *cfg, msd_meteor *out,
                    int64_t cap, int64_t *count, double *thresholds, double *over) {
    if (!ctx || (!band_db && nb) || (!out && cap) || !count) return fail(MSD_ERR_INVALID, "msd_live_detect: null");
    int rc = check_live_cfg(cfg);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    const int64_t ld = nb > 0 ? nb : 1;
    const int64_t dcap = cap > 0 ? cap : 1;
    // scratch: band_db[3*ld] | over[ld] | thr[ld] | nb | count | status(pad) | meteors[dcap]
    const size_t head = sizeof(double) * 5 * ld + 32;
    void *s;
    if ((rc = ctx_scratch(ctx, SCRATCH_DETECTIONS, head + sizeof(msd_meteor) * dcap, &s))) return rc;
    char *base = static_cast<char *>(s);
    double *dband = reinterpret_cast<double *>(base);
    double *dover = dband + 3 * ld;
    double *dthr = dover + ld;
    int64_t *dnb = reinterpret_cast<int64_t *>(dthr + ld);
    int64_t *dcount = dnb + 1;
    int32_t *dstatus = reinterpret_cast<int32_t *>(dcount + 1);
    msd_meteor *dmet = reinterpret_cast<msd_meteor *>(base + head);
    if (nb) MSD_HIP(hipMemcpyAsync(dband, band_db, sizeof(double) * 3 * nb, hipMemcpyHostToDevice, ctx->stream));
    MSD_HIP(hipMemcpyAsync(dnb, &nb, sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    // band_db rows were packed with ld = nb
    rc = launch_live(ctx, dband, dnb, 1, ld, cfg, dmet, dcap, dcount, dthr, dover, dstatus);
    if (rc) return rc;
    int64_t cnt = 0;
    MSD_HIP(hipMemcpyAsync(&cnt, dcount, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    *count = cnt;
    const int64_t ncopy = cnt < cap ? cnt : cap;
    if (ncopy > 0)
        MSD_HIP(hipMemcpyAsync(out, dmet, sizeof(msd_meteor) * ncopy, hipMemcpyDeviceToHost, ctx->stream));
    if (thresholds && nb)
        MSD_HIP(hipMemcpyAsync(thresholds, dthr, sizeof(double) * nb, hipMemcpyDeviceToHost, ctx->stream));
    if (over && nb) MSD_HIP(hipMemcpyAsync(over, dover, sizeof(double) * nb, hipMemcpyDeviceToHost, ctx->stream));
    MSD_HIP(hipStreamSynchronize(ctx->stream));
    if (cnt > cap) return fail(MSD_ERR_CAPACITY, "live: more meteors than capacity");
    return MSD_OK;
}

int msd_live_session_create(msd_ctx *ctx, const msd_live_cfg *cfg, const msd_welch_cfg *welch, const double *window,
                            int64_t nstreams, int64_t max_push_blocks, int64_t hist_blocks, int dtype,
                            msd_live_session **out) {
    if (!out || !cfg) return fail(MSD_ERR_INVALID, "msd_live_session_create: null cfg or out");
    *out = nullptr;
    int rc = check_live_cfg(cfg);
    if (rc) return rc;
    if (nstreams < 1 || nstreams > 0x7fffffLL) return fail(MSD_ERR_INVALID, "msd_live_session_create: nstreams < 1");
    if (max_push_blocks < 1) return fail(MSD_ERR_INVALID, "msd_live_session_create: max_push_blocks < 1");
    if (hist_blocks < cfg->avg_win_blocks)
        return fail(MSD_ERR_INVALID, "msd_live_session_create: hist_blocks < avg_win_blocks");
    if (welch) {
        if (!window) return fail(MSD_ERR_INVALID, "msd_live_session_create: null window");
        if (welch->block_size != cfg->block_size || welch->nbands != 3)
            return fail(MSD_ERR_INVALID, "msd_live_session_create: welch needs cfg's block_size and 3 bands");
        if (!dtype_size(dtype)) return fail(MSD_ERR_INVALID, "msd_live_session_create: unknown dtype");
    }
    if (!ctx) return fail(MSD_ERR_INVALID, "msd_live_session_create: null ctx");
    DeviceGuard g(ctx->device);
    auto *s = new msd_live_session();
    s->ctx = ctx;
    s->cfg = *cfg;
    s->dtype = dtype;
    s->F = nstreams;
    s->P = max_push_blocks;
    s->H = hist_blocks;
    const size_t F = (size_t)nstreams, P = (size_t)max_push_blocks, H = (size_t)hist_blocks;
    const char *what = "msd_live_session_create";
    (rc = s->d_state.alloc(F, what)) || (rc = s->d_hist.alloc(F * (H + P), what)) ||
        (rc = s->d_thr.alloc(F * P, what)) || (rc = s->d_over.alloc(F * P, what)) ||
        (rc = s->d_meta.alloc(4 * F, what)) || (rc = s->d_aux.alloc(4 * F, what)) || (rc = s->d_status.alloc(F, what));
    if (!rc && welch) {
        const size_t es = dtype_size(dtype), B = (size_t)cfg->block_size;
        s->stride = (int64_t)(((P + 1) * B + 63) / 64 * 64);  // every stream's blocks aligned as a file's are
        (rc = s->d_band.alloc(F * 3 * P, what)) || (rc = s->d_stage.alloc(es * F * (size_t)s->stride + 256, what)) ||
            (rc = s->d_rem.alloc(es * F * B, what)) || (rc = msd_welch_plan_create(ctx, welch, window, &s->plan));
    }
    if (rc || (rc = ls_reset(s, 0, s->F))) {
        msd_live_session_destroy(s);  // (drains the stream: the reset may be in flight)
        return rc;
    }
    *out = s;
    return MSD_OK;
}

void msd_live_session_destroy(msd_live_session *s) { destroy_plan(s); }

int msd_live_session_push_rows_dev(msd_live_session *s, const double *band_db, const int64_t *nblocks,
                                   int64_t max_blocks, int64_t ld, msd_meteor *out, int64_t cap, int64_t *counts,
                                   double *thresholds, double *over, int32_t *status) {
    if (!s || !nblocks || (max_blocks > 0 && !band_db) || (!out && cap))
        return fail(MSD_ERR_INVALID, "msd_live_session_push_rows_dev: null");
    if (max_blocks < 0 || max_blocks > s->P || max_blocks > ld || cap < 0)
        return fail(MSD_ERR_INVALID, "msd_live_session_push_rows_dev: need 0 <= max_blocks <= min(ld, max_push_blocks)");
    DeviceGuard g(s->ctx->device);
    return ls_detect(s, band_db, nblocks, max_blocks, ld, out, cap, counts, thresholds ? thresholds : s->d_thr.get(),
                     thresholds ? ld : s->P, over ? over : s->d_over.get(), over ? ld : s->P, status, nullptr, nullptr);
}

int msd_live_session_push_samples_dev(msd_live_session *s, const void *x, const int64_t *off, const int64_t *len,
                                      int64_t max_len, msd_meteor *out, int64_t cap, int64_t *counts,
                                      int64_t *new_blocks, double *band_db, double *thresholds, double *over,
                                      int64_t ld, int32_t *status) {
    if (!s || !off || !len || (max_len > 0 && !x) || (!out && cap))
        return fail(MSD_ERR_INVALID, "msd_live_session_push_samples_dev: null");
    if (!s->plan) return fail(MSD_ERR_INVALID, "msd_live_session_push_samples_dev: the session takes rows only");
    const int64_t B = s->cfg.block_size;
    if (max_len < 0 || max_len > s->P * B || cap < 0)
        return fail(MSD_ERR_INVALID, "msd_live_session_push_samples_dev: need 0 <= max_len <= max_push_blocks * block_size");
    const int64_t max_blocks = (B - 1 + max_len) / B;  // <= P
    if ((band_db || thresholds || over) && ld < max_blocks)
        return fail(MSD_ERR_INVALID, "msd_live_session_push_samples_dev: ld < (block_size - 1 + max_len) / block_size");
    DeviceGuard g(s->ctx->device);
    int rc;
    switch (dtype_size(s->dtype)) {
        case 1: rc = ls_gather<uint8_t>(s, x, off, len, max_len); break;
        case 2: rc = ls_gather<uint16_t>(s, x, off, len, max_len); break;
        case 4: rc = ls_gather<uint32_t>(s, x, off, len, max_len); break;
        default: rc = ls_gather<uint64_t>(s, x, off, len, max_len); break;
    }
    if (rc) return rc;
    double *band = band_db ? band_db : s->d_band.get();
    const int64_t ld_band = band_db ? ld : s->P;
    const int64_t F = s->F;
    if ((rc = launch_welch(s->plan, s->d_stage.get(), s->dtype, s->d_meta.get(), s->d_meta.get() + F, F, max_blocks, band, ld_band,
                           nullptr)))
        return rc;
    return ls_detect(s, band, s->d_meta.get() + 2 * F, max_blocks, ld_band, out, cap, counts,
                     thresholds ? thresholds : s->d_thr.get(), thresholds ? ld : s->P, over ? over : s->d_over.get(),
                     over ? ld : s->P, status, new_blocks, s->d_meta.get() + 3 * F);
}

// the host forms' epilogue: stream f's count, status, meteors and the new blocks' values to the host
static int ls_fetch(msd_live_session *s, int64_t f, const msd_meteor *dmet, int64_t cap,
                    msd_meteor *out, int64_t *count, int64_t *new_blocks, double *band_db, double *thresholds,
                    double *over, int64_t ld, int32_t *status) {
    hipStream_t st = s->ctx->stream;
    const int64_t F = s->F;
    int64_t cnt = 0, nb = 0;
    int32_t stat = 0;
    MSD_HIP(hipMemcpyAsync(&cnt, s->d_aux.get() + 2 * F + f, sizeof(cnt), hipMemcpyDeviceToHost, st));
    MSD_HIP(hipMemcpyAsync(&stat, s->d_status.get() + f, sizeof(stat), hipMemcpyDeviceToHost, st));
    MSD_HIP(hipMemcpyAsync(&nb, s->d_aux.get() + 3 * F + f, sizeof(nb), hipMemcpyDeviceToHost, st));
    MSD_HIP(hipStreamSynchronize(st));
    *count = cnt;
    if (new_blocks) *new_blocks = nb;
    if (status) *status = stat;
    const int64_t ncopy = cnt < cap ? cnt : cap;
    if (ncopy > 0) MSD_HIP(hipMemcpyAsync(out, dmet + f * cap, sizeof(msd_meteor) * ncopy, hipMemcpyDeviceToHost, st));
    if (nb > 0) {
        const size_t bytes = sizeof(double) * (size_t)nb;
        if (band_db)
            for (int j = 0; j < 3; ++j)
                MSD_HIP(hipMemcpyAsync(band_db + j * ld, s->d_band.get() + (f * 3 + j) * s->P, bytes, hipMemcpyDeviceToHost, st));
        if (thresholds) MSD_HIP(hipMemcpyAsync(thresholds, s->d_thr.get() + f * s->P, bytes, hipMemcpyDeviceToHost, st));
        if (over) MSD_HIP(hipMemcpyAsync(over, s->d_over.get() + f * s->P, bytes, hipMemcpyDeviceToHost, st));
    }
    MSD_HIP(hipStreamSynchronize(st));
    if (cnt > cap) return fail(MSD_ERR_CAPACITY, "live session: more meteors than capacity");
    return MSD_OK;
}

int msd_live_session_push_rows(msd_live_session *s, int64_t stream, const double *band_db, int64_t nb,
                               msd_meteor *out, int64_t cap, int64_t *count, double *thresholds, double *over,
                               int32_t *status) {
    if (!s || (!band_db && nb) || (!out && cap) || !count) return fail(MSD_ERR_INVALID, "msd_live_session_push_rows: null");
    if (stream < 0 || stream >= s->F || nb < 0 || nb > s->P || cap < 0)
        return fail(MSD_ERR_INVALID, "msd_live_session_push_rows: stream or nb (<= max_push_blocks) out of range");
    msd_ctx *ctx = s->ctx;
    DeviceGuard g(ctx->device);
    const int64_t F = s->F, ld = nb > 0 ? nb : 1, dcap = cap > 0 ? cap : 1;
    // scratch: the rows of every stream slot [F][3][ld] (only `stream`'s are read) | meteors [F][dcap]
    const size_t b_rows = sizeof(double) * 3 * (size_t)ld * (size_t)F;
    void *sp;
    int rc;
    if ((rc = ctx_scratch(ctx, SCRATCH_DETECTIONS, b_rows + sizeof(msd_meteor) * (size_t)dcap * (size_t)F, &sp))) return rc;
    double *drows = static_cast<double *>(sp);
    msd_meteor *dmet = reinterpret_cast<msd_meteor *>(static_cast<char *>(sp) + b_rows);
    std::vector<int64_t> nbs((size_t)F, 0);
    nbs[(size_t)stream] = nb;
    hipStream_t st = ctx->stream;
    if (nb) MSD_HIP(hipMemcpyAsync(drows + stream * 3 * ld, band_db, sizeof(double) * 3 * nb, hipMemcpyHostToDevice, st));
    MSD_HIP(hipMemcpyAsync(s->d_aux.get(), nbs.data(), sizeof(int64_t) * F, hipMemcpyHostToDevice, st));
    MSD_HIP(hipStreamSynchronize(st));  // nbs leaves scope below
    if ((rc = ls_detect(s, drows, s->d_aux.get(), nb, ld, dmet, dcap, s->d_aux.get() + 2 * F, s->d_thr.get(), s->P, s->d_over.get(), s->P,
                        s->d_status.get(), s->d_aux.get() + 3 * F, nullptr)))
        return rc;
    return ls_fetch(s, stream, dmet, dcap, out, count, nullptr, nullptr, thresholds, over, 0, status);
}

int msd_live_session_push_samples(msd_live_session *s, int64_t stream, const void *x, int64_t n, msd_meteor *out,
                                  int64_t cap, int64_t *count, int64_t *new_blocks, double *band_db,
                                  double *thresholds, double *over, int64_t ld, int32_t *status) {
    if (!s || (!x && n) || (!out && cap) || !count) return fail(MSD_ERR_INVALID, "msd_live_session_push_samples: null");
    if (!s->plan) return fail(MSD_ERR_INVALID, "msd_live_session_push_samples: the session takes rows only");
    const int64_t B = s->cfg.block_size;
    if (stream < 0 || stream >= s->F || n < 0 || n > s->P * B || cap < 0)
        return fail(MSD_ERR_INVALID, "msd_live_session_push_samples: stream or n (<= max_push_blocks * block_size) out of range");
    if ((band_db || thresholds || over) && ld < (B - 1 + n) / B)
        return fail(MSD_ERR_INVALID, "msd_live_session_push_samples: ld < (block_size - 1 + n) / block_size");
    msd_ctx *ctx = s->ctx;
    DeviceGuard g(ctx->device);
    const int64_t F = s->F, dcap = cap > 0 ? cap : 1;
    const size_t es = dtype_size(s->dtype);
    void *dx, *dm;
    int rc;
    if ((rc = ctx_scratch(ctx, SCRATCH_SAMPLES, ((size_t)n * es + 255) / 256 * 256, &dx))) return rc;
    if ((rc = ctx_scratch(ctx, SCRATCH_DETECTIONS, sizeof(msd_meteor) * (size_t)dcap * (size_t)F, &dm))) return rc;
    msd_meteor *dmet = static_cast<msd_meteor *>(dm);
    std::vector<int64_t> meta((size_t)(2 * F), 0);  // off | len
    meta[(size_t)(F + stream)] = n;
    hipStream_t st = ctx->stream;
    if (n) MSD_HIP(hipMemcpyAsync(dx, x, (size_t)n * es, hipMemcpyHostToDevice, st));
    MSD_HIP(hipMemcpyAsync(s->d_aux.get(), meta.data(), sizeof(int64_t) * 2 * F, hipMemcpyHostToDevice, st));
    MSD_HIP(hipStreamSynchronize(st));  // meta leaves scope below
    if ((rc = msd_live_session_push_samples_dev(s, dx, s->d_aux.get(), s->d_aux.get() + F, n, dmet, dcap, s->d_aux.get() + 2 * F,
                                                s->d_aux.get() + 3 * F, nullptr, nullptr, nullptr, 0, s->d_status.get())))
        return rc;
    return ls_fetch(s, stream, dmet, dcap, out, count, new_blocks, band_db, thresholds, over, ld, status);
}

int msd_live_session_state(msd_live_session *s, int64_t first, int64_t n, msd_live_stream_state *out) {
    if (!s || (!out && n)) return fail(MSD_ERR_INVALID, "msd_live_session_state: null");
    if (first < 0 || n < 0 || first + n > s->F) return fail(MSD_ERR_INVALID, "msd_live_session_state: streams out of range");
    if (!n) return MSD_OK;
    DeviceGuard g(s->ctx->device);
    MSD_HIP(hipMemcpyAsync(out, s->d_state.get() + first, sizeof(msd_live_stream_state) * (size_t)n, hipMemcpyDeviceToHost,
                           s->ctx->stream));
    MSD_HIP(hipStreamSynchronize(s->ctx->stream));
    return MSD_OK;
}

int msd_live_session_history(msd_live_session *s, int64_t stream, double *out, int64_t cap, int64_t *n) {
    if (!s || !n || (!out && cap)) return fail(MSD_ERR_INVALID, "msd_live_session_history: null");
    if (stream < 0 || stream >= s->F || cap < 0) return fail(MSD_ERR_INVALID, "msd_live_session_history: stream out of range");
    msd_live_stream_state S;
    if (int rc = msd_live_session_state(s, stream, 1, &S)) return rc;
    *n = S.retained;
    const int64_t m = S.retained < cap ? S.retained : cap;
    if (m <= 0) return MSD_OK;
    DeviceGuard g(s->ctx->device);
    MSD_HIP(hipMemcpyAsync(out, s->d_hist.get() + stream * (s->H + s->P), sizeof(double) * (size_t)m, hipMemcpyDeviceToHost,
                           s->ctx->stream));
    MSD_HIP(hipStreamSynchronize(s->ctx->stream));
    return MSD_OK;
}

int msd_live_session_reset(msd_live_session *s, int64_t stream) {
    if (!s) return fail(MSD_ERR_INVALID, "msd_live_session_reset: null");
    if (stream < -1 || stream >= s->F) return fail(MSD_ERR_INVALID, "msd_live_session_reset: stream out of range");
    DeviceGuard g(s->ctx->device);
    return stream < 0 ? ls_reset(s, 0, s->F) : ls_reset(s, stream, 1);
}

}  // extern "C"
