// Fast path of the STFT power spectrogram for nperseg = nfft = 1024 (the headline
// configuration: scipy.signal.spectrogram(x, fs, 'hann', 1024, 512) as called at
// dsp/src/main.py:52-54 / :132-133 and BASELINE configs C1-C4).
//
// Mapping (measured in profiles/stft1024_xwave_ab.txt: 5.564 against 5.713 ms per C3 launch for the
// mapping before it, in which a wave kept its two frames through pass 3 and the powers left through an
// LDS tile; LDS issue cycles -19 %, VALU instructions -3.7 %, no bank conflicts).  One workgroup = 16 waves (4 per SIMD: one wave alone issues a VALU op
// only every ~4 cycles, so the SIMD needs several) = one tile of 32 consecutive frames.  Every
// radix-8 Stockham pass runs in registers, 8 complex points per lane and stream, two independent
// instruction streams per wave (interleaved by the compiler):
//   passes 1 and 2 by frame: wave w owns the frame pair (2w, 2w + 1) of the tile, one frame per stream,
//   64 lanes x 8 points;
//   load    lane l holds z[l + 64 r] = x[2(l+64r)] + i x[2(l+64r)+1] (r = 0..7): one
//           sample pair per lane per instruction, 256 B coalesced per wave;
//   detrend frame mean from an exact integer reduction: DPP adds inside each row of
//           16 lanes, then four v_readlane (no LDS round trip);
//   pass 1  → transpose through the frame's LDS region → pass 2 → the frame's LDS region;
//   pass 3 by bin, across the workgroup: the 64 pass-3 butterflies are 32 slots, the conjugate pairs
//           (j, 64 - j), j = 1..31, and the self-conjugate (0, 32); a half-wave owns one slot and its 32
//           lanes are the tile's 32 frames.  Stream A is butterfly j, stream B butterfly 64 - j, so a
//           lane holds Z[j + 64 r] and its conjugate partner Z[512 - j - 64 r] (B's register 7 - r) of
//           its own frame: no cross-lane traffic.  B's twiddles are the conjugates of A's, its DFT8
//           outputs A's formula shifted by one index (W512^((64-j) r) = W8^r conj(W512^(j r)));
//   post    real-spectrum split, |X|^2 * scale (x2 off DC / Nyquist): a lane holds one column entry
//           of 16 rows (17 in slot 0), and each row leaves as one non-temporal dword store in
//           which each half-wave writes one 128-B row segment, straight from registers.
// Workgroups are persistent and walk a contiguous range of tiles (the half frame shared by
// neighbouring tiles is re-read from L2); each wave loads its next tile's frame pair
// into the sample registers as soon as the current pair is windowed.
#include <vector>

#include "fft_butterfly.h"
#include "msd_internal.h"

#include <cmath>
#include <type_traits>

namespace msd {
namespace {

constexpr int F_NW = 16;                  // waves per workgroup (4 per SIMD)
constexpr int F_TT = 32;                  // frames per tile
constexpr int F_K = 513;                  // one-sided bins
constexpr int F_SCRF = 576;               // float2 per frame region (phys(511) = 571)
// Frame buffer: one region per frame of the tile.  Frame f sits at (f >> 1) * F_PAIRF + (f & 1) * F_SCRF
// and holds point n at phys(n) ^ (f & 1).  In the pass-3 reads the 32 lanes of a ds_read_b64 group read
// the same point of the 32 frames: with F_PAIRF = 2 (mod 32) the pair bases take the 16 even float2
// banks and the parity flip the odd ones, so the group covers all 64 banks once.  Every base stays
// 16-B aligned for the pass-1 ds_write_b128 (an odd frame swaps the two float2 of a write instead),
// and inside a frame the flip only permutes banks, so the phys() patterns stay conflict-free
// (tools/lds_bank_model.py checks every access pattern of the kernel).
constexpr int F_PAIRF = 2 * F_SCRF + 2;
constexpr int F_TAB_OFF = (F_TT / 2) * F_PAIRF * 8;
// per-lane constants, one 144-B row per lane [lane][18 float2]: window pairs w[2(l + 64 r)..] (r = 0..7,
// at 0) and pass-2 twiddles W64^{(l&7) r} (r = 1..7, at 8).  Read as ds_read_b128; the 36-dword row
// stride is 4 x odd, so a b128 lane group hits 16 disjoint 4-bank ranges (conflict-free)
constexpr int F_TABW = 18;
// per-slot constants, one 96-B row per slot [33][12 float2]: pass-3 twiddles W512^{j r} (r = 1..7, at 0)
// and post twiddles W1024^{j + 64 r} (r = 0..3, at 8; those of r + 4 are -i times these).  Row 32 is
// butterfly 32 of slot 0 (its post twiddles times i, so that the r >= 4 form applies).  A half-wave
// reads one address (broadcast)
constexpr int F_SLOT_OFF = F_TAB_OFF + F_TABW * 64 * 8;
constexpr int F_SLOTW = 12;
// integer samples: the frames' mean remainders, double-buffered by tile parity (written by the frame's
// wave before the pass-2 barrier, read by wave 0 in the post pass)
constexpr int F_RB_OFF = F_SLOT_OFF + 33 * F_SLOTW * 8;
constexpr int F_LDS = F_RB_OFF + 2 * F_TT * 4;
static_assert(F_LDS <= 160 * 1024, "LDS budget");
static_assert(F_PAIRF % 32 == 2 && F_TAB_OFF % 16 == 0 && F_SLOT_OFF % 16 == 0, "frame buffer banking / alignment");

// cadd / csub / cmul / mul_mi, dft4, dft8, dft8_windowed (host-checkable: butterfly_check.cpp)
using namespace bfly;

// a * conj(b)
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// Frame-region layout (float2 index): bit 4 of n flips bits 1 and 3, plus 4 float2 of
// padding per 32.  It makes the transposes' access patterns inside a frame (16-B pass-1 writes, 8-B
// reads, 8-B pass-2 writes) free of bank conflicts under the gfx950 LDS model — found by
// tools/lds_swizzle_search.py.  phys(n + 64 r) = phys(n) + 72 r.
__device__ __forceinline__ int phys(int n) { return (n ^ (((n >> 4) & 1) * 10)) + ((n >> 5) << 2); }

template <typename T>
struct PairIO;
template <>
struct PairIO<int16_t> {
    using raw_t = uint32_t;
    static constexpr bool kInt = true;
    __device__ static raw_t load(const int16_t *p) { return *reinterpret_cast<const uint32_t *>(p); }
    __device__ static raw_t zero() { return 0u; }
    __device__ static int ilo(raw_t r) { return (int)(int16_t)(r & 0xffffu); }
    __device__ static int ihi(raw_t r) { return (int)(int16_t)(r >> 16); }
    __device__ static float lo(raw_t r) { return cvt_i16_lo(r); }
    __device__ static float hi(raw_t r) { return cvt_i16_hi(r); }
    __device__ static int sum2(raw_t r, int acc) { return dot2_i16<1, 1>(r, acc); }
};
template <>
struct PairIO<uint8_t> {
    using raw_t = uint32_t;
    static constexpr bool kInt = true;
    __device__ static raw_t load(const uint8_t *p) { return *reinterpret_cast<const uint16_t *>(p); }
    __device__ static raw_t zero() { return 0u; }
    __device__ static int ilo(raw_t r) { return (int)(r & 0xffu); }
    __device__ static int ihi(raw_t r) { return (int)((r >> 8) & 0xffu); }
    __device__ static float lo(raw_t r) { return (float)ilo(r); }
    __device__ static float hi(raw_t r) { return (float)ihi(r); }
    __device__ static int sum2(raw_t r, int acc) { return acc + ilo(r) + ihi(r); }
};
template <>
struct PairIO<float> {
    using raw_t = float2;
    static constexpr bool kInt = false;
    __device__ static raw_t load(const float *p) { return *reinterpret_cast<const float2 *>(p); }
    __device__ static raw_t zero() { return make_float2(0.f, 0.f); }
    __device__ static int ilo(raw_t) { return 0; }
    __device__ static int ihi(raw_t) { return 0; }
    __device__ static float lo(raw_t r) { return r.x; }
    __device__ static float hi(raw_t r) { return r.y; }
};

// per-file geometry kept in scalar registers while a workgroup walks its tiles
struct FileCur {
    int64_t f, ti;  // file, tile within file
    int64_t nfr;    // frames in the file
    int64_t base;   // element offset of the file
};

// sample-pair registers per lane for the wave's frame pair (t, t + 1): frame t in raw[0..7], frame
// t + 1 in raw[RB..RB+7].  SH (hop 512, integer samples): frame t + 1 starts at frame t's
// sample 512, so its first half IS raw[4..7] (RB = 4, 12 registers, 12 loads instead of 16)
template <bool SH>
struct PairRegs {
    static constexpr int RB = SH ? 4 : 8;
    static constexpr int N = RB + 8;
};


template <typename T, bool SH>
__device__ __forceinline__ void load_pair(const T *__restrict__ x, const FileCur &fc, int64_t t, int hop, int l,
                                          typename PairIO<T>::raw_t (&raw)[PairRegs<SH>::N]) {
    using IO = PairIO<T>;
    constexpr int RB = PairRegs<SH>::RB;
    if (t < fc.nfr) {  // wave-uniform
        const T *p = x + uniform_i64(fc.base + t * (int64_t)hop) + 2 * l;
#pragma unroll
        for (int r = 0; r < 8; ++r) raw[r] = IO::load(p + 128 * r);
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) raw[r] = IO::zero();
    }
    constexpr int r0 = SH ? 4 : 0;  // SH: the second frame's first half is already in raw[4..7]
    if (t + 1 < fc.nfr) {
        const T *p = x + uniform_i64(fc.base + (t + 1) * (int64_t)hop) + 2 * l;
#pragma unroll
        for (int r = r0; r < 8; ++r) raw[RB + r] = IO::load(p + 128 * r);
    } else {
#pragma unroll
        for (int r = r0; r < 8; ++r) raw[RB + r] = IO::zero();
    }
}

// WIDE: 64-bit output offsets (files of 2^20 frames and more); SH: hop 512 with integer samples
// DYN: the workgroups take chunks of consecutive tiles from a guided schedule (sched[k] .. sched[k+1],
// at least 2 tiles) by an atomic ticket instead of one fixed range each (as cstft4096_kernel, where it
// balances the workgroups' unequal speeds); the next chunk's ticket is drawn when a chunk starts and
// read at its last tile, at least one tile barrier later.
template <typename T, int WIDE, bool SH, bool DYN = false>
__global__ __launch_bounds__(F_NW * 64, 1) void stft1024_kernel(
    const T *__restrict__ x, const int64_t *__restrict__ off, const int64_t *__restrict__ len,
    int64_t tiles_per_file, int64_t ntiles, int64_t tiles_per_wg, int hop, float wscale, int detrend,
    const float *__restrict__ g_win, const float2 *__restrict__ g_tw, const float2 *__restrict__ g_post,
    float *__restrict__ out, int64_t ld, const int64_t *__restrict__ sched, int64_t nchunks,
    unsigned long long *__restrict__ ticket, float2 dcw0, float2 dcw1) {
    using IO = PairIO<T>;
    using raw_t = typename IO::raw_t;
    // the transposes' LDS read bases held in 16 registers across the tile loop (read8 below) where that costs no
    // scratch: int16 and the hop-512 uint8 form with 32-bit offsets (116-122 VGPRs).  The float32 forms, uint8 at
    // other hops and every 64-bit-offset form sit at 118-128 VGPRs already and would spill 8-100 B
    constexpr bool HOIST = (std::is_same_v<T, int16_t> || SH) && !WIDE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    const int l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar frame addresses
    // passes 1 and 2: the regions of this wave's frames 2 wave (even) and 2 wave + 1 (odd)
    float2 *fb0 = buf + wave * F_PAIRF, *fb1 = fb0 + F_SCRF;
    float2 *t_all = reinterpret_cast<float2 *>(smem + F_TAB_OFF);
    float2 *s_all = reinterpret_cast<float2 *>(smem + F_SLOT_OFF);
    float *rbuf = reinterpret_cast<float *>(smem + F_RB_OFF);
    const float2 *tab = t_all + l * F_TABW;  // this lane's constants
    for (int i = tid; i < 64 * F_TABW; i += F_NW * 64) {
        const int li = i / F_TABW, c = i % F_TABW;
        float2 e = make_float2(0.f, 0.f);
        if (c < 8) {
            const float2 gw = *reinterpret_cast<const float2 *>(g_win + 2 * (li + 64 * c));
            e = make_float2(gw.x * wscale, gw.y * wscale);  // window * sqrt(scale / 2)
        } else if (c < 15) {
            e = g_tw[8 * (li & 7) * (c - 7)];
        }
        t_all[i] = e;
    }
    for (int i = tid; i < 33 * F_SLOTW; i += F_NW * 64) {
        const int j = i / F_SLOTW, c = i % F_SLOTW;  // row 32: butterfly 32
        float2 e = make_float2(0.f, 0.f);
        if (c < 7) {
            e = g_tw[j * (c + 1)];
        } else if (c >= 8) {
            e = g_post[j + 64 * (c - 8)];
            if (j == 32) e = make_float2(-e.y, e.x);  // times i
        }
        s_all[i] = e;
    }
    // Transpose addresses as lane bases plus compile-time offsets (LDS instruction immediates), q = 1 the
    // odd frame's (^ 1).  Pass-1 writes phys(8 l + r): bit 4 of 8 l + r is a lane bit and flips r's bit 1,
    // so r = 0, 4 go from wr0 and r = 2, 6 from wr2.  Pass-1 reads phys(l + 64 r) = phys(l) + 72 r.
    // Pass-2 writes phys(o2 + 8 r): bit 4 is r's bit 1, which flips bit 1 of the lane part o2 (w2[q][1]) and
    // bit 3 of 8 r; the padding is 8 (l >> 3) + 4 (r >> 2)
    const int wr0 = phys(8 * l), wr2 = phys(8 * l + 2);
    const int rd[2] = {phys(l), phys(l) ^ 1};
    const int o2 = 64 * (l >> 3) + (l & 7), o2p = 8 * (l >> 3);  // pass 2 (Ns = 8): out[o2 + 8 r]
    const int w2[2][2] = {{o2 + o2p, (o2 ^ 2) + o2p}, {(o2 ^ 1) + o2p, (o2 ^ 3) + o2p}};
    auto c2 = [](int r) { return ((8 * r) ^ ((r & 2) ? 8 : 0)) + 4 * (r >> 2); };
    // The transposes' reads, points n + 64 r (r = 0..7) at buf[idx + 72 r], as eight ds_read_b64 (2 LDS cycles
    // each, one 32-lane group on banks mod 64 -- what the layouts are built for).  Off one base register the
    // compiler merges pairs of them into ds_read2_b64 (8 cycles, 16-lane groups on banks mod 32), so r and
    // r + 4 share a base (288 float2 apart: past a ds_read2's offsets) and the four bases are made opaque
    auto read8 = [&](int idx, float2 (&dst)[8]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int ik = idx + 72 * k;
            asm volatile("" : "+v"(ik));
            dst[k] = buf[ik];
            dst[k + 4] = buf[ik + 288];
        }
    };
    // HOIST: the same four bases as opaque 32-bit LDS addresses (the x 8 included) made once, before the tile
    // loop.  A read is then the ds_read_b64 alone; the opaque index above costs a v_mov, an s_nop and a
    // v_lshl_add in front of every pair of reads in every iteration (32 VALU instructions and 16 nops per
    // wave-iteration, eight of those chains right behind the tile barrier).  Measured -2.1 to -2.3 % on the C3
    // launch (profiles/stft1024_barrier_window_ab.txt)
    typedef float vf2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const vf2 lds_cf2;
    struct Bases8 {
        lds_cf2 *p[4];
    };
    auto bases8 = [&](int idx) {
        Bases8 b;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lds_cf2 *p = (lds_cf2 *)buf + (idx + 72 * k);
            if constexpr (HOIST) asm volatile("" : "+v"(p));
            b.p[k] = p;
        }
        return b;
    };
    auto get8 = [&](const Bases8 &b, int idx, float2 (&dst)[8]) {
        if constexpr (HOIST) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const vf2 lo = b.p[k][0], hi = b.p[k][288];
                dst[k] = make_float2(lo.x, lo.y);
                dst[k + 4] = make_float2(hi.x, hi.y);
            }
        } else {
            read8(idx, dst);
        }
    };
    // the table entries as ds_read_b128 (two float2 each)
    auto tab4 = [&](int c) { return *reinterpret_cast<const float4 *>(tab + c); };
    // pass 3: this lane's frame of the tile and its half-wave's slot: butterflies jA (stream A) and jB
    // (stream B); slot 0 is (0, 32), every other slot j the conjugate pair (j, 64 - j)
    const int frm = l & 31, fpar = l & 1;
    const int sl = 2 * wave + (l >> 5);
    const int jB = sl ? 64 - sl : 32;
    const int fbase = (frm >> 1) * F_PAIRF + fpar * F_SCRF;
    const int i3a = fbase + (phys(sl) ^ fpar), i3b = fbase + (phys(jB) ^ fpar);
    const float2 *stA = s_all + sl * F_SLOTW;
    // output rows of this lane from the tile's base, as 32-bit byte offsets (WIDE = 0: K*ld*4 < 2^31) with
    // the multiples of 64 rows as scalar offsets: bin j + 64 r at offA + 64 r rows, its mirror
    // 512 - j - 64 r at offB + 64 (7 - r) rows
    const uint32_t ld4 = (uint32_t)ld * 4u;
    const uint32_t offA = (uint32_t)sl * ld4 + 4u * frm, offB = (uint32_t)(64 - sl) * ld4 + 4u * frm;
    __syncthreads();

    __shared__ int64_t slot[2];  // DYN: drawn chunk tickets
    int64_t tb, te;              // the current range of tiles
    int par = 0;
    if constexpr (DYN) {
        if (tid == 0) slot[0] = (int64_t)atomicAdd(ticket, 1ull);
        __syncthreads();
        const int64_t k = uniform_i64(slot[0]);
        if (k >= nchunks) return;
        tb = uniform_i64(sched[k]);
        te = uniform_i64(sched[k + 1]);
        if (tid == 0) slot[1] = (int64_t)atomicAdd(ticket, 1ull);  // the chunk after
        // published before any wave reads it: a one-tile first chunk (ntiles = 1, the schedule's only
        // chunk below cmin) reads slot[1] at its first loop head, with no tile barrier in between
        __syncthreads();
        par = 1;
    } else {
        tb = (int64_t)blockIdx.x * tiles_per_wg;
        te = tb + tiles_per_wg < ntiles ? tb + tiles_per_wg : ntiles;
        if (tb >= te) return;
    }
    auto file_at = [&](int64_t f, int64_t ti) {
        FileCur c;
        c.f = f;
        c.ti = ti;
        const int64_t n = len[f];
        c.nfr = n >= 1024 ? (n - 1024) / hop + 1 : 0;
        c.base = off[f];
        return c;
    };
    auto advance = [&](const FileCur &c) {
        return c.ti + 1 < tiles_per_file ? FileCur{c.f, c.ti + 1, c.nfr, c.base} : file_at(c.f + 1, 0);
    };
    FileCur cur = file_at(tb / tiles_per_file, tb % tiles_per_file);
    const int wcol = wave * 2;  // the two tile columns (frames) of this wave

    constexpr int RB = PairRegs<SH>::RB, NR = PairRegs<SH>::N;
    raw_t raw[NR];
    load_pair<T, SH>(x, cur, cur.ti * F_TT + wcol, hop, l, raw);
    bool b_ok = cur.ti * F_TT + wcol + 1 < cur.nfr;  // the pair's second frame exists (wave-uniform)
    const float hs = vgpr_f(0.70710678118654752440f);  // sqrt(1/2) of the DFT8s, in a VGPR
    int tpar = 0;  // tile parity: the half of rbuf in use
    const Bases8 bt0 = bases8(wave * F_PAIRF + rd[0]), bt1 = bases8(wave * F_PAIRF + F_SCRF + rd[1]);
    const Bases8 b3a = bases8(i3a), b3b = bases8(i3b);

    for (int64_t tl = tb;;) {
        // the next tile: the next of this range, else (DYN) the first of the next drawn chunk
        bool has_next = tl + 1 < te, jump = false;
        int64_t ntl = tl + 1, nte = te;
        if constexpr (DYN) {
            if (!has_next) {
                const int64_t k2 = uniform_i64(slot[par]);
                if (k2 < nchunks) {
                    has_next = jump = true;
                    ntl = uniform_i64(sched[k2]);
                    nte = uniform_i64(sched[k2 + 1]);
                }
            }
        }
        const FileCur nxt = !has_next ? cur : jump ? file_at(ntl / tiles_per_file, ntl % tiles_per_file) : advance(cur);
        const bool b_cur = b_ok;
        float2 v[2][8], wv[8];
        // ---- detrend (consumes raw); the window is applied inside pass 1
        float rb[2] = {0.f, 0.f};  // integer samples: the mean's fractional part, times 1024
        {
            float mean[2], xr[2] = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if constexpr (IO::kInt) {
                    int s = 0;
                    if constexpr (SH) {  // frame sums from the three half sums (h1 shared)
                        int h[3] = {0, 0, 0};
#pragma unroll
                        for (int r = 0; r < 12; ++r) h[r >> 2] = IO::sum2(raw[r], h[r >> 2]);
                        s = h[q] + h[q + 1];
                    } else {
#pragma unroll
                        for (int r = 0; r < 8; ++r) s = IO::sum2(raw[RB * q + r], s);
                    }
                    s = row_sum_i(s);
                    const int tot = __builtin_amdgcn_readlane(s, 0) + __builtin_amdgcn_readlane(s, 16) +
                                    __builtin_amdgcn_readlane(s, 32) + __builtin_amdgcn_readlane(s, 48);
                    // the mean tot / 1024 = a + b / 1024 exactly (a = floor, 0 <= b < 1024): x - a is
                    // an exact integer (|x - a| < 2^16), so the frame is detrended by one subtraction
                    // at any offset, and b / 1024 times the window's DFT comes off bins 0 and 1 after
                    // the FFT (post pass).  (float(tot) / 1024, rounds 1-5, was exact only while
                    // |tot| < 2^24; the two-part mean hi + lo measured +7.9 % on this loop.)
                    mean[q] = detrend ? (float)(tot >> 10) : 0.f;
                    rb[q] = detrend ? (float)(tot & 1023) : 0.f;
                } else {
                    // float samples: the frame's first sample (lane 0's first value) comes off before
                    // the float sums, so that they accumulate the variation and not a DC offset (a
                    // float sum of 1024 values near m is off by ~10 u |m|: a residual DC otherwise);
                    // the mean is xref + the mean of x - xref
                    auto rl = [](float a, int lane) {
                        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a), lane));
                    };
                    const float xref = detrend ? rl(IO::lo(raw[RB * q]), 0) : 0.f;
                    float s = 0.f;
#pragma unroll
                    for (int r = 0; r < 8; ++r) s += (IO::lo(raw[RB * q + r]) - xref) + (IO::hi(raw[RB * q + r]) - xref);
                    s = row_sum_f(s);
                    const float tot = (rl(s, 0) + rl(s, 16)) + (rl(s, 32) + rl(s, 48));
                    mean[q] = detrend ? tot * (1.0f / 1024.0f) : 0.f;
                    xr[q] = xref;
                }
            }
            // each sample register converted once (SH: the shared half serves both frames); float
            // samples relative to their frame's xref
            float2 fr[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                if constexpr (IO::kInt) fr[i] = make_float2(IO::lo(raw[i]), IO::hi(raw[i]));
                else fr[i] = make_float2(IO::lo(raw[i]) - xr[i / RB], IO::hi(raw[i]) - xr[i / RB]);
            }
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const float4 w4 = tab4(r);
                wv[r] = make_float2(w4.x, w4.y);
                wv[r + 1] = make_float2(w4.z, w4.w);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    v[q][r] = make_float2(fr[RB * q + r].x - mean[q], fr[RB * q + r].y - mean[q]);
            }
            if (SH && !b_cur) {  // no second frame: its tile column must be zero (the loads were not)
#pragma unroll
                for (int r = 0; r < 8; ++r) v[1][r] = make_float2(0.f, 0.f);
                rb[1] = 0.f;
            }
        }
        // ---- prefetch the next tile's frame pair into the (now free) sample registers
        if (has_next) {
            load_pair<T, SH>(x, nxt, nxt.ti * F_TT + wcol, hop, l, raw);
            b_ok = nxt.ti * F_TT + wcol + 1 < nxt.nfr;
        }

        if constexpr (IO::kInt) {  // the frames' remainders to wave 0, which owns bins 0 and 1
            if (l < 2) rbuf[tpar * F_TT + wcol + l] = l ? rb[1] : rb[0];
        }

        // ---- pass 1 (Ns = 1): out[8 l + r], each frame through its own region (the odd frame's points
        // at phys() ^ 1: the two float2 of a 16-B write swap)
        dft8_windowed(v[0], v[0], wv, hs);
        dft8_windowed(v[1], v[1], wv, hs);
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            const int n = ((r & 2) ? wr2 : wr0) + (r & 4);
            *reinterpret_cast<float4 *>(&fb0[n]) =
                make_float4(v[0][r].x, v[0][r].y, v[0][r + 1].x, v[0][r + 1].y);
            *reinterpret_cast<float4 *>(&fb1[n]) =
                make_float4(v[1][r + 1].x, v[1][r + 1].y, v[1][r].x, v[1][r].y);
        }
        wave_sync();
        get8(bt0, wave * F_PAIRF + rd[0], v[0]);
        get8(bt1, wave * F_PAIRF + F_SCRF + rd[1], v[1]);
        wave_sync();
        // ---- pass 2 (Ns = 8): out[64 (l>>3) + (l&7) + 8 r]
        {
            float2 w[8];  // pass-2 twiddles r = 1..7 at 8..14
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                float4 w4 = tab4(8 + r);
                w[r + 1] = make_float2(w4.x, w4.y);
                if (r < 6) w[r + 2] = make_float2(w4.z, w4.w);
                // the last entry's other half is padding: kept a 16-B read all the same (narrowed to a
                // ds_read_b64, whose 32-lane groups meet the 36-dword lane stride in a 2-way conflict)
                else asm volatile("" : "+v"(w4.z), "+v"(w4.w));
            }
#pragma unroll
            for (int r = 1; r < 8; ++r) {
                v[0][r] = cmul(v[0][r], w[r]);
                v[1][r] = cmul(v[1][r], w[r]);
            }
        }
        dft8(v[0], hs);
        dft8(v[1], hs);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            fb0[w2[0][(r >> 1) & 1] + c2(r)] = v[0][r];
            fb1[w2[1][(r >> 1) & 1] + c2(r)] = v[1][r];
        }
        lds_barrier();  // the tile's pass-2 output is complete
        // ---- pass 3 (Ns = 64) by bin: this lane's frame frm, butterflies j (A) and 64 - j (B) of its
        // half-wave's slot.  A holds Z[j + 64 r]; B's DFT8 input takes conj(A's twiddles) and its output
        // index shifts by one: Z[64 - j + 64 k] = Y[(k + 1) & 7].
        // ---- post: X' = 2X = (Z + conj Zm) + W^k (-i)(Z - conj Zm), Zm = Z[(512 - k) mod 512],
        // and from the same e, o the mirror bin X'[512 - k] = conj(e - W^k o).  The lane owns the
        // eight pairs (k = j + 64 r, 512 - k), r = 0..7: Zm is B's register 7 - r = Y[(8 - r) & 7], and
        // W^(k + 256) = -i W^k.  The window carries sqrt(scale / 2): |X'|^2 is the doubled one-sided density.
        // SP (wave 0): its lanes 0..31 hold slot 0, butterflies 0 (A) and 32 (B, its own twiddle row), each
        // its own conjugate partner: pairs r < 4 are (A[r], A[(8 - r) & 7]), bins 64 r and 512 - 64 r (r = 0:
        // DC and Nyquist, not doubled), pairs r >= 4 are (B[r - 4], B[11 - r]), bins 32 + 64 (r - 4) and
        // their mirrors, and bin 256 = 2 conj(Z[256]) is a 17th row.  Its lanes 32..63 hold slot 1;
        // bins 0 and 1 take the integer mean's remainder (dcw0, dcw1).
        char *of = reinterpret_cast<char *>(out + cur.f * (int64_t)F_K * ld + cur.ti * F_TT);
        // WIDE = 0: a buffer resource on the tile's base, the lane's 32-bit row offsets and scalar
        // multiples of 64 rows (no per-store 64-bit address arithmetic).  WIDE = 1: the lower of the two
        // half-waves' rows as a 64-bit scalar base and one row (ld * 4 < 2^32 B) in the lane offset; rows that
        // are not neighbours (slot 0's butterfly 32 beside slot 1) leave as one store per half-wave
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(of, 0, (int)((uint32_t)F_K * ld4), 0x00020000);
        typedef __attribute__((address_space(1))) float gfloat;
        // streaming (non-temporal) stores: written once, never re-read here.  row(h): the row of half-wave h
        auto put = [&](float p, uint32_t voff, auto row, int srow, bool split = false) {
            if constexpr (WIDE) {
                if (split) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if ((l >> 5) == h)
                            __builtin_nontemporal_store(
                                p, (gfloat *)(of + uniform_i64((int64_t)(row(h) + srow) * ld * 4)) + frm);
                } else {
                    const bool up = row(0) < row(1);  // rows of the two halves: neighbours
                    const uint32_t o = ((l >> 5) == (up ? 1 : 0) ? ld4 : 0u) + 4u * frm;
                    __builtin_nontemporal_store(
                        p, (gfloat *)(of + uniform_i64((int64_t)(row(up ? 0 : 1) + srow) * ld * 4) + o));
                }
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, p), rsrc, voff, srow * ld4, 2 /* nt */);
            }
        };
        auto pass3 = [&](auto spc) {
            constexpr bool SP = decltype(spc)::value;
            const bool s0 = SP && l < 32;  // this lane holds slot 0
            // slot 0's butterfly 32: its own constants row; its bins 32 + 64 (r - 4) and their mirrors
            // 288 + 64 (7 - r) as rows from 64 (r - 4) and 64 (7 - r)
            const float2 *stB = s0 ? s_all + 32 * F_SLOTW : stA;
            auto rowA = [&](int h) { return 2 * wave + h; };
            auto rowB = [&](int h) { return 64 - 2 * wave - h; };
            auto rowA_hi = [&](int h) { return SP && h == 0 ? 32 : 2 * wave + h + 256; };
            auto rowB_hi = [&](int h) { return SP && h == 0 ? 288 : 64 - 2 * wave - h; };
            const uint32_t offA_hi = offA + (s0 ? 32u : 256u) * ld4, offB_hi = offB + (s0 ? 224u * ld4 : 0u);
            float2 a[8], y[8];
            get8(b3a, i3a, a);
            get8(b3b, i3b, y);
            lds_barrier();  // every wave has read the tile's pass-2 output: the frame regions are free
            auto row4 = [](const float2 *p, int c) { return *reinterpret_cast<const float4 *>(p + c); };
            {
                float2 w[8], wb[8];  // pass-3 twiddles r = 1..7 at 0..6
#pragma unroll
                for (int r = 0; r < 8; r += 2) {
                    const float4 w4 = row4(stA, r);
                    w[r + 1] = make_float2(w4.x, w4.y);
                    if (r < 6) w[r + 2] = make_float2(w4.z, w4.w);
                    const float4 b4 = SP ? row4(stB, r) : w4;
                    wb[r + 1] = make_float2(b4.x, b4.y);
                    if (r < 6) wb[r + 2] = make_float2(b4.z, b4.w);
                }
#pragma unroll
                for (int r = 1; r < 8; ++r) {
                    a[r] = cmul(a[r], w[r]);
                    y[r] = cmulc(y[r], wb[r]);
                }
            }
            dft8(a, hs);
            dft8(y, hs);
            float2 wp[8];  // post twiddles at 8..11; SP: those of r >= 4 from B's row
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const float4 w4 = row4(stA, 8 + r);
                wp[r] = make_float2(w4.x, w4.y);
                wp[r + 1] = make_float2(w4.z, w4.w);
                const float4 b4 = SP ? row4(stB, 8 + r) : w4;
                wp[r + 4] = make_float2(b4.x, b4.y);
                wp[r + 5] = make_float2(b4.z, b4.w);
            }
            float rbv = 0.f;
            if constexpr (SP && IO::kInt) rbv = rbuf[tpar * F_TT + frm];
            const float2 dcw = s0 ? dcw0 : dcw1;
            const float sc0 = s0 ? 0.5f : 1.0f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                float2 z = a[r], m = y[(8 - r) & 7];
                if constexpr (SP) {
                    if (r < 4) {
                        if (s0) m = a[(8 - r) & 7];
                    } else if (s0) {
                        z = y[r - 3];
                        m = y[(12 - r) & 7];
                    }
                }
                const float2 e = make_float2(z.x + m.x, z.y - m.y);
                const float2 o = make_float2(z.y + m.y, m.x - z.x);  // -i (z - conj m)
                float2 t = cmul(wp[r], o);
                if (r >= 4) t = mul_mi(t);
                float2 X1 = cadd(e, t);
                const float2 X2 = csub(e, t);
                if constexpr (SP && IO::kInt) {
                    if (r == 0) {  // bins 0, 1: X' -= (b / 1024) 2 ws W_k, the mean's fractional part
                        X1.x = __builtin_fmaf(-rbv, dcw.x, X1.x);
                        X1.y = __builtin_fmaf(-rbv, dcw.y, X1.y);
                    }
                }
                float p1 = X1.x * X1.x + X1.y * X1.y, p2 = X2.x * X2.x + X2.y * X2.y;
                if (SP && r == 0) {
                    p1 *= sc0;
                    p2 *= sc0;
                }
                if (SP && r >= 4) {
                    put(p1, offA_hi, rowA_hi, 64 * (r - 4), true);
                    put(p2, offB_hi, rowB_hi, 64 * (7 - r), true);
                } else {
                    put(p1, offA, rowA, 64 * r);
                    put(p2, offB, rowB, 64 * (7 - r));
                }
            }
            if constexpr (SP) {
                if (s0) put((a[4].x * a[4].x + a[4].y * a[4].y) * 4.0f, offA, rowA, 256);  // bin 256
            }
        };
        if (wave == 0) pass3(std::true_type{});
        else pass3(std::false_type{});
        tpar ^= 1;
        cur = nxt;
        if (!has_next) break;
        if constexpr (DYN) {
            if (jump) {  // into the next chunk: draw the one after it
                par ^= 1;
                if (tid == 0) slot[par] = (int64_t)atomicAdd(ticket, 1ull);
            }
        }
        tl = ntl;
        te = nte;
    }
}

template <typename T>
int launch_fast_t(msd_stft_plan *p, const void *x, const int64_t *off, const int64_t *len, int64_t nfiles, float *out,
                  int64_t ld) {
    const bool wide = (uint64_t)F_K * (uint64_t)ld * 4u >= (1ull << 31);
    const bool sh = PairIO<T>::kInt && p->hop == 512;
    auto kern = wide ? (sh ? stft1024_kernel<T, 1, PairIO<T>::kInt> : stft1024_kernel<T, 1, false>)
                     : (sh ? stft1024_kernel<T, 0, PairIO<T>::kInt> : stft1024_kernel<T, 0, false>);
    if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(kern), F_LDS)) return rc;
    const int cus = p->ctx->num_cu;  // queried once in msd_create
    const int64_t tiles_per_file = ld / F_TT;
    const int64_t ntiles = tiles_per_file * nfiles;
    int64_t wgs = cus;  // one 16-wave workgroup per CU (LDS-bound residency)
    if (wgs > ntiles) wgs = ntiles;
    const float ws = static_cast<float>(std::sqrt(p->scale * 0.5));
    // the mean's fractional part b / 1024 on bins 0, 1: X' = 2 ws X, so the coefficient is 2 ws W_k / 1024
    const double cf = 2.0 * std::sqrt(p->scale * 0.5) / 1024.0;
    const float2 dcw0 = make_float2((float)(cf * p->win_dft01[0].x), (float)(cf * p->win_dft01[0].y));
    const float2 dcw1 = make_float2((float)(cf * p->win_dft01[1].x), (float)(cf * p->win_dft01[1].y));
    if (p->ctx->stft_sched == 2) {
        // guided schedule of tile chunks (>= 2 tiles), rebuilt when (ntiles, wgs) change
        auto dkern = wide ? (sh ? stft1024_kernel<T, 1, PairIO<T>::kInt, true> : stft1024_kernel<T, 1, false, true>)
                          : (sh ? stft1024_kernel<T, 0, PairIO<T>::kInt, true> : stft1024_kernel<T, 0, false, true>);
        if (int rc = ensure_dyn_lds(reinterpret_cast<const void *>(dkern), F_LDS)) return rc;
        // guided: each chunk 1 / (2 wgs) of what is left, at least 2 tiles, none below that at the end
        if (int rc = guided_sched_prepare(p->sched, p->ctx->stream, ntiles, wgs, 2, 2, 1, true)) return rc;
        hipLaunchKernelGGL(dkern, dim3((unsigned)wgs), dim3(F_NW * 64), F_LDS, p->ctx->stream, static_cast<const T *>(x),
                           off, len, tiles_per_file, ntiles, (int64_t)0, p->hop, ws, p->detrend, p->d_window.get(),
                           p->d_tw.get(), p->d_post.get(), out, ld, p->sched.bounds.get(), p->sched.n,
                           p->sched.ticket.get(), dcw0, dcw1);
        MSD_HIP(hipGetLastError());
        return MSD_OK;
    }
    const int64_t per = (ntiles + wgs - 1) / wgs;
    wgs = (ntiles + per - 1) / per;
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(F_NW * 64), F_LDS, p->ctx->stream, static_cast<const T *>(x),
                       off, len, tiles_per_file, ntiles, per, p->hop, ws, p->detrend, p->d_window.get(), p->d_tw.get(),
                       p->d_post.get(), out, ld, nullptr, (int64_t)0, nullptr, dcw0, dcw1);
    MSD_HIP(hipGetLastError());
    return MSD_OK;
}

}  // namespace

// returns 1 if the fast path handled the launch, 0 if not applicable, <0 on error
int launch_stft1024(msd_stft_plan *p, const void *x, int dtype, const int64_t *off, const int64_t *len,
                    int64_t nfiles, float *out, int64_t ld) {
    if (p->nperseg != 1024 || (p->hop & 1)) return 0;
    // integer samples need a window whose DFT vanishes past bin 1 (the mean's fractional part is
    // corrected on bins 0, 1 only); others take the generic kernel's exact two-part mean
    if ((dtype == MSD_I16 || dtype == MSD_U8) && p->detrend && !p->win_dft_compact) return 0;
    int rc;
    switch (dtype) {
        case MSD_I16: rc = launch_fast_t<int16_t>(p, x, off, len, nfiles, out, ld); break;
        case MSD_F32: rc = launch_fast_t<float>(p, x, off, len, nfiles, out, ld); break;
        case MSD_U8: rc = launch_fast_t<uint8_t>(p, x, off, len, nfiles, out, ld); break;
        default: return 0;
    }
    return rc == MSD_OK ? 1 : rc;
}

}  // namespace msd
