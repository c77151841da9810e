// CPU check of the down-converter's host plan (ddc_plan.h, the header ddc.hip compiles):
//   * refusals: every limit of the contract, with its code;
//   * the reduced shift, and r(n) = (n p) mod q against 128-bit arithmetic at n = 2^62, q = 2^24 - 3, at
//     negative n and around zero;
//   * the phase tables against long double sines of the unreduced angle: within 2^-60 before rounding,
//     half an ulp after, exact quarter turns, and the two-table product against the single factor within
//     the chain's share (2 sqrt 2 + 2 sqrt 2) u;
//   * the polyphase layout: slot() is one-to-one into the plane for every staged sample, an output's
//     lanes read consecutive slots, and the tile fits the LDS budget;
//   * the output counts at every pos0 mod D against a count by enumeration, and stream emission: pushes
//     of any lengths plus the flush emit every output of the batch row once;
//   * the kernel's summation order (groups of K4 FMAs, partial sums in group order) in float64 against a
//     long-double sum: within chain u gain S_m, for REAL and both SSB forms.
// No HIP.  `make -C meteor-scatter_amd/csrc ddc_check` builds build/ddc_check_san with g++
// -fsanitize=address,undefined.   ddc_check [SEED]   prints one "ok ..." line per check, or "FAIL ...".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ddc_plan.h"

namespace {

using namespace msd::ddc;

int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++failures;                  \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");           \
        }                                \
    } while (0)

msd_ddc_cfg cfg_of(int mode, int D, int ntaps, int64_t p, int64_t q, int out = MSD_F64, double gain = 1.0) {
    msd_ddc_cfg c{};
    c.mode = mode, c.decim = D, c.ntaps = ntaps, c.out_dtype = out, c.shift_num = p, c.shift_den = q, c.gain = gain;
    return c;
}

void check_refusals() {
    const char *msg = nullptr;
    auto rc = [&](msd_ddc_cfg c) { return validate(&c, &msg); };
    CHECK(validate(nullptr, &msg) == MSD_ERR_INVALID, "null cfg");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 97, 0, 1)) == MSD_OK, "valid REAL");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 1024, 4095, (1 << 24) - 1, 1 << 24)) == MSD_OK, "valid SSB at the limits");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 48, 385, 10, 64)) == MSD_OK, "reducible shift");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 48, 385, 2, (int64_t)1 << 25)) == MSD_OK, "q = 2^24 after reduction");
    CHECK(rc(cfg_of(2, 12, 97, 0, 1)) == MSD_ERR_INVALID, "mode");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 0, 97, 0, 1)) == MSD_ERR_UNSUPPORTED, "D = 0");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 1025, 97, 0, 1)) == MSD_ERR_UNSUPPORTED, "D = 1025");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 0, 0, 1)) == MSD_ERR_UNSUPPORTED, "ntaps = 0");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 4097, 0, 1)) == MSD_ERR_UNSUPPORTED, "ntaps = 4097");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 96, 0, 1)) == MSD_ERR_INVALID, "even ntaps");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 97, 0, 1, MSD_F32)) == MSD_ERR_INVALID, "out dtype");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 97, 1, 4)) == MSD_ERR_UNSUPPORTED, "REAL with a shift");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 12, 97, 0, 4)) == MSD_OK, "REAL with 0 / 4");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 12, 97, 4, 4)) == MSD_ERR_INVALID, "p = q");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 12, 97, -1, 4)) == MSD_ERR_INVALID, "p < 0");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 12, 97, 0, 0)) == MSD_ERR_INVALID, "q = 0");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 12, 97, 1, ((int64_t)1 << 24) + 1)) == MSD_ERR_UNSUPPORTED, "q = 2^24 + 1");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 12, 97, 1, 4, MSD_F64, NAN)) == MSD_ERR_INVALID, "gain NaN");
    CHECK(dtype_fits(MSD_DDC_REAL, MSD_I16) && dtype_fits(MSD_DDC_REAL, MSD_F32) && !dtype_fits(MSD_DDC_REAL, MSD_CI16) &&
              !dtype_fits(MSD_DDC_REAL, MSD_F64),
          "REAL dtypes");
    CHECK(dtype_fits(MSD_DDC_SSB, MSD_CI16) && dtype_fits(MSD_DDC_SSB, MSD_CF32) && !dtype_fits(MSD_DDC_SSB, MSD_I16),
          "SSB dtypes");
    Plan P;
    msd_ddc_cfg c = cfg_of(MSD_DDC_SSB, 48, 385, 30, 192);
    CHECK(make_plan(&c, P, &msg) == MSD_OK && P.p == 5 && P.q == 32 && !P.two && P.c == 192, "reduction 30/192 = 5/32");
    c = cfg_of(MSD_DDC_SSB, 48, 385, 7, 192000);
    CHECK(make_plan(&c, P, &msg) == MSD_OK && P.two && P.step == (256 * 7) % 192000, "two tables at q = 192000");
    std::printf("ok refusals\n");
}

void check_phase() {
    const int64_t q = (1 << 24) - 3;
    for (int64_t p : {(int64_t)1, (int64_t)1234567, q - 1})
        for (int64_t n : {(int64_t)0, (int64_t)1, q - 1, q, q + 1, (int64_t)1 << 40, ((int64_t)1 << 40) + 3, (int64_t)1 << 62,
                          ((int64_t)1 << 62) + 12345, INT64_MAX}) {
            const __int128 want = ((__int128)n * p) % q;
            CHECK(phase(n, p, q) == (int64_t)want, "r(%lld) p %lld", (long long)n, (long long)p);
        }
    // negative n (a tile's first staged sample lies before sample 0): the mathematical residue
    for (int64_t n : {(int64_t)-1, (int64_t)-4094, -q, -q - 1}) {
        __int128 want = ((__int128)n * 1234567) % q;
        if (want < 0) want += q;
        CHECK(phase(n, 1234567, q) == (int64_t)want, "r(%lld)", (long long)n);
    }
    // a thread's incremental phase: r(n + 256) = r(n) + step mod q
    const int64_t p = 1234567, step = (256 * p) % q;
    for (int64_t n : {(int64_t)0, ((int64_t)1 << 62) - 100}) {
        int64_t r = phase(n, p, q);
        for (int t = 1; t < 50; ++t) {
            r += step;
            if (r >= q) r -= q;
            CHECK(r == phase(n + 256 * t, p, q), "incremental phase");
        }
    }
    std::printf("ok phase: r(n) exact at n = 2^62, q = 2^24 - 3\n");
}

void check_tables() {
    const long double TWO_PI = 6.283185307179586476925286766559005768L;
    double worst = 0.0, worst2 = 0.0;
    for (int64_t q : {(int64_t)1, (int64_t)4, (int64_t)7, (int64_t)32, (int64_t)4096, (int64_t)192000, ((int64_t)1 << 24) - 3}) {
        msd_ddc_cfg c = cfg_of(MSD_DDC_SSB, 48, 385, q > 1 ? 1 : 0, q);
        Plan P;
        const char *msg = nullptr;
        CHECK(make_plan(&c, P, &msg) == MSD_OK, "plan q %lld", (long long)q);
        std::vector<double> t1, t2;
        tables(P, t1, t2);
        CHECK(t1.size() == 2 * (size_t)(P.two ? TABLE_MAX : q), "t1 size");
        CHECK(P.two == (q > TABLE_MAX), "two");
        for (size_t r = 0; r < t1.size() / 2; ++r) {
            const long double a = TWO_PI * (long double)r / (long double)q;
            const long double cr = cosl(a), ci = -sinl(a);
            // (cosl of the unreduced angle is itself within ~2^-62 here: r / q < 1)
            const double e = (double)std::fmax(fabsl((long double)t1[2 * r] - cr), fabsl((long double)t1[2 * r + 1] - ci));
            worst = std::fmax(worst, e / 0x1p-53);
            CHECK(e <= 0x1p-53 * 0.5001, "t1[%zu] of q %lld off by %g u", r, (long long)q, e / 0x1p-53);
        }
        if (q % 4 == 0) {  // quarter turns are exact
            const size_t k = (size_t)(q / 4);
            if (!P.two) CHECK(t1[2 * k] == 0.0 && t1[2 * k + 1] == -1.0 && t1[4 * k] == -1.0 && t1[4 * k + 1] == 0.0, "quarter turns of q %lld", (long long)q);
        }
        CHECK(t1[0] == 1.0 && t1[1] == 0.0 && !std::signbit(t1[1]), "entry 0");
        if (!P.two) continue;
        CHECK(t2.size() == 2 * (size_t)((q + TABLE_MAX - 1) / TABLE_MAX), "t2 size");
        // the product of the two entries, as the kernel forms it, against the single factor
        std::mt19937_64 rng(q);
        for (int it = 0; it < 20000; ++it) {
            const int64_t r = it < 4 ? (it & 1 ? q - 1 - it : it) : (int64_t)(rng() % (uint64_t)q);
            const size_t rh = (size_t)(r >> TABLE_BITS), rl = (size_t)(r & (TABLE_MAX - 1));
            CHECK(2 * rh + 1 < t2.size(), "rh in range");
            const double ax = t2[2 * rh], ay = t2[2 * rh + 1], bx = t1[2 * rl], by = t1[2 * rl + 1];
            const double wx = std::fma(ax, bx, -(ay * by)), wy = std::fma(ax, by, ay * bx);
            const long double a = TWO_PI * (long double)r / (long double)q;
            const double e = (double)hypotl((long double)wx - cosl(a), (long double)wy + sinl(a));
            worst2 = std::fmax(worst2, e / 0x1p-53);
            CHECK(e <= 0x1p-53 * (4.0 * std::sqrt(2.0)), "two-table factor of r %lld, q %lld off by %g u", (long long)r, (long long)q, e / 0x1p-53);
        }
    }
    std::printf("ok tables: worst entry %.3f u, worst two-table product %.3f u of 5.66\n", worst, worst2);
}

void check_layout() {
    const int shapes[][2] = {{1, 1}, {2, 3}, {12, 5}, {12, 97}, {48, 385}, {1024, 4095}, {3, 4095}, {1024, 1}, {7, 4095}, {1000, 3}};
    for (auto &s : shapes) {
        const int D = s[0], ntaps = s[1];
        msd_ddc_cfg c = cfg_of(MSD_DDC_REAL, D, ntaps, 0, 1);
        Plan P;
        const char *msg = nullptr;
        CHECK(make_plan(&c, P, &msg) == MSD_OK, "plan %d/%d", D, ntaps);
        CHECK(P.TM >= 1 && P.TM * P.G == THREADS && P.K4 * P.G >= ntaps && (P.K4 - 1) * P.G < ntaps + P.G, "groups %d/%d", D, ntaps);
        CHECK(P.lds_bytes <= LDS_MAX && P.lds_bytes == sizeof(double) * (2 * (size_t)P.plane + THREADS), "lds %d/%d", D, ntaps);
        CHECK((P.U & 1) && !(P.plane & 1) && P.plane >= D * P.U, "U odd, plane even");
        const int S = P.TM * D + ntaps - 1;
        std::vector<char> used((size_t)P.plane, 0);
        for (int j = 0; j < S; ++j) {
            const int sl = slot(j, D, P.U);
            CHECK(sl >= 0 && sl < P.plane && !used[(size_t)sl], "slot %d of %d/%d", j, D, ntaps);
            if (sl >= 0 && sl < P.plane) used[(size_t)sl] = 1;
        }
        // the staging loop's incremental slot and the filter's incremental address, as ddc_kernel forms them
        for (int tid : {0, 1, THREADS - 1}) {
            int jr = tid % D, ju = tid / D;
            const int dr = THREADS % D, du = THREADS / D;
            for (int j = tid; j < S; j += THREADS) {
                CHECK(jr * P.U + ju == slot(j, D, P.U), "incremental slot");
                jr += dr, ju += du;
                if (jr >= D) jr -= D, ++ju;
            }
        }
        for (int g = 0; g < P.G; ++g) {
            const int k0 = g * P.K4, k1 = k0 + P.K4 < ntaps ? k0 + P.K4 : ntaps;
            if (k0 >= k1) continue;
            for (int i : {0, P.TM - 1}) {
                const int a = ntaps - 1 - k0;
                int ar = a % D, addr = ar * P.U + a / D + i;
                for (int k = k0; k < k1; ++k) {
                    CHECK(addr == slot(i * D + ntaps - 1 - k, D, P.U), "filter address %d/%d g %d k %d", D, ntaps, g, k);
                    if (ar == 0) ar = D - 1, addr += (D - 1) * P.U - 1;
                    else --ar, addr -= P.U;
                }
            }
        }
        std::printf("ok layout %d/%d: TM %d, G %d, K4 %d, U %d, %zu bytes of LDS, chain %.0f\n", D, ntaps, P.TM, P.G, P.K4, P.U,
                    P.lds_bytes, chain(P));
    }
}

void check_counts(unsigned seed) {
    std::mt19937_64 rng(seed);
    const char *msg = nullptr;
    for (int D : {1, 2, 3, 12, 48, 1024}) {
        for (int ntaps : {1, 5, 97}) {
            msd_ddc_cfg c = cfg_of(MSD_DDC_REAL, D, ntaps, 0, 1);
            const int cc = (ntaps - 1) / 2;
            for (int64_t base : {(int64_t)0, ((int64_t)1 << 40), ((int64_t)1 << 62)}) {
                for (int ph = 0; ph < D; ph += (D > 64 ? 37 : 1)) {
                    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)cc, (int64_t)cc + 1, (int64_t)D - 1, (int64_t)D, (int64_t)D + 1, (int64_t)5 * D + 3}) {
                        const int64_t pos0 = base + ph;
                        int64_t m0 = -1, cnt = -1;
                        CHECK(out_len(&c, pos0, n, &m0, &cnt, &msg) == MSD_OK, "out_len");
                        // by enumeration from the multiple of D at or below pos0
                        int64_t first = -1, k = 0;
                        for (int64_t m = pos0 / D; m * D < pos0 + n; ++m)
                            if (m * D >= pos0) {
                                if (first < 0) first = m;
                                ++k;
                            }
                        CHECK(cnt == k && (k == 0 || m0 == first), "count D %d pos0 %lld n %lld: %lld / %lld", D, (long long)pos0, (long long)n,
                              (long long)cnt, (long long)k);
                        // a stream reset to pos0 and pushed in random pieces, then flushed: every output once
                        int64_t count = pos0, emitted = 0, next = cdiv(pos0, D);
                        const int64_t start_m = next;
                        int64_t left = n;
                        bool okay = true;
                        while (true) {
                            const int64_t piece = left ? (int64_t)(rng() % (uint64_t)(left + 1)) : 0;
                            int64_t lo = cdiv(count - cc, D);
                            if (lo < start_m) lo = start_m;
                            int64_t hi = cdiv(count + piece - cc, D);
                            if (hi < lo) hi = lo;
                            okay = okay && lo == next;
                            emitted += hi - lo, next = hi, count += piece, left -= piece;
                            if (!left) break;
                        }
                        int64_t lo = cdiv(count - cc, D);
                        if (lo < start_m) lo = start_m;
                        int64_t hi = cdiv(count, D);
                        if (hi < lo) hi = lo;
                        okay = okay && lo == next;
                        emitted += hi - lo;
                        CHECK(okay && emitted == cnt, "stream emission D %d ntaps %d pos0 %lld n %lld", D, ntaps, (long long)pos0, (long long)n);
                    }
                }
            }
        }
    }
    msd_ddc_cfg c = cfg_of(MSD_DDC_REAL, 12, 5, 0, 1);
    CHECK(out_len(&c, -1, 5, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "negative pos0");
    CHECK(out_len(&c, 5, -1, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "negative n");
    CHECK(out_len(&c, INT64_MAX - 5, 100, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "overflow");
    std::printf("ok counts: every pos0 mod D, streams emit each output once\n");
}

// ddc_kernel's arithmetic for one output on the CPU: mix, groups of K4 FMAs in ascending k, partial sums in
// group order, gain, the output mixer
double kernel_output(const Plan &P, const std::vector<double> &h, const std::vector<double> &t1, const std::vector<double> &t2,
                     const std::vector<double> &xr, const std::vector<double> &xi, int64_t pos0, int64_t m) {
    const int64_t N = (int64_t)xr.size();
    std::vector<double> part((size_t)P.G, 0.0);
    for (int g = 0; g < P.G; ++g) {
        double acc = 0.0;
        for (int k = g * P.K4; k < (g + 1) * P.K4 && k < P.ntaps; ++k) {
            const int64_t n = m * P.D + P.c - k;
            double zr = 0.0, zi = 0.0;
            if (n >= pos0 && n < pos0 + N) {
                const double a = xr[(size_t)(n - pos0)], b = xi[(size_t)(n - pos0)];
                if (P.mode == MSD_DDC_SSB) {
                    const int64_t r = phase(n, P.p, P.q);
                    double wx, wy;
                    if (P.two) {
                        const size_t rh = (size_t)(r >> TABLE_BITS), rl = (size_t)(r & (TABLE_MAX - 1));
                        const double ax = t2[2 * rh], ay = t2[2 * rh + 1], bx = t1[2 * rl], by = t1[2 * rl + 1];
                        wx = std::fma(ax, bx, -(ay * by)), wy = std::fma(ax, by, ay * bx);
                    } else {
                        wx = t1[2 * (size_t)r], wy = t1[2 * (size_t)r + 1];
                    }
                    zr = std::fma(a, wx, -(b * wy)), zi = std::fma(a, wy, b * wx);
                } else {
                    zr = a;
                }
            }
            acc = std::fma(h[(size_t)k], (P.mode == MSD_DDC_SSB && (m & 1)) ? zi : zr, acc);
        }
        part[(size_t)g] = acc;
    }
    double v = part[0];
    for (int g = 1; g < P.G; ++g) v = v + part[(size_t)g];
    double o = P.gain * v;
    if (P.mode == MSD_DDC_SSB && ((m & 3) == 1 || (m & 3) == 2)) o = -o;
    return o;
}

void check_order(unsigned seed) {
    const long double TWO_PI = 6.283185307179586476925286766559005768L;
    struct Case { int mode, D, ntaps; int64_t p, q, pos0; };
    const Case cases[] = {{MSD_DDC_REAL, 12, 97, 0, 1, 0}, {MSD_DDC_REAL, 1024, 4095, 0, 1, 7}, {MSD_DDC_SSB, 48, 385, 5, 32, 0},
                          {MSD_DDC_SSB, 48, 385, 7, 192000, ((int64_t)1 << 40) + 3}, {MSD_DDC_SSB, 2, 3, 1234567, (1 << 24) - 3, (int64_t)1 << 62},
                          {MSD_DDC_SSB, 3, 4095, 1, 7, 1}};
    std::mt19937_64 rng(seed);
    for (const Case &cs : cases) {
        msd_ddc_cfg c = cfg_of(cs.mode, cs.D, cs.ntaps, cs.p, cs.q, MSD_F64, 1.5);
        Plan P;
        const char *msg = nullptr;
        CHECK(make_plan(&c, P, &msg) == MSD_OK, "plan");
        std::vector<double> t1, t2, h((size_t)cs.ntaps);
        if (cs.mode == MSD_DDC_SSB) tables(P, t1, t2);
        for (auto &v : h) v = (double)((int64_t)(rng() % 2001) - 1000) / 1000.0;
        const int64_t N = (int64_t)cs.D * 6 + cs.ntaps;
        std::vector<double> xr((size_t)N), xi((size_t)N, 0.0);
        for (auto &v : xr) v = (double)((int64_t)(rng() % 65536) - 32768);
        if (cs.mode == MSD_DDC_SSB)
            for (auto &v : xi) v = (double)((int64_t)(rng() % 65536) - 32768);
        int64_t m0 = 0, cnt = 0;
        CHECK(out_len(&c, cs.pos0, N, &m0, &cnt, &msg) == MSD_OK, "out_len");
        double worst = 0.0;
        for (int64_t m = m0; m < m0 + cnt; ++m) {
            long double vr = 0.0L, vi = 0.0L, S = 0.0L;
            for (int k = 0; k < cs.ntaps; ++k) {
                const int64_t n = m * cs.D + P.c - k;
                if (n < cs.pos0 || n >= cs.pos0 + N) continue;
                const long double a = xr[(size_t)(n - cs.pos0)], b = xi[(size_t)(n - cs.pos0)];
                long double zr = a, zi = 0.0L;
                if (cs.mode == MSD_DDC_SSB) {
                    const long double th = TWO_PI * (long double)phase(n, P.p, P.q) / (long double)P.q;
                    zr = a * cosl(th) + b * sinl(th), zi = b * cosl(th) - a * sinl(th);
                }
                vr += (long double)h[(size_t)k] * zr, vi += (long double)h[(size_t)k] * zi;
                S += fabsl((long double)h[(size_t)k]) * hypotl(a, b);
            }
            long double want = vr;
            if (cs.mode == MSD_DDC_SSB) want = (m & 3) == 0 ? vr : ((m & 3) == 1 ? -vi : ((m & 3) == 2 ? -vr : vi));
            want *= (long double)P.gain;
            const double got = kernel_output(P, h, t1, t2, xr, xi, cs.pos0, m);
            const double bound = chain(P) * 0x1p-53 * P.gain * (double)S;
            const double e = (double)fabsl((long double)got - want);
            if (bound > 0) worst = std::fmax(worst, e / bound);
            CHECK(e <= bound, "order %d/%d m %lld: error %g over bound %g", cs.D, cs.ntaps, (long long)m, e, bound);
        }
        std::printf("ok order mode %d %d/%d q %lld: chain %.0f, worst error %.4f of the bound\n", cs.mode, cs.D, cs.ntaps, (long long)cs.q,
                    chain(P), worst);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
    check_refusals();
    check_phase();
    check_tables();
    check_layout();
    check_counts(seed);
    check_order(seed);
    return failures ? 1 : 0;
}
