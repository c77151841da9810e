// CPU check of the resampler's host plan (resamp_plan.h, the header resamp.hip compiles):
//   * refusals: every limit of the contract, with its code;
//   * the output counts against 128-bit arithmetic at pos0 = 0, 2^40 + 3 and the position limit
//     (pos0 + n) up = 2^62, against a count by enumeration at small positions, and stream emission: pushes
//     of any lengths plus the flush emit every output of the batch row once, the flush at most
//     ceil(c / M) + 1 of them, and no output not yet emitted reaches behind the history;
//   * the branch / offset arithmetic of a tile (phi0, n0(m0), then phi0 + o M in 32 bits) against the
//     definition for every coprime (L, M) with L <= 8, M <= 9, and for the shipped ratios at far positions;
//   * the layouts: every staged sample and every tap has exactly one slot inside its region, the lane map
//     is a permutation of the tile's outputs, every read of the filter loop lands on a staged sample and a
//     real tap, and the tile fits the LDS budget;
//   * the kernel's summation order (groups of K FMAs down a branch, partial sums in group order) in float64
//     against a long-double sum: within chain u gain S_m, for REAL and both SSB forms.
// No HIP.  `make -C meteor-scatter_amd/csrc resamp_check` builds build/resamp_check_san with g++
// -fsanitize=address,undefined.   resamp_check [SEED]   prints one "ok ..." line per check, or "FAIL ...".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "resamp_plan.h"

namespace {

using namespace msd::resamp;
using msd::ddc::cdiv;
using msd::ddc::phase;

int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++failures;                  \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");           \
        }                                \
    } while (0)

msd_resamp_cfg cfg_of(int mode, int L, int M, int ntaps, int64_t p = 0, int64_t q = 1, int out = MSD_F64, double gain = 1.0) {
    msd_resamp_cfg c{};
    c.mode = mode, c.up = L, c.down = M, c.ntaps = ntaps, c.out_dtype = out, c.shift_num = p, c.shift_den = q, c.gain = gain;
    return c;
}

void check_refusals() {
    const char *msg = nullptr;
    auto rc = [&](msd_resamp_cfg c) { return validate(&c, &msg); };
    CHECK(validate(nullptr, &msg) == MSD_ERR_INVALID, "null cfg");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 3, 25)) == MSD_OK, "valid REAL");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 255, 1024, 4095, (1 << 24) - 1, 1 << 24)) == MSD_OK, "valid SSB at the limits");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 256, 1, 4095)) == MSD_OK, "pure interpolation");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 1, 12, 97)) == MSD_OK, "up = 1");
    CHECK(rc(cfg_of(2, 2, 3, 25)) == MSD_ERR_INVALID, "mode");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 0, 3, 25)) == MSD_ERR_UNSUPPORTED, "up = 0");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 257, 3, 25)) == MSD_ERR_UNSUPPORTED, "up = 257");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 0, 25)) == MSD_ERR_UNSUPPORTED, "down = 0");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 1025, 25)) == MSD_ERR_UNSUPPORTED, "down = 1025");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 3, 0)) == MSD_ERR_UNSUPPORTED, "ntaps = 0");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 3, 4097)) == MSD_ERR_UNSUPPORTED, "ntaps = 4097");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 3, 24)) == MSD_ERR_INVALID, "even ntaps");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 4, 6, 25)) == MSD_ERR_INVALID, "gcd 2");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 3, 3, 25)) == MSD_ERR_INVALID, "gcd 3");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 3, 25, 0, 1, MSD_F32)) == MSD_ERR_INVALID, "out dtype");
    CHECK(rc(cfg_of(MSD_DDC_REAL, 2, 3, 25, 1, 4)) == MSD_ERR_UNSUPPORTED, "REAL with a shift");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 2, 3, 25, 4, 4)) == MSD_ERR_INVALID, "p = q");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 2, 3, 25, 1, ((int64_t)1 << 24) + 1)) == MSD_ERR_UNSUPPORTED, "q = 2^24 + 1");
    CHECK(rc(cfg_of(MSD_DDC_SSB, 2, 3, 25, 1, 4, MSD_F64, NAN)) == MSD_ERR_INVALID, "gain NaN");
    Plan P;
    msd_resamp_cfg c = cfg_of(MSD_DDC_SSB, 2, 125, 1001, 30, 192);
    CHECK(make_plan(&c, P, &msg) == MSD_OK && P.p == 5 && P.q == 32 && !P.two && P.c == 500 && P.I == 501, "reduction 30/192 = 5/32");
    c = cfg_of(MSD_DDC_SSB, 2, 125, 1001, 7, 250000);
    CHECK(make_plan(&c, P, &msg) == MSD_OK && P.two && P.step == (256 * 7) % 250000, "two tables at q = 250000");
    std::printf("ok refusals\n");
}

void check_counts(unsigned seed) {
    std::mt19937_64 rng(seed);
    const char *msg = nullptr;
    const int ratios[][2] = {{1, 1}, {2, 3}, {3, 2}, {7, 5}, {40, 441}, {160, 441}, {2, 125}, {256, 1}, {255, 1024}, {1, 12}, {1, 1024}};
    for (auto &r : ratios) {
        const int L = r[0], M = r[1];
        for (int ntaps : {1, 25, 4095}) {
            msd_resamp_cfg c = cfg_of(MSD_DDC_REAL, L, M, ntaps);
            const int cc = (ntaps - 1) / 2, I = (ntaps + L - 1) / L;
            const int64_t lim = MAX_POS / L;
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)M - 1, (int64_t)M, (int64_t)M + 1, (int64_t)5 * M + 3, (int64_t)I, (int64_t)1000}) {
                for (int64_t pos0 : {(int64_t)0, (int64_t)1, (int64_t)M - 1, (int64_t)M, ((int64_t)1 << 40) + 3, lim - n}) {
                    if (pos0 < 0 || pos0 + n > lim) continue;
                    int64_t m0 = -1, cnt = -1;
                    CHECK(out_len(&c, pos0, n, &m0, &cnt, &msg) == MSD_OK, "out_len %d/%d pos0 %lld n %lld", L, M, (long long)pos0, (long long)n);
                    const __int128 a = (__int128)pos0 * L, b = (__int128)(pos0 + n) * L;
                    const int64_t lo = (int64_t)((a + M - 1) / M), hi = (int64_t)((b + M - 1) / M);
                    CHECK(m0 == lo && cnt == hi - lo, "count %d/%d pos0 %lld n %lld: %lld / %lld", L, M, (long long)pos0, (long long)n,
                          (long long)cnt, (long long)(hi - lo));
                    if (pos0 < 2000 && n <= 1000) {  // by enumeration
                        int64_t k = 0, first = -1;
                        for (int64_t m = 0; m * M < (pos0 + n) * L; ++m)
                            if (m * M >= pos0 * L) {
                                if (first < 0) first = m;
                                ++k;
                            }
                        CHECK(cnt == k && (k == 0 || first == m0), "enumeration %d/%d pos0 %lld n %lld", L, M, (long long)pos0, (long long)n);
                    }
                    // a stream reset to pos0 and pushed in random pieces, then flushed: every output once
                    int64_t count = pos0, emitted = 0, next = out_index(pos0, L, M), left = n;
                    bool okay = true;
                    while (true) {
                        const int64_t piece = left ? (int64_t)(rng() % (uint64_t)(left + 1)) : 0;
                        const int64_t lo2 = stream_emitted(pos0, count, L, M, cc), hi2 = stream_emitted(pos0, count + piece, L, M, cc);
                        okay = okay && lo2 == next && hi2 >= lo2 && hi2 - lo2 <= cdiv(piece * L, M) + 1;
                        // the oldest input of an output not yet emitted lies inside the new history
                        const int64_t oldest = (hi2 * M + cc) / L - (I - 1);
                        okay = okay && oldest >= count + piece - (I - 1);
                        emitted += hi2 - lo2, next = hi2, count += piece, left -= piece;
                        if (!left) break;
                    }
                    const int64_t lo2 = stream_emitted(pos0, count, L, M, cc), hi2 = out_index(count, L, M);
                    okay = okay && lo2 == next && hi2 >= lo2 && hi2 - lo2 <= cdiv(cc, M) + 1;
                    emitted += hi2 - lo2;
                    CHECK(okay && emitted == cnt, "stream emission %d/%d ntaps %d pos0 %lld n %lld", L, M, ntaps, (long long)pos0, (long long)n);
                }
            }
            CHECK(out_len(&c, lim, 1, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "one past the limit");
            CHECK(out_len(&c, lim + 1, 0, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "pos0 past the limit");
            CHECK(out_len(&c, 0, lim + 1, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "n past the limit");
            CHECK(out_len(&c, 0, lim, nullptr, nullptr, &msg) == MSD_OK, "n at the limit");
        }
    }
    msd_resamp_cfg c = cfg_of(MSD_DDC_REAL, 2, 3, 5);
    CHECK(out_len(&c, -1, 5, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "negative pos0");
    CHECK(out_len(&c, 5, -1, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "negative n");
    CHECK(out_len(&c, INT64_MAX - 5, 100, nullptr, nullptr, &msg) == MSD_ERR_INVALID, "overflow");
    std::printf("ok counts: 128-bit and enumerated counts, the position limit, streams emit each output once\n");
}

// the tile arithmetic of resamp_kernel for a tile starting at output m0: returns false on a mismatch with
// the definition
bool tile_matches(int L, int M, int ntaps, int TM, int64_t m0) {
    const int c = (ntaps - 1) / 2, I = (ntaps + L - 1) / L;
    const int64_t t0 = m0 * M + c, n00 = t0 / L;
    const int phi0 = (int)(t0 - n00 * L);
    const int64_t nb = n00 - (I - 1);
    for (int o = 0; o < TM; ++o) {
        int phi, dn;
        branch_of(L, M, phi0, o, phi, dn);
        const __int128 t = (__int128)(m0 + o) * M + c;
        if (phi != (int)(t % L) || nb + (I - 1) + dn != (int64_t)(t / L)) return false;
        const int Iphi = branch_len(ntaps, L, phi);
        int want = 0;
        for (int k = phi; k < ntaps; k += L) ++want;
        if (Iphi != want || Iphi > I) return false;
    }
    return true;
}

void check_branches() {
    int pairs = 0;
    for (int L = 1; L <= 8; ++L)
        for (int M = 1; M <= 9; ++M) {
            if (msd::ddc::gcd64(L, M) != 1) continue;
            ++pairs;
            for (int ntaps : {1, 3, 25, 97}) {
                // over L consecutive outputs the branches are a permutation
                std::vector<int> seen((size_t)L, 0);
                const int c = (ntaps - 1) / 2;
                for (int m = 0; m < L; ++m) ++seen[(size_t)((m * M + c) % L)];
                for (int v : seen) CHECK(v == 1, "branches of %d/%d are no permutation", L, M);
                for (int64_t m0 : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)256, (int64_t)257, ((int64_t)1 << 40) + 3})
                    CHECK(tile_matches(L, M, ntaps, 256, m0), "tile arithmetic %d/%d ntaps %d m0 %lld", L, M, ntaps, (long long)m0);
            }
        }
    const int far[][3] = {{2, 3, 25}, {3, 2, 25}, {40, 441, 3529}, {20, 147, 1177}, {2, 125, 1001}, {160, 441, 4095}, {256, 1, 4095}, {255, 1024, 4095}};
    for (auto &s : far) {
        const int64_t mmax = (MAX_POS / s[1]) - 256;  // m M <= 2^62
        for (int64_t m0 : {(int64_t)0, (int64_t)12345, mmax})
            CHECK(tile_matches(s[0], s[1], s[2], 256, m0), "tile arithmetic %d/%d at m0 %lld", s[0], s[1], (long long)m0);
    }
    std::printf("ok branches: %d coprime pairs with L <= 8, M <= 9, and the shipped ratios up to m M = 2^62\n", pairs);
}

void check_layout() {
    const int shapes[][3] = {{1, 1, 1}, {2, 3, 1}, {2, 3, 25}, {3, 2, 25}, {7, 5, 3}, {2, 125, 1001}, {40, 441, 3529}, {20, 147, 1177},
                             {160, 441, 4095}, {256, 1, 4095}, {255, 1024, 4095}, {1, 12, 97}, {1, 1024, 4095}, {256, 1023, 1}};
    for (auto &s : shapes) {
        const int L = s[0], M = s[1], ntaps = s[2];
        msd_resamp_cfg c = cfg_of(MSD_DDC_REAL, L, M, ntaps);
        Plan P;
        const char *msg = nullptr;
        CHECK(make_plan(&c, P, &msg) == MSD_OK, "plan %d/%d/%d", L, M, ntaps);
        CHECK(P.TM >= 1 && P.TM * P.G == THREADS && P.K * P.G >= P.I && P.K <= P.I, "groups %d/%d/%d", L, M, ntaps);
        CHECK(P.lds_bytes <= msd::ddc::LDS_MAX && P.lds_bytes == sizeof(double) * (2 * (size_t)P.plane + (size_t)P.tapn + THREADS),
              "lds %d/%d/%d", L, M, ntaps);
        CHECK(!(P.plane & 1) && P.plane >= P.smax && P.tapn == P.I * L && P.tapn >= ntaps && P.tapn < ntaps + L, "regions %d/%d/%d", L, M, ntaps);
        CHECK(P.B >= 1 && P.B <= P.TM && !(P.B & (P.B - 1)), "lane map B %d", P.B);
        // taps: slot i L + phi holds h[phi + i L]: each k < I L once
        std::vector<char> used((size_t)P.tapn, 0);
        for (int i = 0; i < P.I; ++i)
            for (int phi = 0; phi < L; ++phi) {
                const int sl = i * L + phi;
                CHECK(sl < P.tapn && !used[(size_t)sl] && sl == phi + i * L, "tap slot");
                used[(size_t)sl] = 1;
            }
        // the lane map: a permutation of the tile's outputs
        std::vector<char> lane((size_t)P.TM, 0);
        for (int t = 0; t < P.TM; ++t) {
            const int o = lane_output(t, P.TM, P.B);
            CHECK(o >= 0 && o < P.TM && !lane[(size_t)o], "lane map %d/%d/%d t %d", L, M, ntaps, t);
            if (o >= 0 && o < P.TM) lane[(size_t)o] = 1;
        }
        // every read of the filter loop, at every tile phase and tile fill: a staged sample, a real tap, each
        // (output, i) once over the groups
        for (int phi0 = 0; phi0 < L; phi0 += (L > 16 ? 7 : 1))
            for (int nout : {1, P.TM / 2 + 1, P.TM}) {
                if (nout > P.TM) continue;
                const int S = (phi0 + (nout - 1) * M) / L + P.I;
                CHECK(S <= P.smax, "staged %d of %d", S, P.smax);
                for (int o = 0; o < nout; ++o) {
                    int phi, dn;
                    branch_of(L, M, phi0, o, phi, dn);
                    const int Iphi = branch_len(ntaps, L, phi);
                    int covered = 0;
                    for (int g = 0; g < P.G; ++g) {
                        const int i0 = g * P.K, i1 = i0 + P.K < Iphi ? i0 + P.K : Iphi;
                        for (int i = i0; i < i1; ++i, ++covered) {
                            const int sl = (P.I - 1) + dn - i, tp = phi + i * L;
                            CHECK(sl >= 0 && sl < S && tp >= 0 && tp < ntaps, "read %d/%d/%d o %d i %d", L, M, ntaps, o, i);
                        }
                    }
                    CHECK(covered == Iphi, "coverage %d/%d/%d o %d", L, M, ntaps, o);
                }
            }
        int cs = 0, ct = 0, cs1 = 0, ct1 = 0;
        lane_map_cost(L, M, ntaps, P.TM, P.B, &cs, &ct);
        lane_map_cost(L, M, ntaps, P.TM, 1, &cs1, &ct1);
        CHECK(cs + ct <= cs1 + ct1, "lane map no worse than the identity");
        const int nph = L < 16 ? L : 16, reads = nph * (P.TM < 64 ? 1 : 2);
        std::printf("ok layout %d/%d/%d: TM %d, G %d, K %d, I %d, B %d, %zu bytes of LDS, chain %.0f, extra LDS cycles per "
                    "half-wave read: samples %.2f taps %.2f (identity map %.2f, %.2f)\n",
                    L, M, ntaps, P.TM, P.G, P.K, P.I, P.B, P.lds_bytes, chain(P), (double)cs / reads, (double)ct / reads,
                    (double)cs1 / reads, (double)ct1 / reads);
    }
}

// resamp_kernel's arithmetic for one output on the CPU
double kernel_output(const Plan &P, const std::vector<double> &h, const std::vector<double> &t1, const std::vector<double> &t2,
                     const std::vector<double> &xr, const std::vector<double> &xi, int64_t pos0, int64_t m) {
    const int64_t N = (int64_t)xr.size();
    const int64_t t = m * P.M + P.c, n0 = t / P.L;
    const int phi = (int)(t - n0 * P.L), Iphi = branch_len(P.ntaps, P.L, phi);
    double v = 0.0;
    for (int g = 0; g < P.G; ++g) {
        double acc = 0.0;
        for (int i = g * P.K; i < (g + 1) * P.K && i < Iphi; ++i) {
            const int64_t n = n0 - i;
            double zr = 0.0, zi = 0.0;
            if (n >= pos0 && n < pos0 + N) {
                const double a = xr[(size_t)(n - pos0)], b = xi[(size_t)(n - pos0)];
                if (P.mode == MSD_DDC_SSB) {
                    const int64_t r = phase(n, P.p, P.q);
                    double wx, wy;
                    if (P.two) {
                        const size_t rh = (size_t)(r >> msd::ddc::TABLE_BITS), rl = (size_t)(r & (msd::ddc::TABLE_MAX - 1));
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
            acc = std::fma(h[(size_t)(phi + i * P.L)], (P.mode == MSD_DDC_SSB && (m & 1)) ? zi : zr, acc);
        }
        v = g == 0 ? acc : v + acc;
    }
    double o = P.gain * v;
    if (P.mode == MSD_DDC_SSB && ((m & 3) == 1 || (m & 3) == 2)) o = -o;
    return o;
}

void check_order(unsigned seed) {
    const long double TWO_PI = 6.283185307179586476925286766559005768L;
    struct Case { int mode, L, M, ntaps; int64_t p, q, pos0; };
    const Case cases[] = {{MSD_DDC_REAL, 2, 3, 25, 0, 1, 0},
                          {MSD_DDC_REAL, 40, 441, 3529, 0, 1, 7},
                          {MSD_DDC_REAL, 256, 1, 4095, 0, 1, 3},
                          {MSD_DDC_REAL, 2, 3, 1, 0, 1, 0},
                          {MSD_DDC_SSB, 2, 125, 1001, 5, 32, 0},
                          {MSD_DDC_SSB, 3, 2, 25, 7, 250000, ((int64_t)1 << 40) + 3},
                          {MSD_DDC_SSB, 7, 5, 3, 1234567, (1 << 24) - 3, (MAX_POS / 7) - 400},
                          {MSD_DDC_SSB, 255, 1024, 4095, 1, 7, 1}};
    std::mt19937_64 rng(seed);
    for (const Case &cs : cases) {
        msd_resamp_cfg c = cfg_of(cs.mode, cs.L, cs.M, cs.ntaps, cs.p, cs.q, MSD_F64, 1.5);
        Plan P;
        const char *msg = nullptr;
        CHECK(make_plan(&c, P, &msg) == MSD_OK, "plan");
        CHECK(chain(P) <= 10.0 + P.I + (P.G - 1), "chain above its cap");
        std::vector<double> t1, t2, h((size_t)cs.ntaps);
        if (cs.mode == MSD_DDC_SSB) tables(P, t1, t2);
        for (auto &v : h) v = (double)((int64_t)(rng() % 2001) - 1000) / 1000.0;
        int64_t N = (int64_t)(cs.M * 6 / cs.L) + 2 * P.I + 5;
        if (N > 300) N = 300 + P.I;
        std::vector<double> xr((size_t)N), xi((size_t)N, 0.0);
        for (auto &v : xr) v = (double)((int64_t)(rng() % 65536) - 32768);
        if (cs.mode == MSD_DDC_SSB)
            for (auto &v : xi) v = (double)((int64_t)(rng() % 65536) - 32768);
        int64_t m0 = 0, cnt = 0;
        CHECK(out_len(&c, cs.pos0, N, &m0, &cnt, &msg) == MSD_OK, "out_len");
        double worst = 0.0;
        int64_t zeros = 0;
        for (int64_t m = m0; m < m0 + cnt; ++m) {
            const __int128 t = (__int128)m * cs.M + P.c;
            const int64_t n0 = (int64_t)(t / cs.L);
            const int phi = (int)(t % cs.L);
            long double vr = 0.0L, vi = 0.0L, S = 0.0L;
            for (int k = phi, i = 0; k < cs.ntaps; k += cs.L, ++i) {
                const int64_t n = n0 - i;
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
            if (phi >= cs.ntaps) {
                ++zeros;
                CHECK(got == 0.0, "a branch with no tap gives %g", got);
            }
            CHECK(e <= bound, "order %d/%d/%d m %lld: error %g over bound %g", cs.L, cs.M, cs.ntaps, (long long)m, e, bound);
        }
        std::printf("ok order mode %d %d/%d/%d q %lld: %lld outputs (%lld of empty branches), chain %.0f, worst error %.4f of the bound\n",
                    cs.mode, cs.L, cs.M, cs.ntaps, (long long)cs.q, (long long)cnt, (long long)zeros, chain(P), worst);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
    check_refusals();
    check_counts(seed);
    check_branches();
    check_layout();
    check_order(seed);
    return failures ? 1 : 0;
}
