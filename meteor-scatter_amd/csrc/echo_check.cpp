// CPU check of echo_plan.h (the header echo.hip compiles), built with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer (make echo_check) and run by tests/test_echo_host.py.  No HIP.
// Prints one "ok <head>: ..." line per check; any other output or a non-zero exit is a failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "echo_plan.h"

using namespace msd::echo;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static msd_echo_cfg cfg(int64_t B, int nperseg, int hop, int k_lo, int k_hi, int n_lo = 0, int n_hi = -1, int pre = 0,
                        int post = 0) {
    return msd_echo_cfg{B, nperseg, hop, k_lo, k_hi, n_lo, n_hi, pre, post};
}

static int code(const msd_echo_cfg &c, int64_t K) {
    const char *msg = nullptr;
    const int rc = validate(&c, K, &msg);
    CHECK((rc == MSD_OK) == (msg == nullptr));
    return rc;
}

static void refusals() {
    CHECK(code(cfg(1200, 1024, 128, 169, 173, 118, 121, 4, 46), 513) == MSD_OK);
    CHECK(code(cfg(1, 1, 1, 0, 0), 1) == MSD_OK);
    CHECK(validate(nullptr, 8, nullptr) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 0, 0), 0) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 3, 2), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, -1, 2), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 2, 8), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 2, 3, -1, 1), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 2, 3, 5, 8), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 2, 3, 9, -5), 8) == MSD_OK);  // an empty noise band, wherever it lies
    CHECK(code(cfg(1200, 1024, 0, 2, 3), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 0, 128, 2, 3), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(0, 1024, 128, 2, 3), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 2, 3, 0, -1, -1, 0), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 2, 3, 0, -1, 0, -1), 8) == MSD_ERR_INVALID);
    CHECK(code(cfg(1200, 1024, 128, 0, MAX_BAND - 1), 1000) == MSD_OK);
    CHECK(code(cfg(1200, 1024, 128, 0, MAX_BAND), 1000) == MSD_ERR_UNSUPPORTED);
    CHECK(code(cfg(1200, 1024, 128, 0, 1, 10, 10 + MAX_BAND), 1000) == MSD_ERR_UNSUPPORTED);
    CHECK(MAX_BAND >= 64);
    std::printf("ok refusals: cfg, bands up to %d rows\n", MAX_BAND);
}

static void spans() {
    // c(s): frame t is centred at t hop + nperseg / 2
    CHECK(first_frame_at(0, 1024, 128) == 0 && first_frame_at(511, 1024, 128) == 0 && first_frame_at(512, 1024, 128) == 0);
    CHECK(first_frame_at(513, 1024, 128) == 1 && first_frame_at(640, 1024, 128) == 1 && first_frame_at(641, 1024, 128) == 2);
    CHECK(first_frame_at(-5, 1024, 128) == 0 && first_frame_at(3, 7, 1) == 0 && first_frame_at(4, 7, 1) == 1);
    for (int64_t s = 0; s < 4000; ++s)
        for (int hop : {1, 3, 128, 512}) {
            const int64_t t = first_frame_at(s, 1023, hop);
            CHECK(t >= 0 && t * hop + 511 >= s && (t == 0 || (t - 1) * hop + 511 < s));
        }
    // blocks of 100 samples, nperseg 8, hop 10: c(100 b) = ceil((100 b - 4) / 10) = 10 b
    const msd_echo_cfg c = cfg(100, 8, 10, 0, 0, 0, -1, 5, 30);
    const msd_det d[3] = {{2, 4, 0.0}, {4, 5, 0.0}, {9, 9, 0.0}};
    Span s = span_of(d, 0, 3, c, 200);
    CHECK(s.a0 == 20 && s.a1 == 40 && s.t0 == 15 && s.t1 == 40 && s.flags == 2);  // the neighbour touches: no post
    s = span_of(d, 1, 3, c, 200);
    CHECK(s.a0 == 40 && s.a1 == 50 && s.t0 == 40 && s.t1 == 80 && s.flags == 1);
    s = span_of(d, 2, 3, c, 200);
    CHECK(s.a0 == 90 && s.a1 == 90 && s.t0 == 85 && s.t1 == 120 && s.flags == 0);  // start == stop: padding only
    s = span_of(d, 2, 3, c, 100);
    CHECK(s.t0 == 85 && s.t1 == 100 && s.flags == 2);                               // clipped at T
    s = span_of(d, 0, 1, cfg(100, 8, 10, 0, 0, 0, -1, 50, 0), 200);
    CHECK(s.t0 == 0 && s.t1 == 40 && s.flags == 1);                                 // clipped at frame 0
    s = span_of(d, 1, 3, c, 0);
    CHECK(s.a0 == 0 && s.a1 == 0 && s.t0 == 0 && s.t1 == 0 && s.flags == 3);        // T = 0
    s = span_of(d, 0, 1, cfg(100, 8, 10, 0, 0), 30);
    CHECK(s.a0 == 20 && s.a1 == 30 && s.t0 == 20 && s.t1 == 30 && s.flags == 0);    // the core clipped at T, no padding
    std::printf("ok spans: c(s), neighbours, clipping, T = 0\n");
}

// 5 x 8 spectrograms, one detection over blocks [0, 8) of one sample, nperseg 1, hop 1: the span is all 8 frames
struct Grid {
    double v[5][8] = {};
    msd_echo run(int k_lo, int k_hi, int n_lo = 0, int n_hi = -1) const {
        const msd_det d{0, 8, 0.0};
        return measure_one(&v[0][0], 5, 8, 8, &d, 0, 1, cfg(1, 1, 1, k_lo, k_hi, n_lo, n_hi));
    }
};

static void records() {
    {  // a single hot cell
        Grid g;
        g.v[2][3] = 7.0, g.v[4][3] = 2.0;
        const msd_echo e = g.run(1, 3, 4, 4);
        CHECK(e.t0 == 0 && e.t1 == 8 && e.t_peak == 3 && e.k_peak == 2 && e.p_peak == 7.0 && e.n_peak == 2.0);
        CHECK(e.d_peak == 0.0 && e.t_half_first == 3 && e.t_half_last == 3 && e.t_efold == 4 && e.flags == 0);
        CHECK(e.e_sig == 7.0 && e.e_noise == 2.0 && e.w_r == 7.0 && e.w_u == 21.0 && e.w_uu == 63.0 && e.w_ur == 21.0);
    }
    {  // two frames tie: the lowest wins; the last frame still within 3 dB, no e-fold after it
        Grid g;
        g.v[2][2] = 5.0, g.v[2][6] = 5.0, g.v[2][7] = 4.0;
        const msd_echo e = g.run(2, 2);
        CHECK(e.t_peak == 2 && e.t_half_first == 2 && e.t_half_last == 7 && e.t_efold == 3 && e.flags == 0);
    }
    {  // two rows tie: the lowest wins
        Grid g;
        g.v[1][4] = 3.0, g.v[3][4] = 3.0;
        const msd_echo e = g.run(1, 3);
        CHECK(e.t_peak == 4 && e.k_peak == 1 && e.p_peak == 6.0 && e.w_r == 0.0);
    }
    {  // a peak in row 0 and one in row K - 1: no parabola
        Grid g;
        g.v[0][1] = 4.0, g.v[1][1] = 3.0;
        msd_echo e = g.run(0, 1);
        CHECK(e.k_peak == 0 && e.d_peak == 0.0 && e.p_peak == 7.0);
        Grid h;
        h.v[4][1] = 4.0, h.v[3][1] = 3.0;
        e = h.run(3, 4);
        CHECK(e.k_peak == 4 && e.d_peak == 0.0 && e.w_r == 7.0);
    }
    {  // a symmetric triple, and (a, b, c) = (1, 4, 3): delta = 0.5 (1 - 3) / ((1 - 8) + 3) = 0.25
        Grid g;
        g.v[1][5] = 2.0, g.v[2][5] = 4.0, g.v[3][5] = 2.0;
        msd_echo e = g.run(2, 2);
        CHECK(e.k_peak == 2 && e.d_peak == 0.0);
        g.v[1][5] = 1.0, g.v[3][5] = 3.0;
        e = g.run(2, 2);  // the neighbours lie outside the band
        CHECK(e.k_peak == 2 && e.d_peak == 0.25 && e.p_peak == 4.0 && e.w_r == 1.0);
        e = g.run(1, 3);
        CHECK(e.k_peak == 2 && e.d_peak == 0.25 && e.p_peak == 8.0 && e.w_r == 8.0 * 1.25);
    }
    {  // the peak in the last frame: bits 2 and 3; an empty span
        Grid g;
        g.v[2][7] = 1.0;
        msd_echo e = g.run(2, 2);
        CHECK(e.t_peak == 7 && e.t_efold == 8 && e.flags == (4 | 8));
        const msd_det d{9, 9, 0.0};
        e = measure_one(&g.v[0][0], 5, 8, 8, &d, 0, 1, cfg(1, 1, 1, 2, 2));
        CHECK(e.t0 == 8 && e.t1 == 8 && e.t_peak == 8 && e.t_efold == 8 && e.k_peak == -1 && e.flags == 0);
        CHECK(std::isnan(e.p_peak) && std::isnan(e.n_peak) && e.d_peak == 0.0 && e.e_sig == 0.0 && e.w_ur == 0.0);
    }
    {  // float32 cells, a padded row stride: columns at or past T are not read (ASan would see a read past the rows)
        std::vector<float> v(5 * 9 - 1, 1.0f);
        const msd_det d{0, 8, 0.0};
        const msd_echo e = measure_one(v.data(), 5, 8, 9, &d, 0, 1, cfg(1, 1, 1, 0, 4, 0, 4));
        CHECK(e.p_peak == 5.0 && e.e_sig == 40.0 && e.e_noise == 40.0 && e.t_peak == 0 && e.flags == (4 | 8));
    }
    std::printf("ok records: hot cell, ties, edge rows, parabola, empty span, strided float32\n");
}

int main() {
    refusals();
    spans();
    records();
    return 0;
}
