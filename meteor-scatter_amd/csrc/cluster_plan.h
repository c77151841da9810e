// Host-side plan of the time-frequency burst clustering (cluster.hip): parameter validation, the LDS layout
// of the two kernels, and a plain C++ restatement of what they compute.  No HIP: cluster.hip compiles it, and
// so does cluster_check.cpp with g++ under the sanitizers.
//
// DBSCAN (include/msdsp.h; sklearn.cluster.DBSCAN(eps, min_samples).fit(p).labels_ as called at
// meteor_detect_class/detector_and_classification.py:20), for points p[0 .. n) in float64 (x, y):
//   A[i][j] = (dx dx + dy dy) <= eps eps, dx = x_i - x_j, dy = y_i - y_j, i == j included, float64, that order,
//             no contraction;
//   core[i] = popcount(A[i]) >= min_samples (the point counts itself);
//   components = the connected components of the core points under A; cluster ids 0, 1, ... by each
//   component's lowest-index core point; a non-core point with a core neighbour takes the lowest id among its
//   core neighbours, else -1;
//   box = (x_min, y_min, x_max, y_max) over all members, border points included (:44-46);
//   critical = (x_max - x_min) >= critical_min_extent (:48-50).
//
// Point extraction (in ORB's place, :12-16): over the window k_lo <= k <= k_hi, t < frames of a float64
// spectrogram [K][ld], candidates are the cells with P > thr (NaN never, +inf always); cell index
// c = t nk + (k - k_lo), nk = k_hi - k_lo + 1; more than max_points candidates: the max_points largest by
// (P descending, c ascending); emitted in ascending c as x = (double)t sx, y = (double)(k - k_lo) sy.
//
// LDS layout of cluster_kernel, in this order: x[512], y[512] (float64), the adjacency bitmask, row i at
// 64-bit words [i ROW_WORDS, i ROW_WORDS + 8) with ROW_WORDS = 9 (the odd stride spreads a wave's rows over
// the banks), label[512], id[512] (int32), and the core / root masks (8 words each).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/msdsp.h"

namespace msd {
namespace cluster {

constexpr int MAX_POINTS = MSD_CLUSTER_MAX_POINTS;
constexpr int THREADS = 256;
constexpr int WORDS = MAX_POINTS / 64;  // 64-bit words of one adjacency row
constexpr int ROW_WORDS = WORDS + 1;    // padded row stride
constexpr size_t LDS_XY = 2 * sizeof(double) * MAX_POINTS;
constexpr size_t LDS_ADJ = sizeof(uint64_t) * MAX_POINTS * ROW_WORDS;
constexpr size_t LDS_LABELS = 2 * sizeof(int32_t) * MAX_POINTS;
constexpr size_t LDS_MASKS = 2 * sizeof(uint64_t) * WORDS;
constexpr size_t LDS_CLUSTER = LDS_XY + LDS_ADJ + LDS_LABELS + LDS_MASKS + 64;  // + flags and counters
constexpr int PEAK_DIGIT_BITS = 8;  // the radix select's digit
constexpr int PEAK_BINS = 1 << PEAK_DIGIT_BITS;
constexpr size_t LDS_PEAKS = sizeof(int32_t) * PEAK_BINS + 128;

inline int bad(const char **msg, int code, const char *m) {
    if (msg) *msg = m;
    return code;
}

// MSD_OK, or the code with *msg set
inline int validate(const msd_cluster_cfg *c, const char **msg) {
    if (!c) return bad(msg, MSD_ERR_INVALID, "null configuration");
    if (!std::isfinite(c->eps) || c->eps < 0) return bad(msg, MSD_ERR_INVALID, "eps must be finite and >= 0");
    if (c->min_samples < 1) return bad(msg, MSD_ERR_INVALID, "min_samples must be >= 1");
    if (std::isnan(c->critical_min_extent)) return bad(msg, MSD_ERR_INVALID, "critical_min_extent is NaN");
    if (c->max_points < 1 || c->max_points > MAX_POINTS)
        return bad(msg, MSD_ERR_UNSUPPORTED, "max_points outside 1 .. 512");
    return MSD_OK;
}

inline int validate_peaks(int64_t K, int64_t frames, int64_t ld, int64_t k_lo, int64_t k_hi, double sx, double sy,
                          int64_t max_points, const char **msg) {
    if (K < 1 || frames < 0 || ld < frames) return bad(msg, MSD_ERR_INVALID, "need K >= 1 and 0 <= frames <= ld");
    if (k_lo < 0 || k_lo > k_hi) return bad(msg, MSD_ERR_INVALID, "need 0 <= k_lo <= k_hi");
    if (k_hi >= K) return bad(msg, MSD_ERR_INVALID, "k_hi must be below K");
    if (!std::isfinite(sx) || !std::isfinite(sy)) return bad(msg, MSD_ERR_INVALID, "sx and sy must be finite");
    if (max_points < 1 || max_points > MAX_POINTS) return bad(msg, MSD_ERR_UNSUPPORTED, "max_points outside 1 .. 512");
    if ((k_hi - k_lo + 1) * frames > 0x7fffffffLL) return bad(msg, MSD_ERR_UNSUPPORTED, "more than 2^31 - 1 cells");
    return MSD_OK;
}

// the order-preserving 64-bit key of a float64: a < b <=> key(a) < key(b) for non-NaN a, b with -0.0 taken as +0.0
inline uint64_t peak_key(double p) {
    if (p == 0.0) p = 0.0;
    uint64_t b;
    static_assert(sizeof b == sizeof p, "float64");
    __builtin_memcpy(&b, &p, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct Summary {
    int32_t n_clusters = 0, n_critical = 0, n_noncritical = 0, n_noise = 0;
};

// the restatement: labels[n], boxes[4 n_clusters]; plain loops, no bit tricks
inline Summary dbscan_ref(const double *xy, int n, double eps, int min_samples, double critical_min_extent,
                          std::vector<int32_t> &labels, std::vector<double> &boxes) {
    const double eps2 = eps * eps;
    auto adj = [&](int i, int j) {
        const double dx = xy[2 * i] - xy[2 * j], dy = xy[2 * i + 1] - xy[2 * j + 1];
        const double a = dx * dx, b = dy * dy;
        return (a + b) <= eps2;
    };
    std::vector<char> core((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += adj(i, j);
        core[(size_t)i] = cnt >= min_samples;
    }
    labels.assign((size_t)n, -1);
    int next = 0;
    std::vector<int> stack;
    for (int s = 0; s < n; ++s) {
        if (!core[(size_t)s] || labels[(size_t)s] >= 0) continue;
        labels[(size_t)s] = next;
        stack.assign(1, s);
        while (!stack.empty()) {
            const int i = stack.back();
            stack.pop_back();
            for (int j = 0; j < n; ++j)
                if (core[(size_t)j] && labels[(size_t)j] < 0 && adj(i, j)) {
                    labels[(size_t)j] = next;
                    stack.push_back(j);
                }
        }
        ++next;
    }
    for (int i = 0; i < n; ++i) {
        if (core[(size_t)i]) continue;
        int best = -1;
        for (int j = 0; j < n; ++j)
            if (core[(size_t)j] && adj(i, j) && (best < 0 || labels[(size_t)j] < best)) best = labels[(size_t)j];
        labels[(size_t)i] = best;
    }
    Summary s;
    s.n_clusters = next;
    boxes.assign(4 * (size_t)next, 0.0);
    std::vector<char> seen((size_t)next, 0);
    for (int i = 0; i < n; ++i) {
        const int l = labels[(size_t)i];
        if (l < 0) {
            ++s.n_noise;
            continue;
        }
        double *b = &boxes[4 * (size_t)l];
        const double x = xy[2 * i], y = xy[2 * i + 1];
        if (!seen[(size_t)l]) {
            seen[(size_t)l] = 1;
            b[0] = b[2] = x;
            b[1] = b[3] = y;
        } else {
            if (x < b[0]) b[0] = x;
            if (y < b[1]) b[1] = y;
            if (x > b[2]) b[2] = x;
            if (y > b[3]) b[3] = y;
        }
    }
    for (int l = 0; l < next; ++l) {
        if ((boxes[4 * (size_t)l + 2] - boxes[4 * (size_t)l]) >= critical_min_extent)
            ++s.n_critical;
        else
            ++s.n_noncritical;
    }
    return s;
}

// the point extraction's restatement over one image spec[K][ld]; returns the candidate count
inline int64_t peaks_ref(const double *spec, int64_t frames, int64_t ld, int k_lo, int k_hi, double thr, double sx,
                         double sy, int max_points, std::vector<double> &xy, std::vector<int32_t> &cell) {
    const int64_t nk = k_hi - k_lo + 1;
    std::vector<int32_t> cand;
    for (int64_t t = 0; t < frames; ++t)
        for (int64_t kk = 0; kk < nk; ++kk)
            if (spec[(k_lo + kk) * ld + t] > thr) cand.push_back((int32_t)(t * nk + kk));
    const int64_t ncand = (int64_t)cand.size();
    auto val = [&](int32_t c) { return spec[(k_lo + c % nk) * ld + c / nk]; };
    std::vector<char> keep(cand.size(), 1);
    if (ncand > max_points) {
        // drop the smallest, the later cell first among equals, until max_points are left (quadratic, exact)
        for (int64_t drop = ncand - max_points; drop > 0; --drop) {
            int64_t w = -1;
            for (int64_t i = 0; i < ncand; ++i) {
                if (!keep[(size_t)i]) continue;
                if (w < 0 || val(cand[(size_t)i]) <= val(cand[(size_t)w])) w = i;
            }
            keep[(size_t)w] = 0;
        }
    }
    xy.clear();
    cell.clear();
    for (int64_t i = 0; i < ncand; ++i) {
        if (!keep[(size_t)i]) continue;
        const int32_t c = cand[(size_t)i];
        cell.push_back(c);
        xy.push_back((double)(c / nk) * sx);
        xy.push_back((double)(c % nk) * sy);
    }
    return ncand;
}

}  // namespace cluster
}  // namespace msd
