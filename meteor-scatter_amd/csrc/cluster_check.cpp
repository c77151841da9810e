// CPU check of cluster_plan.h (the header cluster.hip compiles), built with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer (make cluster_check) and run by tests/test_cluster_host.py.  No HIP.
// Prints one "ok <head>: ..." line per check; any other output or a non-zero exit is a failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <random>

#include "cluster_plan.h"

using namespace msd::cluster;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static int code(double eps, double ext, int ms, int mp) {
    msd_cluster_cfg c{eps, ext, ms, mp};
    const char *msg = nullptr;
    const int rc = validate(&c, &msg);
    CHECK((rc == MSD_OK) == (msg == nullptr));
    return rc;
}

static void refusals() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(code(30, 5, 5, 500) == MSD_OK && code(0, 0, 1, 1) == MSD_OK && code(1e300, -1, 1 << 30, 512) == MSD_OK);
    CHECK(code(-1, 5, 5, 500) == MSD_ERR_INVALID && code(inf, 5, 5, 500) == MSD_ERR_INVALID);
    CHECK(code(nan, 5, 5, 500) == MSD_ERR_INVALID && code(30, nan, 5, 500) == MSD_ERR_INVALID);
    CHECK(code(30, 5, 0, 500) == MSD_ERR_INVALID && code(30, 5, -3, 500) == MSD_ERR_INVALID);
    CHECK(code(30, 5, 5, 0) == MSD_ERR_UNSUPPORTED && code(30, 5, 5, 513) == MSD_ERR_UNSUPPORTED);
    CHECK(validate(nullptr, nullptr) == MSD_ERR_INVALID);
    const char *msg = nullptr;
    CHECK(validate_peaks(1025, 145, 160, 328, 491, 3.4, 2.2, 500, &msg) == MSD_OK);
    CHECK(validate_peaks(1025, 145, 160, 491, 328, 1, 1, 500, &msg) == MSD_ERR_INVALID);
    CHECK(validate_peaks(1025, 145, 160, 328, 1025, 1, 1, 500, &msg) == MSD_ERR_INVALID);
    CHECK(validate_peaks(1025, 145, 160, -1, 4, 1, 1, 500, &msg) == MSD_ERR_INVALID);
    CHECK(validate_peaks(1025, 145, 144, 0, 4, 1, 1, 500, &msg) == MSD_ERR_INVALID);
    CHECK(validate_peaks(0, 0, 0, 0, 0, 1, 1, 500, &msg) == MSD_ERR_INVALID);
    CHECK(validate_peaks(8, 4, 4, 0, 7, nan, 1, 500, &msg) == MSD_ERR_INVALID);
    CHECK(validate_peaks(8, 4, 4, 0, 7, 1, 1, 0, &msg) == MSD_ERR_UNSUPPORTED);
    CHECK(validate_peaks(8, 4, 4, 0, 7, 1, 1, 513, &msg) == MSD_ERR_UNSUPPORTED);
    CHECK(validate_peaks(8193, (int64_t)1 << 20, (int64_t)1 << 20, 0, 8192, 1, 1, 500, &msg) == MSD_ERR_UNSUPPORTED);
    CHECK(validate_peaks(8, 0, 0, 0, 7, 1, 1, 1, &msg) == MSD_OK);
    std::printf("ok refusals: cfg and window\n");
}

static void layout() {
    CHECK(WORDS == 8 && ROW_WORDS % 2 == 1);
    CHECK(LDS_ADJ == 512 * 9 * 8 && LDS_XY == 8192 && LDS_LABELS == 4096);
    CHECK(LDS_CLUSTER <= 64 * 1024 && 3 * LDS_CLUSTER <= 160 * 1024);
    // a wave's 32-lane half reads rows i .. i + 31 at one word: 32 distinct 8-byte slots of the 64 banks
    for (int w = 0; w < WORDS; ++w) {
        bool used[32] = {};
        for (int i = 0; i < 32; ++i) {
            const int slot = ((i * ROW_WORDS + w) * 2 % 64) / 2;
            CHECK(!used[slot]);
            used[slot] = true;
        }
    }
    std::printf("ok layout: cluster %zu B, peaks %zu B\n", LDS_CLUSTER, LDS_PEAKS);
}

static void keys() {
    const double inf = std::numeric_limits<double>::infinity();
    const double v[] = {-inf, -1e300, -1.0, -5e-324, 0.0, 5e-324, 1e-300, 1.0, 1.0 + 2.3e-16, 1e300, inf};
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) CHECK((v[i] < v[j]) == (peak_key(v[i]) < peak_key(v[j])));
    CHECK(peak_key(-0.0) == peak_key(0.0));
    std::printf("ok keys: %d values\n", n);
}

// an independent DBSCAN: union-find over core-core edges, ids by first appearance in index order
static std::vector<int32_t> dbscan_uf(const std::vector<double> &xy, double eps, int ms) {
    const int n = (int)xy.size() / 2;
    auto adj = [&](int i, int j) {
        const double dx = xy[2 * i] - xy[2 * j], dy = xy[2 * i + 1] - xy[2 * j + 1];
        return dx * dx + dy * dy <= eps * eps;
    };
    std::vector<int> core(n), parent(n);
    std::iota(parent.begin(), parent.end(), 0);
    for (int i = 0; i < n; ++i) {
        int c = 0;
        for (int j = 0; j < n; ++j) c += adj(i, j);
        core[i] = c >= ms;
    }
    auto find = [&](int a) {
        while (parent[a] != a) a = parent[a] = parent[parent[a]];
        return a;
    };
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (core[i] && core[j] && adj(i, j)) {
                const int a = find(i), b = find(j);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);
            }
    std::vector<int32_t> id(n, -1), lab(n, -1);
    int next = 0;
    for (int i = 0; i < n; ++i)
        if (core[i]) {
            const int r = find(i);
            if (id[r] < 0) id[r] = next++;
            lab[i] = id[r];
        }
    for (int i = 0; i < n; ++i)
        if (!core[i])
            for (int j = 0; j < n; ++j)
                if (core[j] && adj(i, j) && (lab[i] < 0 || lab[j] < lab[i])) lab[i] = lab[j];
    return lab;
}

static void dbscan_cases() {
    std::vector<int32_t> lab;
    std::vector<double> box;
    // the contested border of tests/test_cluster_ref.py
    std::vector<double> p = {0, 0, 1, 0, 0, 1, 1, 1, 0, 2, 8, 0, 9, 0, 8, 1, 9, 1, 9, 2, 4.5, -3.5};
    Summary s = dbscan_ref(p.data(), 11, 5.0, 5, 5.0, lab, box);
    CHECK((lab == std::vector<int32_t>{0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0}));
    CHECK(s.n_clusters == 2 && s.n_noise == 0 && s.n_critical == 0 && s.n_noncritical == 2);
    CHECK(box[0] == 0 && box[1] == -3.5 && box[2] == 4.5 && box[3] == 2);  // the border point widens box 0
    CHECK(box[4] == 8 && box[5] == 0 && box[6] == 9 && box[7] == 2);
    s = dbscan_ref(p.data(), 11, 5.0, 5, 4.5, lab, box);  // extent == the bound: critical
    CHECK(s.n_critical == 1 && s.n_noncritical == 1);
    // 3-4-5 at eps 5: the tie is inside
    std::vector<double> q = {0, 0, 3, 4};
    s = dbscan_ref(q.data(), 2, 5.0, 2, 5.0, lab, box);
    CHECK(lab[0] == 0 && lab[1] == 0 && s.n_clusters == 1 && s.n_noncritical == 1);
    s = dbscan_ref(q.data(), 2, 5.0, 3, 5.0, lab, box);
    CHECK(lab[0] == -1 && lab[1] == -1 && s.n_clusters == 0 && s.n_noise == 2);
    s = dbscan_ref(q.data(), 2, 4.999, 1, 5.0, lab, box);
    CHECK(lab[0] == 0 && lab[1] == 1 && s.n_clusters == 2);
    s = dbscan_ref(q.data(), 0, 5.0, 1, 5.0, lab, box);
    CHECK(lab.empty() && box.empty() && s.n_clusters == 0 && s.n_noise == 0);
    // a 512-point chain at spacing == eps
    std::vector<double> c(1024);
    for (int i = 0; i < 512; ++i) c[2 * i] = 30.0 * i, c[2 * i + 1] = 0;
    s = dbscan_ref(c.data(), 512, 30.0, 3, 5.0, lab, box);
    CHECK(s.n_clusters == 1 && s.n_noise == 0 && box[2] == 30.0 * 511 && s.n_critical == 1);
    CHECK(lab == dbscan_uf(c, 30.0, 3));
    // two chains joined only by the last point: one cluster, id 0
    std::vector<double> j;
    for (int i = 0; i < 100; ++i) j.push_back(i), j.push_back(0);
    for (int i = 0; i < 100; ++i) j.push_back(i), j.push_back(10);
    j.push_back(99), j.push_back(5);
    s = dbscan_ref(j.data(), 201, 5.0, 2, 5.0, lab, box);
    CHECK(s.n_clusters == 1 && lab[100] == 0 && lab[200] == 0);
    s = dbscan_ref(j.data(), 200, 5.0, 2, 5.0, lab, box);
    CHECK(s.n_clusters == 2 && lab[0] == 0 && lab[100] == 1);
    std::printf("ok dbscan: fixed cases\n");

    std::mt19937_64 rng(12345);
    int fits = 0;
    for (int n : {1, 5, 63, 64, 65, 200, 511, 512})
        for (double eps : {3.0, 5.0, 8.0, 30.0})
            for (int ms : {1, 2, 3, 5, 8}) {
                const int span = 4 + (int)(rng() % (unsigned)(6 * (int)std::sqrt((double)n) + 10));
                std::vector<double> r(2 * (size_t)n);
                for (auto &v : r) v = (double)(rng() % (unsigned)span);
                s = dbscan_ref(r.data(), n, eps, ms, 5.0, lab, box);
                CHECK(lab == dbscan_uf(r, eps, ms));
                CHECK(s.n_critical + s.n_noncritical == s.n_clusters && (int)box.size() == 4 * s.n_clusters);
                int noise = 0;
                for (int i = 0; i < n; ++i) {
                    noise += lab[i] < 0;
                    if (lab[i] >= 0) {
                        const double *b = &box[4 * (size_t)lab[i]];
                        CHECK(b[0] <= r[2 * i] && r[2 * i] <= b[2] && b[1] <= r[2 * i + 1] && r[2 * i + 1] <= b[3]);
                    }
                }
                CHECK(noise == s.n_noise);
                ++fits;
            }
    std::printf("ok dbscan: %d random fits against union-find\n", fits);
}

static void peaks() {
    std::mt19937_64 rng(99);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int runs = 0;
    for (int levels : {2, 3, 7, 1000})
        for (int cap : {1, 4, 25, 512}) {
            const int K = 12, ld = 40, frames = 33, k_lo = 2, k_hi = 9, nk = k_hi - k_lo + 1;
            std::vector<double> spec((size_t)K * ld);
            for (auto &v : spec) v = (double)(rng() % (unsigned)levels);
            for (int k = 0; k < K; ++k)
                for (int t = frames; t < ld; ++t) spec[(size_t)k * ld + t] = (k & 1) ? nan : 1e300;  // the padding
            for (int t = 0; t < ld; ++t) spec[(size_t)t] = spec[(size_t)(K - 1) * ld + t] = 1e300;  // rows outside
            spec[(size_t)k_lo * ld] = inf;
            spec[(size_t)k_hi * ld + frames - 1] = nan;
            for (double thr : {-1.0, 0.0, 1.0, 1e9}) {
                std::vector<double> xy;
                std::vector<int32_t> cell;
                const int64_t ncand = peaks_ref(spec.data(), frames, ld, k_lo, k_hi, thr, 3.5, 2.25, cap, xy, cell);
                // independently: sort the candidates by (value descending, cell ascending)
                std::vector<int32_t> all;
                for (int c = 0; c < nk * frames; ++c)
                    if (spec[(size_t)(k_lo + c % nk) * ld + c / nk] > thr) all.push_back(c);
                CHECK(ncand == (int64_t)all.size());
                auto val = [&](int32_t c) { return spec[(size_t)(k_lo + c % nk) * ld + c / nk]; };
                std::stable_sort(all.begin(), all.end(), [&](int32_t a, int32_t b) { return val(a) > val(b); });
                if ((int)all.size() > cap) all.resize((size_t)cap);
                std::sort(all.begin(), all.end());
                CHECK(all == cell && xy.size() == 2 * cell.size());
                for (size_t i = 0; i < cell.size(); ++i) {
                    CHECK(xy[2 * i] == (double)(cell[i] / nk) * 3.5 && xy[2 * i + 1] == (double)(cell[i] % nk) * 2.25);
                    CHECK(val(cell[i]) < 1e300 || val(cell[i]) == inf);
                }
                ++runs;
            }
        }
    std::printf("ok peaks: %d selections against a stable sort\n", runs);
}

int main() {
    refusals();
    layout();
    keys();
    dbscan_cases();
    peaks();
    return 0;
}
