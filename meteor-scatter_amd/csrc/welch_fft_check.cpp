// CPU check of the pruned real transform welch_fft.hip runs (welch_fft_plan.h: the plan, the table of
// roots, the modulation, the Stockham passes and the bin ownership), in float64 against a long-double
// DFT of the same real values followed by zeros.  For every (nperseg, nfft):
//   * every bin 0 .. nfft/2 is owned by exactly one output of one sub-transform;
//   * every bin lies within chain u sum_n |v_n| of the long-double DFT, u = 2^-53, chain counted from
//     the header's roundings by the rules of tests/spec_signals.py -- the fold 1, the modulation 2.41
//     (one rounded product per component and the rounded root), log2 Lp add levels, a rounded
//     twiddle product (4.24) in front of every pass but the first -- and rounded up;
//   * the axes of the table of roots are exact.
// The shapes are those of tests/test_gpu_welch_spectrum.py and the corners of the plan (Lp = 2, a
// segment of one sample, nperseg one past a power of two, the in-place sizes).
// No HIP.  `make -C meteor-scatter_amd/csrc welch_fft_check` builds build/welch_fft_check_san with
// g++ -fsanitize=address,undefined.
//   welch_fft_check [SEED]     prints one "ok ..." line per shape, or "FAIL ..."
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "welch_fft_plan.h"

namespace {

using msd::wfft::cd;
using msd::wfft::Plan;

double chain_of(const Plan &P) {
    const double cmul = 2.0 * std::sqrt(2.0) + std::sqrt(2.0);
    return std::ceil(1.0 + (1.0 + std::sqrt(2.0)) + (P.logLp & 1) + 2.0 * (P.logLp / 2) + cmul * (P.npass > 0 ? P.npass - 1 : 0));
}

// the plan on the CPU: X[k], k = 0 .. nfft/2, of v[0 .. nperseg); owner[k] counts the outputs that own k
void run_plan(const Plan &P, const std::vector<cd> &W, const std::vector<double> &v, std::vector<cd> &X,
              std::vector<int> &owner) {
    std::vector<cd> a((size_t)P.Lp), b((size_t)P.Lp);
    for (int r = 0; r < P.nsub; ++r) {
        for (int n = 0; n < P.Lp; ++n) {
            const double v0 = n < P.nperseg ? v[(size_t)n] : 0.0;
            const double v1 = P.fold && n + P.Lp < P.nperseg ? v[(size_t)(n + P.Lp)] : 0.0;
            a[(size_t)n] = msd::wfft::modulated(P, r, v0, v1, W[(size_t)msd::wfft::mod_index(P, r, n)]);
        }
        cd *src = a.data(), *dst = b.data();
        for (int p = 0; p < P.npass; ++p) {
            const int rdx = msd::wfft::pass_radix(P, p), Ns = msd::wfft::pass_ns(P, p);
            for (int j = 0; j < P.Lp / rdx; ++j) {
                if (rdx == 2) msd::wfft::butterfly<2>(src, dst, W.data(), P.Lp, P.nfft, Ns, j);
                else msd::wfft::butterfly<4>(src, dst, W.data(), P.Lp, P.nfft, Ns, j);
            }
            cd *t = src;
            src = dst;
            dst = t;
        }
        for (int q = 0; q < P.Lp; ++q) {
            const int k = msd::wfft::owned_bin(P, r, q);
            if (k < 0) continue;
            ++owner[(size_t)k];
            // an output past nfft/2 is the conjugate of the bin it owns
            X[(size_t)k] = r + P.R * q <= P.nfft / 2 ? src[q] : cd{src[q].x, -src[q].y};
        }
    }
}

bool check(int nperseg, int nfft, unsigned seed) {
    Plan P;
    if (!msd::wfft::make_plan(nperseg, nfft, P)) {
        printf("FAIL %d/%d: no plan\n", nperseg, nfft);
        return false;
    }
    if (P.Lp * P.R != nfft || P.R < 2 || (P.fold && P.R != 2) || (!P.fold && P.Lp < nperseg) || (1 << P.logLp) != P.Lp) {
        printf("FAIL %d/%d: inconsistent plan Lp %d R %d fold %d\n", nperseg, nfft, P.Lp, P.R, P.fold);
        return false;
    }
    for (int k = 0; k < P.K; ++k) {  // bin_source inverts owned_bin
        int r = -1, q = -1;
        msd::wfft::bin_source(P, k, r, q);
        if (r < 0 || r >= P.nsub || q < 0 || q >= P.Lp || msd::wfft::owned_bin(P, r, q) != k) {
            printf("FAIL %d/%d: bin %d has source (%d, %d)\n", nperseg, nfft, k, r, q);
            return false;
        }
    }
    std::vector<cd> W((size_t)nfft);
    msd::wfft::unit_roots(nfft, W.data());
    if (W[0].x != 1.0 || W[0].y != 0.0 || W[(size_t)nfft / 4].x != 0.0 || W[(size_t)nfft / 4].y != -1.0 ||
        W[(size_t)nfft / 2].x != -1.0 || W[(size_t)nfft / 2].y != 0.0) {
        printf("FAIL %d/%d: the table's axes are not exact\n", nperseg, nfft);
        return false;
    }
    const long double tau = 6.283185307179586476925286766559005768L;
    std::vector<long double> wc((size_t)nfft), ws((size_t)nfft);
    for (int j = 0; j < nfft; ++j) wc[(size_t)j] = cosl(tau * j / nfft), ws[(size_t)j] = -sinl(tau * j / nfft);
    std::mt19937 rng(seed + 31u * (unsigned)nperseg + (unsigned)nfft);
    std::normal_distribution<double> g(0.0, 1.0);
    const double chain = chain_of(P), u = std::ldexp(1.0, -53);
    double worst = 0.0;
    for (int trial = 0; trial < 3; ++trial) {
        std::vector<double> v((size_t)nperseg);
        if (trial == 2) {
            for (auto &e : v) e = 0.0;
            v[(size_t)(nperseg - 1)] = 1.0;  // the last sample alone (the folded half when there is one)
        } else {
            const double dc = trial ? 1000.0 : 0.0;
            for (auto &e : v) e = dc + g(rng);
        }
        long double l1 = 0;
        for (double e : v) l1 += fabsl((long double)e);
        std::vector<cd> X((size_t)P.K, cd{0.0, 0.0});
        std::vector<int> owner((size_t)P.K, 0);
        run_plan(P, W, v, X, owner);
        for (int k = 0; k < P.K; ++k) {
            if (owner[(size_t)k] != 1) {
                printf("FAIL %d/%d: bin %d owned %d times\n", nperseg, nfft, k, owner[(size_t)k]);
                return false;
            }
            long double re = 0, im = 0;
            for (int n = 0; n < nperseg; ++n) {
                const size_t t = (size_t)(((long long)n * k) & (nfft - 1));
                re += v[(size_t)n] * wc[t];
                im += v[(size_t)n] * ws[t];
            }
            const double e = (double)hypotl((long double)X[(size_t)k].x - re, (long double)X[(size_t)k].y - im);
            const double bound = chain * u * (double)l1;
            if (!(e <= bound)) {
                printf("FAIL %d/%d trial %d: bin %d off by %.3g, bound %.3g (chain %g)\n", nperseg, nfft, trial, k, e, bound,
                       chain);
                return false;
            }
            if (bound > 0 && e / bound > worst) worst = e / bound;
        }
    }
    printf("ok %d/%d: Lp %d, %d sub-transforms, %d passes%s, chain %g, worst error %.3f of the bound\n", nperseg, nfft, P.Lp,
           P.nsub, P.npass, P.fold ? ", folded" : "", chain, worst);
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atol(argv[1]) : 1u;
    static const int shapes[][2] = {{256, 4096}, {256, 256}, {16, 16},   {200, 256},  {256, 512},  {256, 16384},
                                    {8192, 16384}, {3000, 4096}, {1, 16},  {2, 16},     {9, 16},     {129, 4096},
                                    {4096, 8192}, {2049, 16384}, {16384, 16384}};
    bool ok = true;
    for (const auto &s : shapes) ok = check(s[0], s[1], seed) && ok;
    Plan P;
    if (msd::wfft::make_plan(16, 24, P) || msd::wfft::make_plan(256, 32768, P) || msd::wfft::make_plan(8, 8, P) ||
        msd::wfft::make_plan(0, 16, P) || msd::wfft::make_plan(17, 16, P)) {
        printf("FAIL: a plan for an unsupported shape\n");
        ok = false;
    }
    return ok ? 0 : 1;
}
