// Host-only check of gbrl_amd/csrc/cv_core.h (compiled with the address and undefined-behaviour sanitizers and run by
// tests/test_control_variates_host.py): the chain's three roundings, the fixed-order sums against long double sums, the statistics of
// cv_finish_host against a plain float64 evaluation, and the launch plan.
#include "cv_core.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace gbrl::kern;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("MISMATCH " __VA_ARGS__); std::printf("  (%s)\n", #cond); std::exit(1); } } while (0)

static void check_chain() {
    std::mt19937_64 rng(19);
    std::uniform_real_distribution<float> u(-2.0f, 2.0f);
    for (int i = 0; i < 100000; ++i) {
        const float m = u(rng), v = u(rng), beta = 0.5f + 0.499f * (u(rng) + 2.0f) / 4.0f, c = cv_sub(1.0f, beta);
        const float a = static_cast<float>(static_cast<double>(beta) * m), b = static_cast<float>(static_cast<double>(c) * v);   // each product rounded once
        CHECK(cv_chain(m, beta, c, v) == static_cast<float>(static_cast<double>(a) + b), "chain step %d\n", i);
    }
    CHECK(cv_beta_ok(0.9f) && !cv_beta_ok(0.0f) && !cv_beta_ok(1.0f) && !cv_beta_ok(NAN), "beta range\n");
    CHECK(cv_scale(0.9f, 0) == 0.0f && cv_scale(0.9f, 1) > 3.16f && cv_scale(0.9f, 1) < 3.17f && cv_scale(0.9f, 1000) == 1.0f, "scale\n");
    CHECK(cv_alpha(3.0f, 1.0f) == 1.0f && cv_alpha(-3.0f, 1.0f) == -1.0f && cv_alpha(0.0f, 0.0f) == 0.0f && cv_alpha(NAN, 1.0f) != cv_alpha(NAN, 1.0f), "alpha\n");
    std::printf("chain: 100000 steps of three roundings, beta, scale, alpha\n");
}

static void check_sums() {
    std::mt19937_64 rng(23);
    std::normal_distribution<double> g(0.0, 1.0);
    for (int S : {1, 2, 63, 64, 65, 1000, 1024}) {
        const int C = 3;
        std::vector<double> part(static_cast<size_t>(S) * C);
        for (double &x : part) x = g(rng);
        for (int c = 0; c < C; ++c) {
            long double want = 0.0L, mag = 0.0L;
            for (int s = 0; s < S; ++s) { want += part[static_cast<size_t>(s) * C + c]; mag += std::fabs(part[static_cast<size_t>(s) * C + c]); }
            CHECK(std::fabs(static_cast<double>(cv_fold(part.data(), S, C, c) - want)) <= 64 * 2.3e-16 * static_cast<double>(mag), "fold of %d slots\n", S);
        }
    }
    std::printf("sums: folds of 1 to 1024 slots against long double\n");
}

static void check_finish() {
    std::mt19937_64 rng(29);
    std::normal_distribution<float> g(0.0f, 1.0f);
    for (long long n : {2ll, 63ll, 65ll, 130ll, 140000ll})
        for (int D : {1, 3}) {
            std::vector<float> G(n * D), M(n * D), ms(n * D), out(n * D), stats(kCvStats * D);
            std::vector<double> part(static_cast<size_t>(cv_walk_slots(n)) * 2 * D);
            for (long long i = 0; i < n * D; ++i) { M[i] = g(rng); G[i] = 0.7f * M[i] + 0.3f * g(rng); }
            cv_finish_host(G.data(), M.data(), n, D, 1.25f, ms.data(), part.data(), out.data(), stats.data());
            for (int j = 0; j < D; ++j) {
                double sg = 0, sm = 0, a = 0, b = 0;
                for (long long r = 0; r < n; ++r) { sg += G[r * D + j]; sm += ms[r * D + j]; }
                const float gbar = static_cast<float>(sg / n), mbar = static_cast<float>(sm / n);
                CHECK(std::fabs(stats[kCvMeanGrads * D + j] - gbar) <= 1.2e-7f * std::fabs(gbar) + 1e-12f && std::fabs(stats[kCvMeanMomentum * D + j] - mbar) <= 1.2e-7f * std::fabs(mbar) + 1e-12f, "means, n %lld\n", n);
                const float gb = stats[kCvMeanGrads * D + j], mb = stats[kCvMeanMomentum * D + j];
                for (long long r = 0; r < n; ++r) {
                    const double mc = cv_sub(ms[r * D + j], mb), gc = cv_sub(G[r * D + j], gb);
                    a += mc * mc; b += gc * mc;
                }
                CHECK(std::fabs(stats[kCvVar * D + j] - static_cast<float>(a / (n - 1))) <= 1.2e-7f * std::fabs(a / (n - 1)), "var, n %lld\n", n);
                CHECK(std::fabs(stats[kCvCov * D + j] - static_cast<float>(b / (n - 1))) <= 1.2e-7f * std::fabs(a / (n - 1)), "cov, n %lld\n", n);
                CHECK(stats[kCvAlpha * D + j] == cv_alpha(stats[kCvCov * D + j], stats[kCvVar * D + j]), "alpha\n");
                for (long long r = 0; r < n; ++r) CHECK(out[r * D + j] == cv_corrected(G[r * D + j], cv_sub(ms[r * D + j], mb), stats[kCvAlpha * D + j]), "result\n");
            }
        }
    std::printf("finish: means, moments, alpha and the corrected gradients at 5 row counts\n");
}

static void check_plan() {
    for (long long n : {2ll, 64ll, 65ll, 1ll << 17, (1ll << 17) + 1, 2147483647ll}) {
        const CvPlan p = cv_plan(n, 128, false, 8);
        CHECK(p.walk_slots == (n + 63) / 64 && p.moment_slots == std::min<long long>(p.walk_slots, kCvMomentSlots) && p.launches == 4, "slots of %lld rows\n", n);
    }
    for (int D : {1, 4, 5, 16, 17, 64, 65, 128}) CHECK(cv_plan(130, 20, false, D).streaming == (D <= 64) && cv_plan(130, 20, false, D).dmax >= D, "D %d\n", D);
    CHECK(cv_plan(130, 623, false, 8).streaming && !cv_plan(130, 624, false, 8).streaming, "the widest float tile\n");   // 64 * 625 * 4 = 160 000 > 156 KiB
    CHECK(cv_plan(130, 77, true, 8).streaming && !cv_plan(130, 78, true, 8).streaming && !cv_plan(130, 20, false, 8, false).streaming, "the widest code tile\n");
    std::printf("plan: slots, template widths, LDS boundaries\n");
}

int main() {
    check_chain();
    check_sums();
    check_finish();
    check_plan();
    std::printf("control variates core: all sections passed\n");
    return 0;
}
