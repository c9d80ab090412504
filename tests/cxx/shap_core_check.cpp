// shap_core_check.cpp -- gbrl_amd/csrc/shap_core.h without a device (tests/test_shap_prepared_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it):
//   1. the reduction rule against a plain loop on random matrices (row counts around the tile, F * D up to 128 * 128, signed zeros, a NaN row);
//   2. the result does not depend on how the rows were cut into chunks: tile partials written chunk by chunk, then finished, give the same bytes;
//   3. the chunk plans at m in {1, 63, 64, 65, 4097} and the default chunk_rows against the budget rule;
//   4. the argument checks.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "shap_core.h"

using namespace gbrl::kern;

namespace {

int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

bool same_bytes(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

// the rule, restated: tiles of 64 rows, sequential float64 sums inside a tile and over the tiles
void plain(const std::vector<float> &phi, long long m, size_t C, std::vector<double> &sum, std::vector<double> &sum_abs) {
    sum.assign(C, 0.0);
    sum_abs.assign(C, 0.0);
    for (size_t c = 0; c < C; ++c) {
        double total = 0.0, total_abs = 0.0;
        for (long long p0 = 0; p0 < m; p0 += 64) {
            volatile double s = 0.0, a = 0.0;   // (volatile: every addition is rounded to float64 on its own)
            for (long long p = p0; p < m && p < p0 + 64; ++p) {
                const float v = phi[static_cast<size_t>(p) * C + c];
                s = s + static_cast<double>(v);
                a = a + static_cast<double>(std::fabs(v));
            }
            total = total + s;
            total_abs = total_abs + a;
        }
        sum[c] = total;
        sum_abs[c] = total_abs;
    }
}

std::vector<float> random_matrix(long long m, size_t C, std::mt19937_64 &rng) {
    std::vector<float> phi(static_cast<size_t>(m) * C);
    std::uniform_real_distribution<float> mag(-1.0f, 1.0f);
    std::uniform_int_distribution<int> expo(-20, 20), kind(0, 15);
    for (float &v : phi) {
        const int k = kind(rng);
        v = k == 0 ? 0.0f : k == 1 ? -0.0f : std::ldexp(mag(rng), expo(rng));   // magnitudes far apart: the order of the additions shows
    }
    return phi;
}

void section_rule() {
    std::mt19937_64 rng(11);
    const long long ms[] = {1, 2, 63, 64, 65, 127, 128, 129, 1000};
    const size_t Cs[] = {1, 3, 17 * 8, 40 * 3};
    for (long long m : ms)
        for (size_t C : Cs) {
            const std::vector<float> phi = random_matrix(m, C, rng);
            std::vector<double> want, want_abs, got(C), got_abs(C);
            plain(phi, m, C, want, want_abs);
            shap_sums_host(phi.data(), m, C, got.data(), got_abs.data());
            CHECK(same_bytes(got, want) && same_bytes(got_abs, want_abs));
        }
    {   // F * D = 128 * 128
        const long long m = 65;
        const size_t C = 128 * 128;
        const std::vector<float> phi = random_matrix(m, C, rng);
        std::vector<double> want, want_abs, got(C), got_abs(C);
        plain(phi, m, C, want, want_abs);
        shap_sums_host(phi.data(), m, C, got.data(), got_abs.data());
        CHECK(same_bytes(got, want) && same_bytes(got_abs, want_abs));
    }
    {   // signed zeros: a column of -0.0 sums to +0.0 (the sum starts from +0.0), its absolute sum too; a NaN row poisons its own column only
        const long long m = 70;
        const size_t C = 3;
        std::vector<float> phi(static_cast<size_t>(m) * C, -0.0f);
        for (long long p = 0; p < m; ++p) phi[static_cast<size_t>(p) * C + 2] = 1.0f;
        phi[5 * C + 1] = std::nanf("");
        std::vector<double> got(C), got_abs(C);
        shap_sums_host(phi.data(), m, C, got.data(), got_abs.data());
        CHECK(got[0] == 0.0 && !std::signbit(got[0]) && got_abs[0] == 0.0 && !std::signbit(got_abs[0]));
        CHECK(std::isnan(got[1]) && std::isnan(got_abs[1]));
        CHECK(got[2] == 70.0 && got_abs[2] == 70.0);
    }
    std::printf("rule: the sums equal the plain loop on every matrix\n");
}

void section_chunks() {
    std::mt19937_64 rng(12);
    const long long m = 4097;
    const size_t C = 24;
    const std::vector<float> phi = random_matrix(m, C, rng);
    std::vector<double> want(C), want_abs(C);
    shap_sums_host(phi.data(), m, C, want.data(), want_abs.data());
    for (int chunk_rows : {64, 128, 1024, 4160, 8192}) {
        const ShapChunkPlan plan = shap_chunk_plan(m, 3, 8, chunk_rows);
        std::vector<double> part(plan.partial_bytes / sizeof(double), -1.0);
        int chunks = 0;
        for (long long p0 = 0; p0 < m; p0 += plan.chunk_rows, ++chunks) {
            const long long count = std::min<long long>(plan.chunk_rows, m - p0);
            CHECK(count <= plan.alloc_rows);
            const float *chunk = phi.data() + static_cast<size_t>(p0) * C;   // (what the scratch holds for this chunk)
            const int tile0 = static_cast<int>(p0 / kShapTileRows);
            for (int t = 0; t < shap_tiles(count); ++t)
                for (size_t c = 0; c < C; ++c) {
                    const int r0 = t * kShapTileRows;
                    double *dst = part.data() + static_cast<size_t>(tile0 + t) * 2 * C;
                    shap_tile_sums(chunk + static_cast<size_t>(r0) * C + c, C, static_cast<int>(std::min<long long>(kShapTileRows, count - r0)), &dst[c], &dst[C + c]);
                }
        }
        CHECK(chunks == plan.n_chunks);
        std::vector<double> got(C), got_abs(C);
        for (size_t c = 0; c < C; ++c) {
            got[c] = shap_finish_sums(part.data() + c, 2 * C, plan.tiles);
            got_abs[c] = shap_finish_sums(part.data() + C + c, 2 * C, plan.tiles);
        }
        CHECK(same_bytes(got, want) && same_bytes(got_abs, want_abs));
    }
    std::printf("chunks: the bytes do not depend on chunk_rows\n");
}

void section_plans() {
    for (long long m : {1ll, 63ll, 64ll, 65ll, 4097ll})
        for (int F : {1, 17, 128})
            for (int D : {1, 8, 128})
                for (int chunk_rows : {0, 64, 128, 4096}) {
                    const ShapChunkPlan p = shap_chunk_plan(m, F, D, chunk_rows);
                    const size_t C = static_cast<size_t>(F) * D;
                    const long long tiles = (m + 63) / 64;
                    CHECK(p.chunk_rows == (chunk_rows ? chunk_rows : shap_default_chunk_rows(F, D)));
                    CHECK(p.chunk_rows % 64 == 0 && p.chunk_rows >= 64);
                    CHECK(p.tiles == tiles && p.partial_bytes == static_cast<size_t>(tiles) * 2 * C * 8);
                    CHECK(p.alloc_rows == std::min<long long>(p.chunk_rows, tiles * 64) && p.scratch_bytes == static_cast<size_t>(p.alloc_rows) * C * 4);
                    CHECK(p.n_chunks == (m + p.chunk_rows - 1) / p.chunk_rows);
                    CHECK(static_cast<long long>(p.n_chunks) * p.chunk_rows >= m && static_cast<long long>(p.n_chunks - 1) * p.chunk_rows < m);
                }
    // the default: the largest multiple of 64 inside the budget, and at least 64
    for (int F : {1, 3, 16, 17, 40, 128, 1000, 4096})
        for (int D : {1, 3, 8, 65, 128}) {
            const long long rows = shap_default_chunk_rows(F, D), row_bytes = 4ll * F * D, budget = 64ll << 20;
            CHECK(rows % 64 == 0 && rows >= 64);
            CHECK(rows == 64 || rows * row_bytes <= budget);
            CHECK((rows + 64) * row_bytes > budget);
        }
    CHECK(shap_default_chunk_rows(128, 8) == 16384 && shap_default_chunk_rows(128, 128) == 1024 && shap_default_chunk_rows(4096, 128) == 64);
    std::printf("plans: chunk plans and the default chunk_rows follow the budget rule\n");
}

void section_checks() {
    for (int ok : {0, 64, 128, 1 << 20}) CHECK(shap_chunk_rows_error(ok).empty());
    for (int bad : {-64, -1, 1, 63, 65, 100}) CHECK(shap_chunk_rows_error(bad).find("is not a positive multiple of 64") != std::string::npos);
    CHECK(shap_matrix_error(1 << 20, 128, 8).empty());
    CHECK(shap_matrix_error((1ll << 31) - 1, 1, 1).empty());
    CHECK(shap_matrix_error(1ll << 31, 1, 1).find("2^31") != std::string::npos);
    CHECK(shap_matrix_error(1 << 20, 128, 16).find("shap_importance_prepared") != std::string::npos);
    CHECK(shap_tree_error(-1, 5).empty() && shap_tree_error(0, 5).empty() && shap_tree_error(4, 5).empty());
    CHECK(shap_tree_error(5, 5).find("outside [0, 5)") != std::string::npos && shap_tree_error(-2, 5).find("tree_idx -2") != std::string::npos);
    CHECK(shap_tree_error(-1, 0) == "the model has no trees");
    std::printf("checks: the refusals that need no device\n");
}

}  // namespace

int main() {
    section_rule();
    section_chunks();
    section_plans();
    section_checks();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all sections passed\n");
    return 0;
}
