// Host-only check of gbrl_amd/csrc/pd_core.h (compiled with the address and undefined-behaviour sanitizers and run by tests/test_pd_host.py): the
// break rule against brute force over every code, the segment of a code, the cell list of an entry, and the launch plan against its budget.
#include "pd_core.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace gbrl::kern;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("MISMATCH " __VA_ARGS__); std::printf("  (%s)\n", #cond); std::exit(1); } } while (0)

// random condition tables: S split rows of up to MD conditions, numeric and categorical, some slots unused (bin -1)
struct Table {
    int MD, F, B;
    std::vector<int32_t> depths, feat, bins;
    std::vector<uint8_t> numeric;
    PdConditions view() const { return PdConditions{depths.data(), feat.data(), numeric.data(), bins.data(), MD}; }
};
static Table random_table(std::mt19937_64 &rng, int S, int MD, int F, int B) {
    Table t{MD, F, B, {}, {}, {}, {}};
    for (int s = 0; s < S; ++s) {
        t.depths.push_back(static_cast<int32_t>(rng() % (MD + 1)));
        for (int d = 0; d < MD; ++d) {
            const bool num = rng() % 5 != 0;
            t.numeric.push_back(num ? 1 : 0);
            t.feat.push_back(static_cast<int32_t>(rng() % F));
            t.bins.push_back(d < t.depths.back() && num ? static_cast<int32_t>(rng() % B) : -1);
        }
    }
    return t;
}

// the answers of every walked numeric condition on `col` to code g
static std::vector<bool> answers(const Table &t, size_t rows, int col, int g) {
    std::vector<bool> a;
    for (size_t s = 0; s < rows; ++s)
        for (int d = 0; d < t.depths[s]; ++d) {
            const size_t k = s * t.MD + d;
            if (t.numeric[k] && t.feat[k] == col) a.push_back(g > t.bins[k]);
        }
    return a;
}

static void check_breaks() {
    std::mt19937_64 rng(20250301);
    long tables = 0, codes_checked = 0;
    for (int rep = 0; rep < 400; ++rep) {
        const int S = static_cast<int>(rng() % 60), MD = 1 + static_cast<int>(rng() % 6), F = 1 + static_cast<int>(rng() % 20), B = 1 + static_cast<int>(rng() % 40);
        const Table t = random_table(rng, S, MD, F, B);
        for (size_t rows : {static_cast<size_t>(S), static_cast<size_t>(S / 2), static_cast<size_t>(0)}) {
            for (int col = 0; col < F; ++col, ++tables) {
                const std::vector<int32_t> codes = pd_break_codes(t.view(), rows, col);
                CHECK(!codes.empty() && codes[0] == 0, "codes do not begin with 0\n");
                for (size_t j = 1; j < codes.size(); ++j) CHECK(codes[j] > codes[j - 1] && codes[j] <= B, "codes not ascending inside [0, B]\n");
                // brute force: a break lies at g exactly where the answers to g - 1 and g differ
                std::vector<int32_t> want{0};
                for (int g = 1; g <= B; ++g, ++codes_checked)
                    if (answers(t, rows, col, g) != answers(t, rows, col, g - 1)) want.push_back(g);
                CHECK(codes == want, "table %d, column %d, %zu rows: %zu breaks, brute force %zu\n", rep, col, rows, codes.size(), want.size());
                if (answers(t, rows, col, 0).empty()) CHECK(codes.size() == 1, "an untested column has breaks\n");
                // every code lies in the segment whose first code answers alike
                for (int g = 0; g <= B; ++g) {
                    const int j = pd_segment_of(codes.data(), static_cast<int>(codes.size()), g);
                    CHECK(j >= 0 && j < static_cast<int>(codes.size()) && codes[j] <= g && (j + 1 == static_cast<int>(codes.size()) || g < codes[j + 1]), "segment of %d\n", g);
                    CHECK(answers(t, rows, col, g) == answers(t, rows, col, codes[j]), "code %d answers unlike its segment's first code %d\n", g, codes[j]);
                }
                // a prefix of the split rows never has more breaks
                const std::vector<int32_t> full = pd_break_codes(t.view(), static_cast<size_t>(S), col);
                CHECK(codes.size() <= full.size(), "a prefix has more breaks than the whole\n");
            }
        }
    }
    std::printf("breaks: %ld (table, column) pairs, %ld codes against brute force\n", tables, codes_checked);
}

static void check_cells() {
    const int32_t a[] = {0, 3, 7}, b[] = {0, 5};
    std::vector<PdVariant> v;
    pd_append_cells(v, 4, a, 3);
    CHECK(v.size() == 3 && pd_cell_count(3, 0) == 3, "one column: %zu cells\n", v.size());
    for (int i = 0; i < 3; ++i) CHECK(v[i].col0 == 4 && v[i].code0 == a[i] && v[i].col1 == -1, "one column, cell %d\n", i);
    v.clear();
    pd_append_cells(v, 4, a, 3, 9, b, 2);
    CHECK(v.size() == 6 && pd_cell_count(3, 2) == 6, "pair: %zu cells\n", v.size());
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 2; ++j) {
            const PdVariant &c = v[static_cast<size_t>(i) * 2 + j];   // row-major: the second column runs fastest
            CHECK(c.col0 == 4 && c.code0 == a[i] && c.col1 == 9 && c.code1 == b[j], "pair, cell (%d, %d)\n", i, j);
        }
    CHECK(pd_cell_count(65536, 65536) == 4294967296ll, "cell count overflows\n");
    std::printf("cells: one column and the row-major product of a pair\n");
}

static void check_plan() {
    static_assert(kPdScratchBudget == (size_t(64) << 20) && kPdMaxLaunchVariants == 64 && kPdPartialRows == 64, "the documented plan");
    long plans = 0;
    const long long ms[] = {1, 63, 64, 65, 4097, 65536, 1 << 20, (1 << 20) + 1, 1 << 24, 123456789, 2147483647ll};
    for (long long m : ms)
        for (int D : {1, 3, 8, 64, 65, 128})
            for (size_t budget : {size_t(8), size_t(4096), size_t(1) << 20, kPdScratchBudget}) {
                const int per = pd_launch_variants(m, D, budget);
                const unsigned long long one = 8ull * D * static_cast<unsigned long long>(pd_partials(m));
                CHECK(per >= 1 && per <= kPdMaxLaunchVariants, "m %lld, D %d: %d variants\n", m, D, per);
                CHECK(per == 1 || per * one <= budget, "m %lld, D %d: %d variants x %llu bytes pass the budget %zu\n", m, D, per, one, budget);
                CHECK(per == kPdMaxLaunchVariants || (per + 1) * one > budget, "m %lld, D %d: %d variants leave room for one more\n", m, D, per);
                ++plans;
            }
    CHECK(pd_launch_variants(1 << 20, 8) == 64 && pd_launch_variants(1 << 20, 128) == 4 && pd_launch_variants(65536, 128) == 64, "the documented shapes\n");
    CHECK(pd_partials(1) == 1 && pd_partials(64) == 1 && pd_partials(65) == 2 && pd_partials(2147483647ll) == 33554432, "partials\n");
    for (int blocks : {1, 2, 1000, 1024, 1025, 1 << 20})
        for (int V : {1, 2, 63, 64})
            for (int cus : {1, 256, 304}) {
                const int per = pd_variants_per_block(blocks, V, cus);
                CHECK(per >= 1 && per <= V, "run of %d variants out of %d\n", per, V);
                CHECK(blocks < 4 * cus || per == V, "%d row blocks fill %d CUs: one run\n", blocks, cus);
                ++plans;
            }
    std::printf("plan: %ld plans inside the budget, never below 1\n", plans);
}

int main() {
    check_breaks();
    check_cells();
    check_plan();
    std::printf("partial dependence core: all sections passed\n");
    return 0;
}
