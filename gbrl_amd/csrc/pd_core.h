// pd_core.h -- the host half of partial dependence on a prepared data set (engine_pd.hip calls it, pd_rows.hip has the kernels; no device and no
// HIP header is needed: tests/cxx/pd_core_check.cpp compiles it alone and checks every rule against brute force).
//
// A tree ensemble on binned data is a step function of each column: a numeric condition on column c is `code > bin`, so the prediction can change,
// as a function of the code of c, only between bin and bin + 1 for a bin that some walked condition on c tests.
//   pd_break_codes   bins(c) = the sorted distinct bins of the numeric conditions on c among the first `split_rows` split rows (the rows the walk of
//                    the trees reads: the caller counts them, greedy run-on trees included); codes(c) = [0] + [b + 1 for b in bins(c)], ascending,
//                    k + 1 entries.  Segment j is the code range [codes[j], codes[j + 1] - 1] (the last one runs to B): every code of a segment
//                    answers every walked condition on c alike, so its first code stands for it.  A column no condition tests: [0].
//   pd_segment_of    the segment of any code g >= 0: the last j with codes[j] <= g.  The definition that the documents state as
//                    numpy.searchsorted(codes, g, side="right") - 1: the library itself never looks a segment up (a caller reads the curve at a
//                    code that way), so its only caller is the check program, which holds it against the break rule
//   pd_append_cells  the cells of an entry as variants: one column -> one variant per code; two columns -> the row-major product codes0 x codes1
//                    (gbrl_hip_partial_dependence_cells: the Python layer builds every entry's variants through it)
//   PdVariant        what a launch walks: up to two columns held at a constant code for every row; col1 = -1: one column; col0 = -1: none (the baseline)
//
// The launch plan.  A launch of V variants over m rows of D outputs writes V x D x nb float64 partials, nb = ceil(m / kPdPartialRows) (one per 64
// consecutive positions of the row list).  pd_launch_variants keeps that scratch under kPdScratchBudget (64 MiB) by cutting the variants of one
// launch: min(kPdMaxLaunchVariants, budget / (8 D nb)), and never below 1 -- a single variant whose partials alone pass the budget (m D > 2^29)
// still runs, with the scratch it needs.  pd_variants_per_block cuts a launch's variants into grid.y runs as permutation importance does: one run
// when the row blocks alone give every CU four blocks (the tile is then read once per launch), more when they do not.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gbrl {
namespace kern {

constexpr int kPdPartialRows = 64;                         // rows per float64 partial (= predict_loss.h's kStagedRows: pd_rows.hip asserts it)
constexpr int kPdMaxLaunchVariants = 64;                   // (= kPermLaunchVariants)
constexpr size_t kPdScratchBudget = size_t(64) << 20;      // bytes of partials one launch may write
constexpr long long kPdMaxVariants = 1ll << 20;            // launched variants of one call

struct PdVariant { int32_t col0, code0, col1, code1; };

// the split conditions of a model beside their bins (Engine::condition_bins' table: a used numeric slot has its bin, every other slot is negative)
struct PdConditions {
    const int32_t *depths;            // [S]
    const int32_t *feature_indices;   // [S][max_depth]
    const uint8_t *is_numerics;       // [S][max_depth]
    const int32_t *bins;              // [S][max_depth]
    int max_depth;
};

inline std::vector<int32_t> pd_break_codes(const PdConditions &c, size_t split_rows, int col) {
    std::vector<int32_t> codes;
    for (size_t s = 0; s < split_rows; ++s)
        for (int d = 0; d < c.max_depth && d < c.depths[s]; ++d) {
            const size_t k = s * static_cast<size_t>(c.max_depth) + d;
            if (c.is_numerics[k] && c.feature_indices[k] == col && c.bins[k] >= 0) codes.push_back(c.bins[k] + 1);
        }
    codes.push_back(0);
    std::sort(codes.begin(), codes.end());
    codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
    return codes;
}

inline int pd_segment_of(const int32_t *codes, int n_codes, int g) {
    return static_cast<int>(std::upper_bound(codes, codes + n_codes, static_cast<int32_t>(g)) - codes) - 1;
}

inline long long pd_cell_count(int n0, int n1 /* 0: one column */) { return static_cast<long long>(n0) * (n1 > 0 ? n1 : 1); }

inline void pd_append_cells(std::vector<PdVariant> &out, int col0, const int32_t *codes0, int n0, int col1 = -1, const int32_t *codes1 = nullptr, int n1 = 0) {
    for (int i = 0; i < n0; ++i) {
        if (col1 < 0) { out.push_back(PdVariant{col0, codes0[i], -1, 0}); continue; }
        for (int j = 0; j < n1; ++j) out.push_back(PdVariant{col0, codes0[i], col1, codes1[j]});
    }
}

inline int pd_partials(long long m) { return static_cast<int>((m + kPdPartialRows - 1) / kPdPartialRows); }

inline int pd_launch_variants(long long m, int D, size_t budget = kPdScratchBudget) {
    const unsigned long long per_variant = sizeof(double) * static_cast<unsigned long long>(D < 1 ? 1 : D) * static_cast<unsigned long long>(std::max(1, pd_partials(m)));
    const unsigned long long fit = budget / per_variant;
    return static_cast<int>(std::min<unsigned long long>(kPdMaxLaunchVariants, std::max<unsigned long long>(1, fit)));
}

inline int pd_variants_per_block(int row_blocks, int n_variants, int cus) {
    const int want = 4 * cus;
    const int runs = std::min(n_variants, std::max(1, (want + row_blocks - 1) / std::max(1, row_blocks)));
    return (n_variants + runs - 1) / std::max(1, runs);
}

}  // namespace kern
}  // namespace gbrl
