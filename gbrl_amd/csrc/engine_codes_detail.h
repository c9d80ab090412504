// engine_codes_detail.h -- the few helpers more than one of the data-set units needs (engine_step_detail.h has the list of the units):
//   runs_on           engine_codes.hip, engine_fit_prepared.hip
//   walked_split_rows / walked_columns   engine_importance.hip, engine_pd.hip
//   mean_loss         engine_objective.hip, engine_fit_prepared.hip
//   check_auc_column  engine_objective.hip, engine_fit_prepared.hip
//   metric_counts     engine_objective.hip, engine_fit_prepared.hip
#pragma once
#include "engine_step_detail.h"
#include "metric_core.h"
#include "objective_core.h"

namespace gbrl {
namespace detail {

// greedy: a tree of one leaf -- the walk of such a tree finds no leaf of its own and runs on into the next tree (Q7)
inline bool runs_on(const Model &model, int t) { return !model.oblivious() && model.leaf_count(t) == 1; }

// the split rows the walk of the trees [0, stop) reads (greedy: through the trees a trailing run of one-leaf trees runs on into, as check_code_range counts them)
inline size_t walked_split_rows(const Model &model, int stop) {
    const int T = model.meta.n_trees;
    int end = stop;
    while (end < T && runs_on(model, end - 1)) ++end;
    return model.oblivious() ? static_cast<size_t>(end) : static_cast<size_t>(end < T ? model.tree_indices[end] : model.meta.n_leaves);
}

// used[f] = 1 for every column f < F that a numeric condition of those split rows tests: ONE rule for "the walk reads this column"
inline std::vector<uint8_t> walked_columns(const Model &model, int stop, int F) {
    std::vector<uint8_t> used(static_cast<size_t>(F), 0);
    const size_t MD = model.meta.max_depth, s1 = walked_split_rows(model, stop);
    for (size_t s = 0; s < s1; ++s)
        for (size_t d = 0; d < MD && static_cast<int>(d) < model.depths[s]; ++d) {
            const size_t c = s * MD + d;
            const int f = model.feature_indices[c];
            if (model.is_numerics[c] && f >= 0 && f < F) used[f] = 1;
        }
    return used;
}

// the mean loss of an objective from the sum of its row losses: rmse is staged_loss's expression
// (rows: the row count, or with weights their float64 sum W)
inline double mean_loss(int objective, double sum, double rows) { return objective == kern::kObjRmse ? std::sqrt(0.5 * sum / rows) : sum / rows; }

// a column of one class has no AUC
inline void check_auc_column(const char *what, int d, uint64_t P, uint64_t N) {
    if (P == 0 || N == 0)
        throw InvalidArgument(std::string(what) + ": column " + std::to_string(d) + " of the targets has no " + (P == 0 ? "positive" : "negative") +
                              " row (a target above 0.5 is positive): its AUC is not defined");
}

// A metric's device integers in the layout kern::metric_value reads: the error's count per column, or per column (2U, P, N) from row[d] = 2U and
// the column's positives among n rows
inline std::vector<uint64_t> metric_counts(int metric, int C, const unsigned long long *row, const unsigned long long *positives, int n) {
    std::vector<uint64_t> c(static_cast<size_t>(C) * kern::metric_count_width(metric), 0);
    for (int d = 0; d < C; ++d) {
        if (metric != kern::kMetricAuc) { c[d] = row[d]; continue; }
        c[3 * d] = row[d]; c[3 * d + 1] = positives[d]; c[3 * d + 2] = static_cast<uint64_t>(n) - positives[d];
    }
    return c;
}

}  // namespace detail

using detail::runs_on;
using detail::walked_split_rows;
using detail::walked_columns;
using detail::mean_loss;
using detail::check_auc_column;
using detail::metric_counts;

}  // namespace gbrl
