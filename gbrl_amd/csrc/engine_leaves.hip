// engine_leaves.hip -- one tree's leaf values set from the rows of a data set (engine_step_detail.h lists the units beside it):
//   Engine::check_leaf_update          what is refused about a leaf rule, its objective and leaf_l2
//   Engine::newton_leaves_prepared     one tree's leaves set to sum g / (sum h + leaf_l2) over a data set's rows (newton_core.h; kern::newton_leaf_sums), the
//                                      rule on the host beside it (newton_values_host); newton_leaves_run is its body, which fit_prepared(leaf_update = newton)
//                                      runs after every step
//   Engine::newton_leaves_prepared_rank  the same from a ranking objective's g and h: rank_gradient's kernels (engine_rank.hip) into two device buffers,
//                                      then that body on them (kern::newton_leaf_sums' buffer form, kObjGiven)
//   Engine::quantile_leaves_prepared   one tree's leaves set to the level's order statistic of the residuals of their rows (quantile_core.h; kern::leaf_quantile),
//                                      the rule on the host beside it (leaf_quantile_host, quantile_rank); quantile_leaves_run is its body, which
//                                      fit_prepared(leaf_update = quantile) runs after every step
#include "engine_codes_detail.h"
#include "newton_core.h"
#include "quantile_core.h"
#include "rank_core.h"

namespace gbrl {

// ---- Newton leaf values: the checks, the rules on the host, one tree's sums on the device and the values from them
void Engine::check_leaf_update(const char *what, int objective, int leaf_update, double leaf_l2) {
    if (leaf_update != kern::kLeafGradient && leaf_update != kern::kLeafNewton && leaf_update != kern::kLeafQuantile)
        throw InvalidArgument(std::string(what) + ": unknown leaf_update " + std::to_string(leaf_update) + " (gradient = 0, newton = 1, quantile = 2)");
    if (!(leaf_l2 >= 0.0) || std::isinf(leaf_l2))
        throw InvalidArgument(std::string(what) + ": leaf_l2 must be finite and >= 0 (and not NaN), got " + std::to_string(leaf_l2));
    if (leaf_update == kern::kLeafNewton && objective == kern::kObjRmse)
        throw InvalidArgument(std::string(what) + ": newton leaf values with the rmse objective are the gradient means the step already stores (use logistic or softmax)");
    if (leaf_update == kern::kLeafNewton && objective == kern::kObjQuantile)
        throw InvalidArgument(std::string(what) + ": newton leaf values with the quantile objective do not exist (its hessian is zero): use leaf_update = quantile");
    if (leaf_update == kern::kLeafQuantile && objective != kern::kObjQuantile)
        throw InvalidArgument(std::string(what) + ": quantile leaf values belong to the quantile objective");
}

void Engine::newton_values_host(const int64_t *sums, int n_leaves, int D, int bits, const float *old_values, const int32_t *depths, double leaf_l2, float *values_out) {
    if (sums == nullptr || old_values == nullptr || depths == nullptr || values_out == nullptr) throw InvalidArgument("newton_values_host: null argument");
    if (n_leaves <= 0 || D < 1) throw InvalidArgument("newton_values_host: leaves and output_dim must be positive");
    if (bits < 0 || bits > 62) throw InvalidArgument("newton_values_host: bits must be in [0, 62]");
    check_leaf_update("newton_values_host", kern::kObjLogistic, kern::kLeafNewton, leaf_l2);
    const double scale = std::ldexp(1.0, bits);
    const size_t W = 2 * static_cast<size_t>(D) + 1;
    for (int l = 0; l < n_leaves; ++l)
        for (int d = 0; d < D; ++d)
            values_out[static_cast<size_t>(l) * D + d] = kern::newton_leaf_value(sums[l * W + d], sums[l * W + D + d], sums[l * W + 2 * D], depths[l], scale, leaf_l2,
                                                                                  old_values[static_cast<size_t>(l) * D + d]);
}

void Engine::newton_leaves_run(const char *what, const PreparedDataset *ds, const kern::CodeRows &cr, int m, const float *d_pred, const void *d_targets, bool abs_index,
                               int objective, int t, double leaf_l2, bool generic, int64_t *sums_out, int *bits_out, float *values_out, const float *d_weights,
                               float weight_max) {
    const gbrl_hip_metadata &md = model.meta;
    hipStream_t s = stream_;
    const int D = md.output_dim;
    const size_t leaf0 = model.first_leaf(t), NL = model.leaf_count(t);
    const size_t W = 2 * static_cast<size_t>(D) + 1, words = NL * W + 1;
    check_code_range(*ds, what, t, t + 1);
    sync_model_to_device();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const bool timed = profiling_ >= 2;
    phase_begin();
    unsigned long long *dacc = zeroed<unsigned long long>(d_newton_acc_, words, "zero leaf sums");
    // (kObjGiven: a ranking objective's g and h from buffers, below the largest query's size, which arrives as weight_max)
    const int bits = d_weights || objective == kern::kObjGiven ? kern::newton_sum_bits(m, weight_max) : kern::newton_sum_bits(m);
    const bool streamed = kern::newton_leaf_sums(mirror_view(), ct, cr, m, t, static_cast<int>(leaf0), static_cast<int>(NL), d_pred, d_targets, abs_index, objective,
                                                 bits, dacc, generic, s, d_weights);
    newton_host_.resize(words);
    read_back(newton_host_.data(), dacc, sizeof(unsigned long long) * words, "D2H leaf sums", "newton_leaves");
    if (timed) join_tail_phase("newton_leaves", "newton_streamed", streamed);   // (1 = the streaming kernel took the sums)
    const unsigned long long flag = newton_host_[words - 1];
    if (flag & kern::kNewtonBadTarget)
        throw InvalidArgument(std::string(what) + ": a logistic target is outside [0, 1] (or NaN): newton leaf values need targets in [0, 1]; the model is unchanged");
    if (flag & kern::kNewtonBadPred)
        throw InvalidArgument(std::string(what) + ": a prediction is not finite: no newton leaf values; the model is unchanged");
    const double scale = std::ldexp(1.0, bits);
    for (size_t l = 0; l < NL; ++l) {
        const long long *a = reinterpret_cast<const long long *>(newton_host_.data()) + l * W;
        float *v = model.values.data() + (leaf0 + l) * D;
        for (int d = 0; d < D; ++d) v[d] = kern::newton_leaf_value(a[d], a[D + d], a[2 * D], model.leaf_depth(t, l), scale, leaf_l2, v[d]);
    }
    ++model.version;
    rewind_values(t);
    if (sums_out) std::memcpy(sums_out, newton_host_.data(), sizeof(int64_t) * NL * W);
    if (bits_out) *bits_out = bits;
    if (values_out) std::memcpy(values_out, model.values.data() + leaf0 * D, sizeof(float) * NL * D);
}

void Engine::newton_leaves_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *pred, bool pred_dev, const void *targets,
                                    bool targets_dev, int objective, int tree, double leaf_l2, int64_t *sums_out, int *bits_out, float *values_out,
                                    const float *weights, bool weights_dev, float weight_max) {
    const gbrl_hip_metadata &md = model.meta;
    const int D = md.output_dim;
    check_prepared_dataset("newton_leaves_prepared", ds);
    if (D > 128) throw Unsupported("newton_leaves_prepared: output_dim > 128");
    if (pred == nullptr) throw InvalidArgument("newton_leaves_prepared: no prediction");
    if (targets == nullptr) throw InvalidArgument("Cannot call newton_leaves_prepared without targets!");
    check_objective("newton_leaves_prepared", objective, D);
    check_leaf_update("newton_leaves_prepared", objective, kern::kLeafNewton, leaf_l2);
    const int t = resolve_tree("newton_leaves_prepared", tree);
    check_row_count("newton_leaves_prepared", "pred", rows, m, ds->n, "sum over");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    if (weights == nullptr && weight_max >= 0.0f) throw InvalidArgument("newton_leaves_prepared: weight_max needs weights");
    if (weights != nullptr && (weight_max != weight_max || weight_max > kern::kWeightMax))
        throw InvalidArgument("newton_leaves_prepared: weight_max must be at most 65536 (and not NaN), got " + std::to_string(weight_max));
    check_code_range(*ds, "newton_leaves_prepared", t, t + 1);
    ensure_device();
    reset_events();
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const size_t n_el = static_cast<size_t>(m) * D, tar_el = objective == kern::kObjSoftmax ? static_cast<size_t>(m) : n_el;
    const float *dp = staged(d_obj_pred_, pred, pred_dev, n_el, "H2D predictions");
    const float *dt = staged(d_obj_targets_, static_cast<const float *>(targets), targets_dev, tar_el, "H2D targets");
    if (objective == kern::kObjSoftmax) check_labels("newton_leaves_prepared", reinterpret_cast<const int32_t *>(dt), m, D, nullptr);
    const float *dw = weights ? staged(d_obj_weights_, weights, weights_dev, static_cast<size_t>(m), "H2D weights") : nullptr;
    if (dw) {   // (the sums divide by no W: weights that are all zero are fine here)
        const float largest = check_weights("newton_leaves_prepared", dw, m, false).max;
        if (weight_max < 0.0f) weight_max = largest;
        else if (weight_max < largest)
            throw InvalidArgument("newton_leaves_prepared: weight_max " + std::to_string(weight_max) + " is below the largest weight given, " + std::to_string(largest));
    }
    newton_leaves_run("newton_leaves_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, dp, dt, /*abs_index=*/false, objective, t,
                      leaf_l2, hooks::on(hooks::CONTINUE_GENERIC), sums_out, bits_out, values_out, dw, dw ? weight_max : 0.0f);
}

// ---- leaf quantiles: the rule on the host, one tree's order statistics on the device and the values from them
int64_t Engine::quantile_rank(int64_t m, float a) {
    if (m < 1 || m > 0x7fffffffll) throw InvalidArgument("quantile_rank: m must be in [1, 2^31 - 1], got " + std::to_string(m));
    if (kern::quantile_bad_level(a)) throw InvalidArgument("quantile_rank: the level " + std::to_string(a) + " is not a finite number strictly inside (0, 1)");
    return kern::quantile_rank(m, a);
}

void Engine::leaf_quantile_host(const float *x, const int32_t *leaves, int m, int D, int n_leaves, const float *alpha, float *values_out, int64_t *counts_out,
                                int64_t *ranks_out) {
    if (x == nullptr || leaves == nullptr) throw InvalidArgument("leaf_quantile_host: null argument");
    if (m <= 0) throw InvalidArgument("leaf_quantile_host: no rows (m must be positive)");
    if (D < 1 || n_leaves < 1) throw InvalidArgument("leaf_quantile_host: leaves and output_dim must be positive");
    check_alpha("leaf_quantile_host", kern::kObjQuantile, alpha, D, false);
    for (size_t i = 0; i < static_cast<size_t>(m) * D; ++i)
        if (kern::quantile_not_finite(x[i])) throw InvalidArgument("leaf_quantile_host: x[" + std::to_string(i / D) + "][" + std::to_string(i % D) + "] is not finite");
    std::vector<std::vector<int32_t>> members(n_leaves);
    for (int r = 0; r < m; ++r)
        if (leaves[r] >= 0 && leaves[r] < n_leaves) members[leaves[r]].push_back(r);
    std::vector<uint32_t> keys;
    for (int l = 0; l < n_leaves; ++l) {
        const std::vector<int32_t> &rows = members[l];
        const long long cnt = static_cast<long long>(rows.size());
        if (counts_out) counts_out[l] = cnt;
        for (int d = 0; d < D; ++d) {
            const size_t at = static_cast<size_t>(l) * D + d;
            const long long k = kern::quantile_rank(cnt, alpha[d]);
            if (ranks_out) ranks_out[at] = k;
            if (values_out == nullptr) continue;
            if (cnt == 0) { values_out[at] = 0.0f; continue; }
            keys.clear();
            for (const int32_t r : rows) keys.push_back(kern::quantile_key(x[static_cast<size_t>(r) * D + d]));
            std::nth_element(keys.begin(), keys.begin() + (cnt - k), keys.end());   // ascending: the k-th largest is element cnt - k
            values_out[at] = kern::quantile_key_value(keys[cnt - k]);
        }
    }
}

void Engine::quantile_leaves_run(const char *what, const PreparedDataset *ds, const kern::CodeRows &cr, int m, const float *d_pred, const float *d_targets,
                                 bool abs_index, const float *d_alpha, int t, bool generic, float *values_out, int64_t *counts_out, int64_t *ranks_out) {
    const gbrl_hip_metadata &md = model.meta;
    hipStream_t s = stream_;
    const int D = md.output_dim;
    const size_t leaf0 = model.first_leaf(t), NL = model.leaf_count(t);
    const size_t nld = NL * D, words = kern::leaf_quantile_result_words(static_cast<int>(NL), D);
    check_code_range(*ds, what, t, t + 1);
    const kern::LeafQuantilePlan plan = kern::leaf_quantile_plan(m, D, static_cast<int>(NL), generic);
    if (!plan.select && !kern::leaf_quantile_fits(m, D))
        throw Unsupported(std::string(what) + ": quantile leaves of a tree with more than " + std::to_string([] { int l = 0; kern::leaf_quantile_geometry(&l, nullptr); return l; }()) +
                          " leaves need rows * output_dim < 2^31 - 2048");
    sync_model_to_device();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const bool timed = profiling_ >= 2;
    phase_begin();
    uint32_t *dres = zeroed<uint32_t>(d_lq_res_, words, "zero leaf quantiles");
    void *scratch = d_lq_scratch_.ensure(plan.scratch_bytes);
    kern::leaf_quantile(mirror_view(), ct, cr, m, t, static_cast<int>(leaf0), static_cast<int>(NL), d_pred, d_targets, abs_index, d_alpha, plan, scratch, dres, s);
    lq_host_.resize(words);
    hip_check(hipGetLastError(), "quantile_leaves kernels");
    read_back(lq_host_.data(), dres, sizeof(uint32_t) * words, "D2H leaf quantiles", "quantile_leaves");
    if (timed) join_tail_phase("quantile_leaves", "quantile_select", plan.select);   // (1 = the select path took the call)
    const uint32_t *keys = lq_host_.data(), *ranks = keys + nld, *counts = ranks + nld;
    const uint32_t flag = counts[NL];
    if (flag & kern::kQuantileBadTarget) throw InvalidArgument(std::string(what) + ": a target is not finite: no quantile leaf values; the model is unchanged");
    if (flag & kern::kQuantileBadPred) throw InvalidArgument(std::string(what) + ": a prediction is not finite: no quantile leaf values; the model is unchanged");
    if (flag & kern::kQuantileBadResidual)
        throw InvalidArgument(std::string(what) + ": a residual fl32(prediction - target) is not finite: no quantile leaf values; the model is unchanged");
    for (size_t l = 0; l < NL; ++l) {
        if (counts[l] == 0 || model.leaf_depth(t, l) <= 0) continue;   // (newton_core.h's rule: such a leaf keeps the value the step gave it)
        float *v = model.values.data() + (leaf0 + l) * D;
        for (int d = 0; d < D; ++d) v[d] = kern::quantile_key_value(keys[l * D + d]);
    }
    ++model.version;
    rewind_values(t);
    if (values_out) std::memcpy(values_out, model.values.data() + leaf0 * D, sizeof(float) * nld);
    if (counts_out) for (size_t l = 0; l < NL; ++l) counts_out[l] = counts[l];
    if (ranks_out) for (size_t i = 0; i < nld; ++i) ranks_out[i] = ranks[i];
}

void Engine::quantile_leaves_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *pred, bool pred_dev, const float *targets,
                                      bool targets_dev, const float *alpha, int tree, float *values_out, int64_t *counts_out, int64_t *ranks_out) {
    const gbrl_hip_metadata &md = model.meta;
    const int D = md.output_dim;
    check_prepared_dataset("quantile_leaves_prepared", ds);
    if (D > 128) throw Unsupported("quantile_leaves_prepared: output_dim > 128");
    if (pred == nullptr) throw InvalidArgument("quantile_leaves_prepared: no prediction");
    if (targets == nullptr) throw InvalidArgument("Cannot call quantile_leaves_prepared without targets!");
    check_alpha("quantile_leaves_prepared", kern::kObjQuantile, alpha, D, false);
    const int t = resolve_tree("quantile_leaves_prepared", tree);
    check_row_count("quantile_leaves_prepared", "pred", rows, m, ds->n, "select over");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, "quantile_leaves_prepared", t, t + 1);
    ensure_device();
    reset_events();
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const size_t n_el = static_cast<size_t>(m) * D;
    const float *dp = staged(d_obj_pred_, pred, pred_dev, n_el, "H2D predictions");
    const float *dt = staged(d_obj_targets_, targets, targets_dev, n_el, "H2D targets");
    const float *da = upload(d_lq_alpha_, alpha, static_cast<size_t>(D), "H2D levels");
    quantile_leaves_run("quantile_leaves_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, dp, dt, /*abs_index=*/false, da, t,
                        hooks::on(hooks::CONTINUE_GENERIC), values_out, counts_out, ranks_out);
}

void Engine::newton_leaves_prepared_rank(const PreparedDataset *ds, const float *pred, bool pred_dev, const int32_t *labels, bool labels_dev, const int32_t *group,
                                         int n_groups, int objective, int ndcg_at, int tree, double leaf_l2, int64_t *sums_out, int *bits_out, float *values_out) {
    const char *what = "newton_leaves_prepared";
    const gbrl_hip_metadata &md = model.meta;
    check_prepared_dataset(what, ds);
    if (pred == nullptr) throw InvalidArgument("newton_leaves_prepared: no prediction");
    if (labels == nullptr) throw InvalidArgument("Cannot call newton_leaves_prepared without targets!");
    const int n = ds->n;
    check_rank_group(what, group, n_groups, n, objective, ndcg_at, md.output_dim);
    check_leaf_update(what, kern::kObjLogistic, kern::kLeafNewton, leaf_l2);   // (a bad leaf_l2)
    const int t = resolve_tree(what, tree);
    check_code_range(*ds, what, t, t + 1);
    ensure_device();
    reset_events();
    const float *dp = staged(d_rk_pred_, pred, pred_dev, static_cast<size_t>(n), "H2D scores");
    const int32_t *dl = staged(d_rk_labels_, labels, labels_dev, static_cast<size_t>(n), "H2D labels");
    RankSet &set = rk_sets_[0];
    rank_prepare(what, set, dl, group, n_groups, n, ndcg_at);
    float *dg = static_cast<float *>(d_rk_grad_.ensure(sizeof(float) * n)), *dh = static_cast<float *>(d_rk_hess_.ensure(sizeof(float) * n));
    rank_eval(set, objective, ndcg_at, dp, dl, nullptr, dg, dh, false, nullptr, nullptr, nullptr);
    hip_check(hipGetLastError(), "newton_leaves_prepared rank kernels");
    unsigned long long flag = 0;
    read_back(&flag, d_rk_stat_.as<unsigned long long>(), sizeof(flag), "D2H rank flags");
    if (flag & kern::kRankBadPred) throw InvalidArgument("newton_leaves_prepared: a prediction is not finite: no newton leaf values; the model is unchanged");
    newton_leaves_run(what, ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), nullptr, 0}, n, dg, dh, /*abs_index=*/false, kern::kObjGiven, t, leaf_l2,
                      hooks::on(hooks::CONTINUE_GENERIC), sums_out, bits_out, values_out, nullptr, static_cast<float>(set.max_group));
}

}  // namespace gbrl
