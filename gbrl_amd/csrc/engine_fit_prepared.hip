// engine_fit_prepared.hip -- the walk over a prepared data set's bin codes, from the host rule up to the two public calls:
//   Engine::condition_bins             every numeric condition of the model as a bin index of a threshold table (host only)
//   sync_code_bins / check_code_range  the same for ONE data set, appended split row by split row, and the refusal of a range the codes cannot express
//   sync_code_tables                   device copies of the bins and of the mirror's packed conditions / greedy node records with the bin as
//                                      their second word (appended like the originals: a loop that adds a tree per iteration converts that tree only)
//   Engine::predict_continue_prepared  predict_continue without the observations (kern::predict_continue_codes)
//   Engine::objective_gradient[_host]  the gradient and the loss of an objective (objective_core.h) for a prediction matrix, on the device and on the host
//   Engine::fit_prepared               fit()'s loop with the running prediction held and the batch never binned again (advance_held: the code walk
//                                      with its gradient tail), in named stages over one FitRun.  Its options: an objective in place of MultiRMSE;
//                                      a validation set that shares the thresholds -- a second held prediction advanced after every iteration by
//                                      the walk's loss tail, Engine::early_stop_scan's rule; every tree grown on a sample of its batch
//                                      (sample_core.h: kern::sample_rows draws the rows and gathers their gradient rows in one pass, 4 bytes come
//                                      back, step_prepared's body grows on the subset) and on a sample of the columns (the host rule of
//                                      sample_core.h per iteration, step_prepared's cols path); a classifier's metric of the validation rows
//                                      per iteration, which then decides the stopping rule and best_n_trees in place of the loss
//                                      ; with goss the row draw is kern::goss_select + kern::goss_sample_passes (one-side sampling: the largest
//                                      gradients and an amplified draw of the rest; tau stays on the device) in place of kern::sample_rows
//                                      ; with a ranking objective (rank_core.h; engine_rank.hip) the walk runs without a gradient tail, the rank
//                                      kernels write the gradient (and hessian) of every row from the rows of its query, newton leaves take their
//                                      sums from those buffers, and both losses come from the same kernels
//   Engine::newton_leaves_prepared     one tree's leaves set to sum g / (sum h + leaf_l2) over a data set's rows (newton_core.h; kern::newton_leaf_sums), the
//                                      rules on the host beside it (objective_hessian_host, newton_values_host); fit_prepared(leaf_update = newton) runs its
//                                      body after every step
//   Engine::quantile_leaves_prepared   one tree's leaves set to the level's order statistic of the residuals of their rows (quantile_core.h; kern::leaf_quantile),
//                                      the rule on the host beside it (leaf_quantile_host, quantile_rank); fit_prepared(leaf_update = quantile) runs its body
//                                      after every step, and objective = quantile adds the pinball gradient and loss to the tails
//   Engine::check_weights[_host]       row weights (objective_core.h, newton_core.h): a weight vector's refusals, its maximum and its float64 sum in a fixed order
//                                      (kern::weight_stats), once per call and vector; the weighted forms of the gradient, the loss, the bias and the Newton
//                                      sums ride in the launches above as one more per-row operand
//   Engine::eval_metric[_host]         the error rate and the exact AUC of a prediction matrix (metric_core.h), on the device and on the host
//
// The rule.  code(r, f) = #{b : thr[f][b] < obs[r, f]} (-0.0 == +0.0; NaN lies below every threshold: code 0).  For a condition x > v whose v
// equals some thr[f][b] let bin = #{b : thr[f][b] < v}.  x > v: every threshold below v, and v itself, is below x, so code >= bin + 1.
// x <= v: only thresholds below v can be below x, so code <= bin.  Hence x > v <=> code > bin, with duplicated thresholds and in any order.
// It does not hold for a v that is not among the feature's thresholds: such a condition is refused (Unsupported), never approximated.
#include "engine_step_detail.h"
#include "objective_core.h"
#include "metric_core.h"
#include "newton_core.h"
#include "quantile_core.h"
#include "rank_core.h"
#include "sample_core.h"

namespace gbrl {

namespace {

constexpr int32_t kBinUnused = -1, kBinInexpressible = -2;

int32_t bin_of(const float *thr, int B, float v) {
    int32_t below = 0;
    bool found = false;
    for (int b = 0; b < B; ++b) {
        below += thr[b] < v ? 1 : 0;
        found = found || thr[b] == v;   // (NaN equals nothing)
    }
    return found ? below : kBinInexpressible;
}

int tree_of_split_row(const Model &model, size_t s) {
    if (model.oblivious()) return static_cast<int>(s);
    const auto it = std::upper_bound(model.tree_indices.begin(), model.tree_indices.end(), static_cast<int32_t>(s));
    return static_cast<int>(it - model.tree_indices.begin()) - 1;
}

std::string inexpressible_message(const Model &model, const char *what, size_t s, int d) {
    const size_t c = s * static_cast<size_t>(model.meta.max_depth) + d;
    return std::string(what) + ": tree " + std::to_string(tree_of_split_row(model, s)) + ", condition " + std::to_string(d) + " (feature " +
           std::to_string(model.feature_indices[c]) + " > " + std::to_string(model.feature_values[c]) +
           ") does not compare against one of the data set's thresholds of that feature: the bin codes cannot express it";
}

// greedy: a tree of one leaf -- the walk of such a tree finds no leaf of its own and runs on into the next tree (Q7)
bool runs_on(const Model &model, int t) {
    if (model.oblivious()) return false;
    const int T = model.meta.n_trees;
    const int l0 = model.tree_indices[t], l1 = t + 1 < T ? model.tree_indices[t + 1] : model.meta.n_leaves;
    return l1 - l0 == 1;
}

}  // namespace

void Engine::condition_bins(const float *thresholds, int F, int B, int32_t *out) const {
    const gbrl_hip_metadata &md = model.meta;
    if (thresholds == nullptr || out == nullptr) throw InvalidArgument("condition_bins: null argument");
    const int want_f = md.iteration > 0 ? md.n_num_features : md.input_dim;
    if (F != want_f) throw InvalidArgument("condition_bins: thresholds of " + std::to_string(F) + " features, the model has " + std::to_string(want_f) + " numeric features");
    if (B != md.n_bins) throw InvalidArgument("condition_bins: " + std::to_string(B) + " thresholds per feature, the model has n_bins = " + std::to_string(md.n_bins));
    const size_t S = model.split_rows(), MD = md.max_depth;
    std::fill(out, out + S * MD, kBinUnused);
    for (size_t s = 0; s < S; ++s)
        for (int d = 0; d < model.depths[s] && d < static_cast<int>(MD); ++d) {
            const size_t c = s * MD + d;
            if (!model.is_numerics[c]) continue;
            const int f = model.feature_indices[c];
            const int32_t bin = (f >= 0 && f < F) ? bin_of(thresholds + static_cast<size_t>(f) * B, B, model.feature_values[c]) : kBinInexpressible;
            if (bin == kBinInexpressible) throw Unsupported(inexpressible_message(model, "condition_bins", s, d));
            out[c] = bin;
        }
}

void Engine::sync_code_bins(const PreparedDataset &ds) {
    const size_t S = model.split_rows(), MD = model.meta.max_depth;
    if (code_ds_id_ != ds.thresholds_id || code_splits_ > S) {   // other thresholds, or the ensemble has shrunk: nothing of the tables is kept
        code_ds_id_ = ds.thresholds_id;
        code_splits_ = code_up_splits_ = code_nodes_ = code_up_nodes_ = 0;
        code_bins_host_.clear(); code_pack_host_.clear(); code_nodes_host_.clear();
    }
    code_bins_host_.resize(S * MD, kBinUnused);
    const int F = ds.F, B = ds.n_bins;
    for (size_t s = code_splits_; s < S; ++s)
        for (size_t d = 0; d < MD; ++d) {
            const size_t c = s * MD + d;
            int32_t bin = kBinUnused;
            if (static_cast<int>(d) < model.depths[s] && model.is_numerics[c]) {
                const int f = model.feature_indices[c];
                bin = (f >= 0 && f < F) ? bin_of(ds.h_thr.data() + static_cast<size_t>(f) * B, B, model.feature_values[c]) : kBinInexpressible;
            }
            code_bins_host_[c] = bin;
        }
    code_splits_ = S;
}

void Engine::check_code_range(const PreparedDataset &ds, const char *what, int start_tree, int stop_tree) {
    sync_code_bins(ds);
    const int T = model.meta.n_trees;
    const size_t MD = model.meta.max_depth;
    if (stop_tree <= start_tree) return;
    int end = stop_tree;
    while (end < T && runs_on(model, end - 1)) ++end;   // the walk of a trailing one-leaf greedy tree reads the conditions of the trees behind it
    const size_t s0 = model.oblivious() ? static_cast<size_t>(start_tree) : static_cast<size_t>(model.tree_indices[start_tree]);
    const size_t s1 = model.oblivious() ? static_cast<size_t>(end) : static_cast<size_t>(end < T ? model.tree_indices[end] : model.meta.n_leaves);
    for (size_t s = s0; s < s1; ++s)
        for (size_t d = 0; d < MD; ++d)
            if (code_bins_host_[s * MD + d] == kBinInexpressible) throw Unsupported(inexpressible_message(model, what, s, static_cast<int>(d)));
}

kern::CodeTables Engine::sync_code_tables(const PreparedDataset &ds) {
    sync_code_bins(ds);
    hipStream_t s = stream_;
    const size_t S = model.split_rows(), MD = model.meta.max_depth;
    constexpr int32_t kNever = 0x7fffffff;   // no u16 code is above it (such a condition is refused before a kernel could read it)
    bool sent = false;
    auto append = [&](DevBuf &buf, const std::vector<int32_t> &host, size_t old_n, size_t new_n) {
        char *p = static_cast<char *>(buf.ensure_keep(std::max<size_t>(new_n, 1) * 4, old_n * 4, s));
        if (new_n > old_n) {
            hip_check(hipMemcpyAsync(p + old_n * 4, host.data() + old_n, (new_n - old_n) * 4, hipMemcpyHostToDevice, s), "H2D code tables");
            sent = true;
        }
    };
    // the packed conditions of the mirror (cond_pack_host_, built by sync_model_to_device) with the threshold word replaced by the bin
    code_pack_host_.resize(S * MD * 2, 0);
    for (size_t c = code_up_splits_ * MD; c < S * MD; ++c) {
        code_pack_host_[2 * c] = cond_pack_host_[2 * c];
        const int32_t bin = code_bins_host_[c];
        code_pack_host_[2 * c + 1] = model.is_numerics[c] ? (bin == kBinInexpressible ? kNever : bin) : cond_pack_host_[2 * c + 1];
    }
    append(m_code_bins_, code_bins_host_, code_up_splits_ * MD, S * MD);
    append(m_code_pack_, code_pack_host_, code_up_splits_ * MD * 2, S * MD * 2);
    code_up_splits_ = S;
    // the greedy node records likewise (same offsets: grd_node_off is the mirror's)
    if (!model.oblivious()) {
        const size_t n_nodes = grd_nodes_host_.size() / 4;
        if (code_nodes_ > n_nodes) code_nodes_ = code_up_nodes_ = 0;
        code_nodes_host_.resize(n_nodes * 4);
        for (size_t k = code_nodes_; k < n_nodes; ++k) {
            int32_t *nd = &code_nodes_host_[k * 4];
            std::memcpy(nd, &grd_nodes_host_[k * 4], 16);
            if (nd[0] >= 0) {
                float v;
                std::memcpy(&v, &nd[1], sizeof(v));
                const int32_t bin = nd[0] < ds.F ? bin_of(ds.h_thr.data() + static_cast<size_t>(nd[0]) * ds.n_bins, ds.n_bins, v) : kBinInexpressible;
                nd[1] = bin == kBinInexpressible ? kNever : bin;
            }
        }
        code_nodes_ = n_nodes;
        append(m_code_nodes_, code_nodes_host_, code_up_nodes_ * 4, n_nodes * 4);
        code_up_nodes_ = n_nodes;
    }
    if (sent) hip_check(hipStreamSynchronize(s), "sync code tables");   // the host vectors may grow (and move) before the next call
    return kern::CodeTables{m_code_bins_.as<int32_t>(), m_code_pack_.as<int32_t>(), m_code_nodes_.as<int32_t>()};
}

void Engine::predict_continue_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *base, bool base_dev, int start_tree,
                                       int stop_tree, float *out, bool out_dev) {
    const gbrl_hip_metadata &md = model.meta;
    check_prepared_dataset("predict_continue_prepared", ds);
    if (md.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    if (out == nullptr) throw InvalidArgument("predict_continue_prepared: no place for the result");
    if (base == nullptr) throw InvalidArgument("predict_continue_prepared: no base prediction");
    if (start_tree < 0 || stop_tree < 0) throw InvalidArgument("invalid tree range");
    const int stop = stop_tree == 0 ? md.n_trees : stop_tree;   // (0 means n_trees)
    if (stop > md.n_trees || start_tree > stop) throw InvalidArgument("predict_continue_prepared: invalid tree range");
    if (m <= 0) throw InvalidArgument("predict_continue_prepared: no rows (m must be positive)");
    if (rows == nullptr && m != ds->n)
        throw InvalidArgument("predict_continue_prepared: base has " + std::to_string(m) + " rows, the data set " + std::to_string(ds->n) + " (pass rows to continue a subset)");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, "predict_continue_prepared", start_tree, stop);
    ensure_device();
    ev_used_ = 0;
    ev_names_.clear();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = rows ? checked_rows(d_sub_rows_, d_rows_mm_, rows, rows_dev, m, ds->n, stream_) : nullptr;
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(m) * md.output_dim;
    float *dout = out_dev ? out : static_cast<float *>(d_pout_.ensure(out_bytes));
    const float *dbase = base;
    if (!base_dev) {   // a base in host memory is copied into the output buffer and continued in place
        hip_check(hipMemcpyAsync(dout, base, out_bytes, hipMemcpyHostToDevice, stream_), "H2D base");
        dbase = dout;
    }
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::predict_continue_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, start_tree, stop, dbase, dout,
                                 nullptr, nullptr, nullptr, nullptr, hooks::on(hooks::CONTINUE_GENERIC), stream_);
    finish("predict_continue_prepared launch", "predict", {{out_dev ? nullptr : out, dout, out_bytes, "D2H preds"}});
}

// ---- objectives: the checks, the gradient rule on the host, the gradient and the loss of a prediction matrix on the device
void Engine::check_objective(const char *what, int objective, int D) {
    if (kern::rank_objective(objective))
        throw InvalidArgument(std::string(what) + ": the ranking objectives (pairwise = 4, lambdarank = 5) sum over the rows of a query, which this call does not know: " +
                              "rank_gradient takes them with group");
    if (objective != kern::kObjRmse && objective != kern::kObjLogistic && objective != kern::kObjSoftmax && objective != kern::kObjQuantile)
        throw InvalidArgument(std::string(what) + ": unknown objective " + std::to_string(objective) + " (rmse = 0, logistic = 1, softmax = 2, quantile = 3)");
    if (objective == kern::kObjSoftmax && D < 2)
        throw InvalidArgument(std::string(what) + ": the softmax objective needs output_dim >= 2, the model has " + std::to_string(D));
}

void Engine::check_alpha(const char *what, int objective, const float *alpha, int D, bool weighted) {
    if (objective != kern::kObjQuantile) {
        if (alpha != nullptr) throw InvalidArgument(std::string(what) + ": alpha is the level table of the quantile objective; this objective takes none");
        return;
    }
    if (alpha == nullptr) throw InvalidArgument(std::string(what) + ": the quantile objective needs alpha, one level per output");
    for (int d = 0; d < D; ++d)
        if (kern::quantile_bad_level(alpha[d]))
            throw InvalidArgument(std::string(what) + ": alpha[" + std::to_string(d) + "] = " + std::to_string(alpha[d]) + " (output " + std::to_string(d) +
                                  ") is not a finite level strictly inside (0, 1)");
    if (weighted) throw Unsupported(std::string(what) + ": row weights with the quantile objective are not supported (bias and leaves would need a weighted quantile)");
}

void Engine::check_labels(const char *what, const int32_t *d_labels, int n, int D, std::vector<int32_t> *counts) {
    hipStream_t s = stream_;
    std::vector<int32_t> h(static_cast<size_t>(D) + 1, 0);
    h[D] = 0x7fffffff;
    int32_t *d = upload(d_obj_counts_, h.data(), h.size(), "H2D label counts");
    kern::label_counts(d_labels, n, D, d, s);
    hip_check(hipMemcpyAsync(h.data(), d, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, s), "D2H label counts");
    hip_check(hipStreamSynchronize(s), "sync");
    if (h[D] != 0x7fffffff) {
        int32_t bad = 0;
        hip_check(hipMemcpyAsync(&bad, d_labels + h[D], sizeof(bad), hipMemcpyDeviceToHost, s), "D2H label");
        hip_check(hipStreamSynchronize(s), "sync");
        throw InvalidArgument(std::string(what) + ": label " + std::to_string(bad) + " (row " + std::to_string(h[D]) + ") is outside [0, " + std::to_string(D) + ")");
    }
    if (counts) counts->assign(h.begin(), h.begin() + D);
}

void Engine::check_weights_host(const char *what, const float *weights, int n) {
    for (int r = 0; r < n; ++r)
        if (kern::obj_weight_bad(weights[r]))
            throw InvalidArgument(std::string(what) + ": weight " + std::to_string(weights[r]) + " (row " + std::to_string(r) + ") is not a finite number in [0, 65536]");
}

Engine::WeightStats Engine::check_weights(const char *what, const float *d_weights, int n, bool need_sum) {
    hipStream_t s = stream_;
    int32_t h[2] = {0x7fffffff, 0};
    int32_t *d = upload(d_wstat_, h, 2, "H2D weight statistics");
    double *d_part = static_cast<double *>(d_wpart_.ensure(sizeof(double) * kern::staged_loss_partials(n)));
    double *d_sum = static_cast<double *>(d_wsum_.ensure(sizeof(double)));
    kern::weight_stats(d_weights, n, d, d_part, d_sum, s);
    WeightStats st;
    hip_check(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s), "D2H weight statistics");
    hip_check(hipMemcpyAsync(&st.sum, d_sum, sizeof(double), hipMemcpyDeviceToHost, s), "D2H weight sum");
    hip_check(hipStreamSynchronize(s), "sync");
    if (h[0] != 0x7fffffff) {
        float bad = 0.0f;
        hip_check(hipMemcpyAsync(&bad, d_weights + h[0], sizeof(bad), hipMemcpyDeviceToHost, s), "D2H weight");
        hip_check(hipStreamSynchronize(s), "sync");
        throw InvalidArgument(std::string(what) + ": weight " + std::to_string(bad) + " (row " + std::to_string(h[0]) + ") is not a finite number in [0, 65536]");
    }
    std::memcpy(&st.max, &h[1], sizeof(float));
    if (need_sum && !(st.sum > 0.0)) throw InvalidArgument(std::string(what) + ": the weights sum to 0: no weighted loss or bias is defined");
    return st;
}

namespace {
void weigh_rows(float *x, const float *weights, int n, int D) {
    for (int r = 0; r < n; ++r)
        for (int d = 0; d < D; ++d) x[static_cast<size_t>(r) * D + d] = kern::obj_weighted(weights[r], x[static_cast<size_t>(r) * D + d]);
}
}  // namespace

void Engine::objective_gradient_host(const float *pred, const void *targets, int n, int D, int objective, float *grad_out, const float *weights, const float *alpha) {
    if (pred == nullptr || targets == nullptr || grad_out == nullptr) throw InvalidArgument("objective_gradient_host: null argument");
    if (n <= 0) throw InvalidArgument("objective_gradient_host: no rows (n must be positive)");
    if (D < 1) throw InvalidArgument("objective_gradient_host: output_dim must be positive");
    check_objective("objective_gradient_host", objective, D);
    check_alpha("objective_gradient_host", objective, alpha, D, weights != nullptr);
    if (weights) check_weights_host("objective_gradient_host", weights, n);
    const size_t n_el = static_cast<size_t>(n) * D;
    if (objective == kern::kObjQuantile) {
        const float *y = static_cast<const float *>(targets);
        for (size_t i = 0; i < n_el; ++i) grad_out[i] = kern::obj_quantile_grad(pred[i], y[i], alpha[i % D]);
        return;
    }
    if (objective == kern::kObjSoftmax) {
        const int32_t *labels = static_cast<const int32_t *>(targets);
        for (int r = 0; r < n; ++r)
            if (labels[r] < 0 || labels[r] >= D)
                throw InvalidArgument("objective_gradient_host: label " + std::to_string(labels[r]) + " (row " + std::to_string(r) + ") is outside [0, " + std::to_string(D) + ")");
        if (grad_out != pred) std::memmove(grad_out, pred, sizeof(float) * n_el);
        for (int r = 0; r < n; ++r) {
            float *row = grad_out + static_cast<size_t>(r) * D;
            kern::obj_softmax_grad_row(row, D, labels[r]);
        }
        if (weights) weigh_rows(grad_out, weights, n, D);
        return;
    }
    const float *y = static_cast<const float *>(targets);
    if (objective == kern::kObjLogistic)
        for (size_t i = 0; i < n_el; ++i) grad_out[i] = kern::obj_logistic_grad(pred[i], y[i]);
    else
        for (size_t i = 0; i < n_el; ++i) grad_out[i] = pred[i] - y[i];
    if (weights) weigh_rows(grad_out, weights, n, D);
}

namespace {
// the mean loss of an objective from the sum of its row losses: rmse is staged_loss's expression
// (rows: the row count, or with weights their float64 sum W)
double mean_loss(int objective, double sum, double rows) { return objective == kern::kObjRmse ? std::sqrt(0.5 * sum / rows) : sum / rows; }
}  // namespace

void Engine::finish_loss_sum(const double *d_part, int n_part, double *d_sum, double *host_sum) {
    kern::staged_loss_finish(d_part, n_part, d_sum, stream_);
    if (host_sum) hip_check(hipMemcpyAsync(host_sum, d_sum, sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H loss");
}

void Engine::objective_gradient(const float *pred, bool pred_dev, const void *targets, bool targets_dev, int n, int objective, float *grad_out, double *loss_out,
                                const float *weights, bool weights_dev, const float *alpha) {
    const int D = model.meta.output_dim;
    if (pred == nullptr || targets == nullptr) throw InvalidArgument("objective_gradient: null argument");
    if (grad_out == nullptr && loss_out == nullptr) throw InvalidArgument("objective_gradient: no place for a result");
    if (n <= 0) throw InvalidArgument("objective_gradient: no rows (n must be positive)");
    if (D > 128) throw Unsupported("objective_gradient: output_dim > 128");
    check_objective("objective_gradient", objective, D);
    check_alpha("objective_gradient", objective, alpha, D, weights != nullptr);
    ensure_device();
    hipStream_t s = stream_;
    const size_t n_el = static_cast<size_t>(n) * D, tar_el = objective == kern::kObjSoftmax ? static_cast<size_t>(n) : n_el;
    const float *dp = pred_dev ? pred : upload(d_obj_pred_, pred, n_el, "H2D predictions");
    const float *dt = targets_dev ? static_cast<const float *>(targets) : upload(d_obj_targets_, static_cast<const float *>(targets), tar_el, "H2D targets");
    if (objective == kern::kObjSoftmax) check_labels("objective_gradient", reinterpret_cast<const int32_t *>(dt), n, D, nullptr);
    const float *dw = weights == nullptr ? nullptr : (weights_dev ? weights : upload(d_obj_weights_, weights, static_cast<size_t>(n), "H2D weights"));
    const double rows = dw ? check_weights("objective_gradient", dw, n, true).sum : static_cast<double>(n);
    float *dg = grad_out == nullptr ? nullptr : (pred_dev ? grad_out : static_cast<float *>(d_obj_grad_.ensure(sizeof(float) * n_el)));
    const int nb = kern::staged_loss_partials(n);
    double *dpart = loss_out ? static_cast<double *>(d_obj_part_.ensure(sizeof(double) * nb)) : nullptr;
    double *dsum = loss_out ? static_cast<double *>(d_obj_sum_.ensure(sizeof(double))) : nullptr;
    const float *da = alpha ? upload(d_lq_alpha_, alpha, static_cast<size_t>(D), "H2D levels") : nullptr;
    kern::objective_rows(objective, dp, dt, n, D, dg, dpart, s, dw, da);
    double sum = 0.0;
    if (loss_out) finish_loss_sum(dpart, nb, dsum, &sum);
    if (grad_out && !pred_dev) hip_check(hipMemcpyAsync(grad_out, dg, sizeof(float) * n_el, hipMemcpyDeviceToHost, s), "D2H gradient");
    hip_check(hipGetLastError(), "objective_gradient kernels");
    hip_check(hipStreamSynchronize(s), "sync");
    if (loss_out) *loss_out = mean_loss(objective, sum, rows);
}

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

void Engine::objective_hessian_host(const float *pred, int n, int D, int objective, float *hess_out, const float *weights) {
    if (pred == nullptr || hess_out == nullptr) throw InvalidArgument("objective_hessian_host: null argument");
    if (n <= 0) throw InvalidArgument("objective_hessian_host: no rows (n must be positive)");
    if (D < 1) throw InvalidArgument("objective_hessian_host: output_dim must be positive");
    check_objective("objective_hessian_host", objective, D);
    if (objective == kern::kObjQuantile)
        throw InvalidArgument("objective_hessian_host: the quantile objective has no hessian to offer (it is zero); its leaf step is leaf_update = quantile");
    if (weights) check_weights_host("objective_hessian_host", weights, n);
    const size_t n_el = static_cast<size_t>(n) * D;
    if (objective == kern::kObjRmse) {
        std::fill(hess_out, hess_out + n_el, 1.0f);
    } else if (objective == kern::kObjLogistic) {
        for (size_t i = 0; i < n_el; ++i) hess_out[i] = kern::obj_logistic_hess(pred[i]);
    } else {
        std::vector<float> row(D);
        for (int r = 0; r < n; ++r) {
            std::copy(pred + static_cast<size_t>(r) * D, pred + static_cast<size_t>(r + 1) * D, row.begin());
            float *h = hess_out + static_cast<size_t>(r) * D;
            kern::obj_softmax_grad_hess_row(row, h, D, 0);
        }
    }
    if (weights) weigh_rows(hess_out, weights, n, D);
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
    const int D = md.output_dim, T = md.n_trees;
    const size_t leaf0 = static_cast<size_t>(model.tree_indices[t]);
    const size_t NL = (t + 1 < T ? static_cast<size_t>(model.tree_indices[t + 1]) : static_cast<size_t>(md.n_leaves)) - leaf0;
    const size_t W = 2 * static_cast<size_t>(D) + 1, words = NL * W + 1;
    check_code_range(*ds, what, t, t + 1);
    sync_model_to_device();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const bool timed = profiling_ >= 2;
    phase_begin();
    unsigned long long *dacc = static_cast<unsigned long long *>(d_newton_acc_.ensure(sizeof(unsigned long long) * words));
    hip_check(hipMemsetAsync(dacc, 0, sizeof(unsigned long long) * words, s), "zero leaf sums");
    // (kObjGiven: a ranking objective's g and h from buffers, below the largest query's size, which arrives as weight_max)
    const int bits = d_weights || objective == kern::kObjGiven ? kern::newton_sum_bits(m, weight_max) : kern::newton_sum_bits(m);
    const bool streamed = kern::newton_leaf_sums(mirror_view(), ct, cr, m, t, static_cast<int>(leaf0), static_cast<int>(NL), d_pred, d_targets, abs_index, objective,
                                                 bits, dacc, generic, s, d_weights);
    newton_host_.resize(words);
    hip_check(hipMemcpyAsync(newton_host_.data(), dacc, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, s), "D2H leaf sums");
    phase_end("newton_leaves");
    hip_check(hipStreamSynchronize(s), "sync");
    if (timed) {   // the phase joins the list the caller's phases are in (a step's list has been resolved already)
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, ev_pool_[ev_used_ - 1].first, ev_pool_[ev_used_ - 1].second), "hipEventElapsedTime");
        --ev_used_;
        ev_names_.pop_back();
        phases_.emplace_back("newton_leaves", ms);
        phases_.emplace_back("newton_streamed", streamed ? 1.f : 0.f);   // (not a time: 1 = the streaming kernel took the sums)
    }
    const unsigned long long flag = newton_host_[words - 1];
    if (flag & kern::kNewtonBadTarget)
        throw InvalidArgument(std::string(what) + ": a logistic target is outside [0, 1] (or NaN): newton leaf values need targets in [0, 1]; the model is unchanged");
    if (flag & kern::kNewtonBadPred)
        throw InvalidArgument(std::string(what) + ": a prediction is not finite: no newton leaf values; the model is unchanged");
    const double scale = std::ldexp(1.0, bits);
    for (size_t l = 0; l < NL; ++l) {
        const long long *a = reinterpret_cast<const long long *>(newton_host_.data()) + l * W;
        const int depth = model.oblivious() ? model.depths[t] : model.depths[leaf0 + l];
        float *v = model.values.data() + (leaf0 + l) * D;
        for (int d = 0; d < D; ++d) v[d] = kern::newton_leaf_value(a[d], a[D + d], a[2 * D], depth, scale, leaf_l2, v[d]);
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
    const int D = md.output_dim, T = md.n_trees;
    check_prepared_dataset("newton_leaves_prepared", ds);
    if (D > 128) throw Unsupported("newton_leaves_prepared: output_dim > 128");
    if (pred == nullptr) throw InvalidArgument("newton_leaves_prepared: no prediction");
    if (targets == nullptr) throw InvalidArgument("Cannot call newton_leaves_prepared without targets!");
    check_objective("newton_leaves_prepared", objective, D);
    check_leaf_update("newton_leaves_prepared", objective, kern::kLeafNewton, leaf_l2);
    if (T == 0) throw InvalidArgument("newton_leaves_prepared: the model has no trees");
    if (tree < -1 || tree >= T) throw InvalidArgument("newton_leaves_prepared: tree " + std::to_string(tree) + " is outside the model's " + std::to_string(T) + " trees (-1: the last)");
    const int t = tree == -1 ? T - 1 : tree;
    if (m <= 0) throw InvalidArgument("newton_leaves_prepared: no rows (m must be positive)");
    if (rows == nullptr && m != ds->n)
        throw InvalidArgument("newton_leaves_prepared: pred has " + std::to_string(m) + " rows, the data set " + std::to_string(ds->n) + " (pass rows to sum over a subset)");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    if (weights == nullptr && weight_max >= 0.0f) throw InvalidArgument("newton_leaves_prepared: weight_max needs weights");
    if (weights != nullptr && (weight_max != weight_max || weight_max > kern::kWeightMax))
        throw InvalidArgument("newton_leaves_prepared: weight_max must be at most 65536 (and not NaN), got " + std::to_string(weight_max));
    check_code_range(*ds, "newton_leaves_prepared", t, t + 1);
    ensure_device();
    ev_used_ = 0;
    ev_names_.clear();
    phases_.clear();
    hipStream_t s = stream_;
    const int32_t *d_rows = rows ? checked_rows(d_sub_rows_, d_rows_mm_, rows, rows_dev, m, ds->n, s) : nullptr;
    const size_t n_el = static_cast<size_t>(m) * D, tar_el = objective == kern::kObjSoftmax ? static_cast<size_t>(m) : n_el;
    const float *dp = pred_dev ? pred : upload(d_obj_pred_, pred, n_el, "H2D predictions");
    const float *dt = targets_dev ? static_cast<const float *>(targets) : upload(d_obj_targets_, static_cast<const float *>(targets), tar_el, "H2D targets");
    if (objective == kern::kObjSoftmax) check_labels("newton_leaves_prepared", reinterpret_cast<const int32_t *>(dt), m, D, nullptr);
    const float *dw = weights == nullptr ? nullptr : (weights_dev ? weights : upload(d_obj_weights_, weights, static_cast<size_t>(m), "H2D weights"));
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
    const int D = md.output_dim, T = md.n_trees;
    const size_t leaf0 = static_cast<size_t>(model.tree_indices[t]);
    const size_t NL = (t + 1 < T ? static_cast<size_t>(model.tree_indices[t + 1]) : static_cast<size_t>(md.n_leaves)) - leaf0;
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
    uint32_t *dres = static_cast<uint32_t *>(d_lq_res_.ensure(sizeof(uint32_t) * words));
    void *scratch = d_lq_scratch_.ensure(plan.scratch_bytes);
    hip_check(hipMemsetAsync(dres, 0, sizeof(uint32_t) * words, s), "zero leaf quantiles");
    kern::leaf_quantile(mirror_view(), ct, cr, m, t, static_cast<int>(leaf0), static_cast<int>(NL), d_pred, d_targets, abs_index, d_alpha, plan, scratch, dres, s);
    lq_host_.resize(words);
    hip_check(hipMemcpyAsync(lq_host_.data(), dres, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, s), "D2H leaf quantiles");
    phase_end("quantile_leaves");
    hip_check(hipGetLastError(), "quantile_leaves kernels");
    hip_check(hipStreamSynchronize(s), "sync");
    if (timed) {   // the phase joins the list the caller's phases are in (a step's list has been resolved already)
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, ev_pool_[ev_used_ - 1].first, ev_pool_[ev_used_ - 1].second), "hipEventElapsedTime");
        --ev_used_;
        ev_names_.pop_back();
        phases_.emplace_back("quantile_leaves", ms);
        phases_.emplace_back("quantile_select", plan.select ? 1.f : 0.f);   // (not a time: 1 = the select path took the call)
    }
    const uint32_t *keys = lq_host_.data(), *ranks = keys + nld, *counts = ranks + nld;
    const uint32_t flag = counts[NL];
    if (flag & kern::kQuantileBadTarget) throw InvalidArgument(std::string(what) + ": a target is not finite: no quantile leaf values; the model is unchanged");
    if (flag & kern::kQuantileBadPred) throw InvalidArgument(std::string(what) + ": a prediction is not finite: no quantile leaf values; the model is unchanged");
    if (flag & kern::kQuantileBadResidual)
        throw InvalidArgument(std::string(what) + ": a residual fl32(prediction - target) is not finite: no quantile leaf values; the model is unchanged");
    for (size_t l = 0; l < NL; ++l) {
        const int depth = model.oblivious() ? model.depths[t] : model.depths[leaf0 + l];
        if (counts[l] == 0 || depth <= 0) continue;   // (newton_core.h's rule: such a leaf keeps the value the step gave it)
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
    const int D = md.output_dim, T = md.n_trees;
    check_prepared_dataset("quantile_leaves_prepared", ds);
    if (D > 128) throw Unsupported("quantile_leaves_prepared: output_dim > 128");
    if (pred == nullptr) throw InvalidArgument("quantile_leaves_prepared: no prediction");
    if (targets == nullptr) throw InvalidArgument("Cannot call quantile_leaves_prepared without targets!");
    check_alpha("quantile_leaves_prepared", kern::kObjQuantile, alpha, D, false);
    if (T == 0) throw InvalidArgument("quantile_leaves_prepared: the model has no trees");
    if (tree < -1 || tree >= T) throw InvalidArgument("quantile_leaves_prepared: tree " + std::to_string(tree) + " is outside the model's " + std::to_string(T) + " trees (-1: the last)");
    const int t = tree == -1 ? T - 1 : tree;
    if (m <= 0) throw InvalidArgument("quantile_leaves_prepared: no rows (m must be positive)");
    if (rows == nullptr && m != ds->n)
        throw InvalidArgument("quantile_leaves_prepared: pred has " + std::to_string(m) + " rows, the data set " + std::to_string(ds->n) + " (pass rows to select over a subset)");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, "quantile_leaves_prepared", t, t + 1);
    ensure_device();
    ev_used_ = 0;
    ev_names_.clear();
    phases_.clear();
    hipStream_t s = stream_;
    const int32_t *d_rows = rows ? checked_rows(d_sub_rows_, d_rows_mm_, rows, rows_dev, m, ds->n, s) : nullptr;
    const size_t n_el = static_cast<size_t>(m) * D;
    const float *dp = pred_dev ? pred : upload(d_obj_pred_, pred, n_el, "H2D predictions");
    const float *dt = targets_dev ? targets : upload(d_obj_targets_, targets, n_el, "H2D targets");
    const float *da = upload(d_lq_alpha_, alpha, static_cast<size_t>(D), "H2D levels");
    quantile_leaves_run("quantile_leaves_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, dp, dt, /*abs_index=*/false, da, t,
                        hooks::on(hooks::CONTINUE_GENERIC), values_out, counts_out, ranks_out);
}

// ---- classifier metrics: the checks, the host rule, the device pipeline (kern::metric_error / kern::metric_auc) and the value from its integers
void Engine::check_metric(const char *what, int objective, int metric) {
    if (metric != kern::kMetricError && metric != kern::kMetricAuc)
        throw InvalidArgument(std::string(what) + ": unknown metric " + std::to_string(metric) + " (error = 1, auc = 2)");
    if (objective == kern::kObjRmse || objective == kern::kObjQuantile)
        throw InvalidArgument(std::string(what) + ": the " + (objective == kern::kObjRmse ? "rmse" : "quantile") + " objective has no metric (error and auc are for logistic and softmax)");
    if (metric == kern::kMetricAuc && objective == kern::kObjSoftmax)
        throw Unsupported(std::string(what) + ": auc with the softmax objective (a multi-class AUC) is not supported");
}

namespace {
// a column of one class has no AUC
void check_auc_column(const char *what, int d, uint64_t P, uint64_t N) {
    if (P == 0 || N == 0)
        throw InvalidArgument(std::string(what) + ": column " + std::to_string(d) + " of the targets has no " + (P == 0 ? "positive" : "negative") +
                              " row (a target above 0.5 is positive): its AUC is not defined");
}
void metric_counts_out(const std::vector<uint64_t> &c, int64_t *counts) {
    if (counts) for (size_t i = 0; i < c.size(); ++i) counts[i] = static_cast<int64_t>(c[i]);
}
}  // namespace

void Engine::eval_metric_host(const float *pred, const void *targets, int n, int D, int objective, int metric, double *value, int64_t *counts) {
    if (pred == nullptr || targets == nullptr) throw InvalidArgument("eval_metric_host: null argument");
    if (value == nullptr && counts == nullptr) throw InvalidArgument("eval_metric_host: no place for a result");
    if (n <= 0) throw InvalidArgument("eval_metric_host: no rows (n must be positive)");
    if (D < 1) throw InvalidArgument("eval_metric_host: output_dim must be positive");
    check_objective("eval_metric_host", objective, D);
    check_metric("eval_metric_host", objective, metric);
    const bool softmax = objective == kern::kObjSoftmax;
    const int C = kern::metric_count_columns(softmax, D);
    std::vector<uint64_t> c(static_cast<size_t>(C) * kern::metric_count_width(metric), 0);
    if (softmax) {
        const int32_t *labels = static_cast<const int32_t *>(targets);
        for (int r = 0; r < n; ++r) {
            if (labels[r] < 0 || labels[r] >= D)
                throw InvalidArgument("eval_metric_host: label " + std::to_string(labels[r]) + " (row " + std::to_string(r) + ") is outside [0, " + std::to_string(D) + ")");
            c[0] += kern::metric_argmax(pred + static_cast<size_t>(r) * D, D) != labels[r] ? 1 : 0;
        }
    } else if (metric == kern::kMetricError) {
        const float *y = static_cast<const float *>(targets);
        for (int r = 0; r < n; ++r)
            for (int d = 0; d < D; ++d) c[d] += kern::metric_logistic_wrong(pred[static_cast<size_t>(r) * D + d], y[static_cast<size_t>(r) * D + d]) ? 1 : 0;
    } else {
        const float *y = static_cast<const float *>(targets);
        std::vector<uint32_t> pos, neg;
        for (int d = 0; d < D; ++d) {
            pos.clear(); neg.clear();
            for (int r = 0; r < n; ++r) {
                const size_t at = static_cast<size_t>(r) * D + d;
                (kern::metric_positive(y[at]) ? pos : neg).push_back(kern::metric_key(pred[at]));
            }
            check_auc_column("eval_metric_host", d, pos.size(), neg.size());
            std::sort(neg.begin(), neg.end());
            uint64_t u2 = 0;
            for (const uint32_t k : pos)
                u2 += static_cast<uint64_t>(std::lower_bound(neg.begin(), neg.end(), k) - neg.begin()) +
                      static_cast<uint64_t>(std::upper_bound(neg.begin(), neg.end(), k) - neg.begin());
            c[3 * d] = u2; c[3 * d + 1] = pos.size(); c[3 * d + 2] = neg.size();
        }
    }
    if (value) *value = kern::metric_value(metric, c.data(), C, static_cast<uint64_t>(n) * (softmax ? 1 : D));
    metric_counts_out(c, counts);
}

void Engine::eval_metric(const float *pred, bool pred_dev, const void *targets, bool targets_dev, int n, int objective, int metric, double *value, int64_t *counts) {
    const int D = model.meta.output_dim;
    if (pred == nullptr || targets == nullptr) throw InvalidArgument("eval_metric: null argument");
    if (value == nullptr && counts == nullptr) throw InvalidArgument("eval_metric: no place for a result");
    if (n <= 0) throw InvalidArgument("eval_metric: no rows (n must be positive)");
    if (D > 128) throw Unsupported("eval_metric: output_dim > 128");
    check_objective("eval_metric", objective, D);
    check_metric("eval_metric", objective, metric);
    const bool softmax = objective == kern::kObjSoftmax, auc = metric == kern::kMetricAuc;
    if (auc && !kern::metric_auc_fits(n, D)) throw Unsupported("eval_metric: auc needs n * output_dim < 2^31 - 2048");
    ensure_device();
    hipStream_t s = stream_;
    const size_t n_el = static_cast<size_t>(n) * D, tar_el = softmax ? static_cast<size_t>(n) : n_el;
    const float *dp = pred_dev ? pred : upload(d_obj_pred_, pred, n_el, "H2D predictions");
    const float *dt = targets_dev ? static_cast<const float *>(targets) : upload(d_obj_targets_, static_cast<const float *>(targets), tar_el, "H2D targets");
    if (softmax) check_labels("eval_metric", reinterpret_cast<const int32_t *>(dt), n, D, nullptr);
    const int C = kern::metric_count_columns(softmax, D);
    std::vector<unsigned long long> h(static_cast<size_t>(C) * 2, 0);   // the counters, and behind them the positives per column (auc)
    unsigned long long *dc = static_cast<unsigned long long *>(d_met_counts_.ensure(sizeof(unsigned long long) * h.size()));
    hip_check(hipMemsetAsync(dc, 0, sizeof(unsigned long long) * h.size(), s), "zero metric counters");
    if (auc) kern::metric_auc(dp, dt, n, D, d_met_scratch_.ensure(kern::metric_auc_scratch_bytes(n, D)), dc + C, dc, s);
    else kern::metric_error(objective, dp, dt, n, D, dc, s);
    hip_check(hipGetLastError(), "eval_metric kernels");
    hip_check(hipMemcpyAsync(h.data(), dc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, s), "D2H metric counters");
    hip_check(hipStreamSynchronize(s), "sync");
    std::vector<uint64_t> c(static_cast<size_t>(C) * kern::metric_count_width(metric), 0);
    for (int d = 0; d < C; ++d) {
        if (!auc) { c[d] = h[d]; continue; }
        const uint64_t P = h[C + d], N = static_cast<uint64_t>(n) - P;
        check_auc_column("eval_metric", d, P, N);
        c[3 * d] = h[d]; c[3 * d + 1] = P; c[3 * d + 2] = N;
    }
    if (value) *value = kern::metric_value(metric, c.data(), C, static_cast<uint64_t>(n) * (softmax ? 1 : D));
    metric_counts_out(c, counts);
}

// ---- the fit: the stopping rule, the refusals that need no data set, a held prediction, and the stages of Engine::fit_prepared in its order
void Engine::early_stop_scan(const double *curve, int n, int rounds, double min_delta, int *stop_after, int *best) {
    if (curve == nullptr || stop_after == nullptr || best == nullptr) throw InvalidArgument("early_stop_scan: null argument");
    if (n <= 0) throw InvalidArgument("early_stop_scan: an empty curve");
    if (rounds < 0) throw InvalidArgument("early_stop_scan: rounds must be >= 0");
    if (!(min_delta >= 0.0)) throw InvalidArgument("early_stop_scan: min_delta must be >= 0 (and not NaN)");
    int b = 0, k = 1;
    for (; k < n; ++k) {
        if (curve[k] < curve[b] - min_delta) b = k;   // (false for a NaN on either side)
        if (rounds > 0 && k - b >= rounds) break;
    }
    *stop_after = k < n ? k : n - 1;
    *best = b;
}

void Engine::precheck_fit(const void *targets, int iterations, const FitOptions &opt, const FitValid *valid) const {
    const gbrl_hip_metadata &md = model.meta;
    check_prepared_model("fit_prepared");
    if (targets == nullptr) throw InvalidArgument("Cannot call fit without targets!");
    if (iterations < 0) throw InvalidArgument("iterations must be >= 0");
    if (md.batch_size <= 0) throw InvalidArgument("batch_size must be positive");
    if (md.max_depth > kern::kMaxPath) throw Unsupported("max_depth > 32 is not supported");
    if (md.n_bins < 1 || md.n_bins > 65534) throw Unsupported("n_bins must be in [1, 65534]");
    if (md.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    check_subsample("fit_prepared", opt.subsample);
    check_colsample("fit_prepared", opt.colsample);
    if (opt.goss_other != 0.0) {   // (0 means off; a NaN is not 0: it reaches check_goss)
        check_goss("fit_prepared", opt.goss_top, opt.goss_other);
        if (opt.subsample < 1.0) throw InvalidArgument("fit_prepared: goss and subsample < 1 are two draws of one iteration's rows: use one of them");
    }
    const bool ranking = kern::rank_objective(opt.objective);
    if (ranking) {   // the ranking objectives: their own list (rank_core.h; a gradient is a sum over the rows of a query)
        check_rank_group("fit_prepared", opt.group, opt.n_groups, -1, opt.objective, opt.ndcg_at, md.output_dim);
        if (opt.subsample < 1.0) throw InvalidArgument("fit_prepared: subsample < 1 with a ranking objective is not supported (a draw of rows cuts queries apart)");
        if (opt.goss_other != 0.0) throw InvalidArgument("fit_prepared: goss with a ranking objective is not supported (a draw of rows cuts queries apart)");
        if (opt.weights != nullptr || (valid != nullptr && valid->weights != nullptr))
            throw InvalidArgument("fit_prepared: weights and valid_weights with a ranking objective are not supported");
        if (opt.alpha != nullptr) throw InvalidArgument("fit_prepared: alpha is the level table of the quantile objective; a ranking objective takes none");
        if (opt.metric != kern::kMetricNone) throw InvalidArgument("fit_prepared: eval_metric with a ranking objective is not supported (valid_loss is 1 - NDCG or the pairwise loss)");
        if (opt.leaf_update == kern::kLeafQuantile) throw InvalidArgument("fit_prepared: quantile leaf values belong to the quantile objective");
        check_leaf_update("fit_prepared", kern::kObjLogistic, opt.leaf_update, opt.leaf_l2);   // (an unknown rule, a bad leaf_l2)
        if (valid != nullptr) {
            if (valid->group == nullptr || valid->n_groups <= 0)
                throw InvalidArgument("fit_prepared: a validation set of a ranking objective needs valid_group, the sizes of its queries");
            check_rank_group("fit_prepared", valid->group, valid->n_groups, -1, opt.objective, opt.ndcg_at, md.output_dim, "valid_group");
        }
    } else {
        if (opt.group != nullptr || opt.n_groups != 0 || opt.ndcg_at != 0 || (valid != nullptr && (valid->group != nullptr || valid->n_groups != 0)))
            throw InvalidArgument("fit_prepared: group, valid_group and ndcg_at belong to the ranking objectives (pairwise, lambdarank)");
        check_objective("fit_prepared", opt.objective, md.output_dim);
        check_leaf_update("fit_prepared", opt.objective, opt.leaf_update, opt.leaf_l2);
        check_alpha("fit_prepared", opt.objective, opt.alpha, md.output_dim, opt.weights != nullptr || (valid != nullptr && valid->weights != nullptr));
    }
    if (opt.leaf_update == kern::kLeafQuantile && opt.goss_other != 0.0)
        throw Unsupported("fit_prepared: goss with quantile leaf values is not supported (the amplified rows would need a weighted quantile)");
    if (opt.metric != kern::kMetricNone) {
        if (valid == nullptr) throw InvalidArgument("fit_prepared: eval_metric needs a validation set (valid=)");
        check_metric("fit_prepared", opt.objective, opt.metric);
    }
    if (valid == nullptr) return;
    if (valid->weights != nullptr && opt.metric != kern::kMetricNone)
        throw Unsupported("fit_prepared: valid_weights with eval_metric is not supported (the metrics count rows; weighted metrics are not implemented)");
    if (valid->targets == nullptr) throw InvalidArgument("fit_prepared: a validation set needs valid_targets");
    if (valid->rounds < 0) throw InvalidArgument("fit_prepared: early_stopping_rounds must be >= 0");
    if (!(valid->min_delta >= 0.0)) throw InvalidArgument("fit_prepared: min_delta must be >= 0 (and not NaN)");
}

// A data set's rows carried through the model's trees: the rows of batch b (bs rows each, the last one shorter) of P hold the trees [0, through[b]).
struct Engine::Held {
    const PreparedDataset *ds = nullptr;
    float *P = nullptr;   // [ds->n][D], device
    int bs = 1;
    std::vector<int> through;
    void start(const PreparedDataset *data, float *pred, int batch_rows) {   // the caller has tiled the bias: through 0 trees everywhere
        ds = data; P = pred; bs = batch_rows;
        through.assign((data->n + batch_rows - 1) / batch_rows, 0);
    }
};

// A walk that ended in a trailing run of one-leaf greedy trees applied nothing for them (it ran off the ensemble): it resumes at the first of them.
void Engine::advance_held(Held &h, int start, int bn, const float *targets, float *grad_out, const float *loss_targets, double *loss_part, bool generic,
                          int objective, const float *weights, const float *d_alpha) {
    const int T = model.meta.n_trees, D = model.meta.output_dim;
    int &through = h.through[start / h.bs];
    int from = through;
    while (from > 0 && runs_on(model, from - 1)) --from;
    check_code_range(*h.ds, "fit_prepared", from, T);
    sync_model_to_device();
    const kern::CodeTables ct = sync_code_tables(*h.ds);
    float *p = h.P + static_cast<size_t>(start) * D;
    const size_t at = static_cast<size_t>(start) * (objective == kern::kObjSoftmax ? 1 : D);   // (softmax: a label per row)
    kern::predict_continue_codes(mirror_view(), ct, kern::CodeRows{h.ds->prep.d_codes, h.ds->n, h.ds->code_groups(), nullptr, start}, bn, from, T, p, p,
                                 targets ? targets + at : nullptr, grad_out, loss_targets ? loss_targets + at : nullptr, loss_part, generic, stream_, objective,
                                 weights ? weights + start : nullptr, d_alpha);
    through = T;
}

// One fit_prepared call behind its argument checks: what the stages share, and the stages in the order Engine::fit_prepared runs them.
struct Engine::FitRun {
    Engine &e;
    const PreparedDataset *const ds;
    const FitOptions opt;
    FitValid *const v;
    const int iterations, n, D, bs, T0;   // T0: the tree count at entry
    const bool generic = hooks::on(hooks::CONTINUE_GENERIC);
    const float *dtar = nullptr, *dvtar = nullptr;   // the targets on the device (softmax: int32 labels behind them, one per row)
    const float *dw = nullptr, *dvw = nullptr;       // the row weights of the two sets on the device (null: none)
    const float *d_alpha = nullptr;                  // quantile: the levels on the device
    float wmax = 0.0f;                               // the largest training weight: what the Newton quantum makes room for
    double W, Wv = 0.0;                              // what the two losses and the bias divide by: the weights' float64 sums, or the row counts
    std::vector<int32_t> class_counts;               // softmax: rows per class of the training set
    Held train, watched;                             // the training rows, in batches of bs; the validation rows, as one batch
    float *G = nullptr;                              // [n][D]: the gradient of the current batch from row 0, of every row for the final loss
    const int32_t *d_iota = nullptr;                 // 0 .. n - 1: the row ranges step_prepared's body gathers (bs < n)
    double *d_vpart = nullptr, *d_vsums = nullptr;   // the validation rows' loss partials, one sum per iteration from k = 0
    // a metric of the validation rows: mC integer counters per iteration from k = 0 (wrong cells per column, or 2U per column), the positives of
    // every validation column (auc), one iteration's counters on the host (a stopping rule reads them back), and the curve the rule sees
    const int mC;
    unsigned long long *d_vmetric = nullptr;
    void *d_mscratch = nullptr;
    std::vector<uint64_t> vpos;
    std::vector<unsigned long long> h_mrow;
    std::vector<double> score;
    bool sampled = false, colsampled = false;
    const bool goss;                                      // one-side sampling takes the place of the subsample draw
    int32_t *d_srows = nullptr, *d_sscratch = nullptr;   // a sampled iteration: the kept rows of the batch, the sampler's block counts + m
    float *Gs = nullptr;                                  // and their gradient rows
    float *d_sfactor = nullptr, *d_eff = nullptr;         // goss: the kept rows' factors; newton: their effective weights fl32(w * factor) by absolute row
    int start = 0, bn = 0;                               // the batch cursor
    const bool ranking;                                  // a ranking objective: targets are int32 labels, the gradient comes from the rank kernels
    float *H = nullptr;                                  // ... its hessian [n] beside G (newton leaves)

    FitRun(Engine &eng, const PreparedDataset *data, int iters, const FitOptions &o, FitValid *valid)
        : e(eng), ds(data), opt(o), v(valid), iterations(iters), n(data->n), D(eng.model.meta.output_dim), bs(eng.model.meta.batch_size), T0(eng.model.meta.n_trees),
          W(static_cast<double>(data->n)), mC(kern::metric_count_columns(o.objective == kern::kObjSoftmax, eng.model.meta.output_dim)), goss(o.goss_other != 0.0),
          ranking(kern::rank_objective(o.objective)) {
        bn = start + bs < n ? bs : n - start;                                       // fitter.cpp:120
    }

    const float *stage(DevBuf &buf, const void *host_or_dev, bool on_dev, int rows) {
        const float *t = static_cast<const float *>(host_or_dev);
        return on_dev ? t : e.upload(buf, t, static_cast<size_t>(rows) * (opt.objective == kern::kObjSoftmax ? 1 : D), "H2D targets");
    }
    // Both target arrays on the device; newton with logistic: a training target outside [0, 1] is refused; softmax: a label outside [0, D), in either set, is refused before anything changes.
    void stage_targets(const void *targets, bool targets_dev) {
        dtar = stage(e.d_fp_targets_, targets, targets_dev, n);
        if (v) dvtar = stage(e.d_fp_vtargets_, v->targets, v->targets_dev, v->ds->n);
        if (v) Wv = static_cast<double>(v->ds->n);
        if (opt.alpha) d_alpha = e.upload(e.d_lq_alpha_, opt.alpha, static_cast<size_t>(D), "H2D levels");
        if (ranking) {   // the labels of both sets checked, their queries on the device; all of it before anything changes
            e.rank_prepare("fit_prepared", e.rk_sets_[1], reinterpret_cast<const int32_t *>(dtar), opt.group, opt.n_groups, n, opt.ndcg_at);
            if (opt.objective == kern::kObjPairwise && e.rk_sets_[1].pairs == 0)
                throw InvalidArgument("fit_prepared: no query of the training set holds two different labels: the pairwise objective has no pair to learn from");
            if (v) e.rank_prepare("fit_prepared (valid_targets)", e.rk_sets_[2], reinterpret_cast<const int32_t *>(dvtar), v->group, v->n_groups, v->ds->n, opt.ndcg_at);
            return;
        }
        if (opt.weights) {
            dw = opt.weights_dev ? opt.weights : e.upload(e.d_fp_weights_, opt.weights, static_cast<size_t>(n), "H2D weights");
            const WeightStats st = e.check_weights("fit_prepared (weights)", dw, n, true);
            wmax = st.max; W = st.sum;
        }
        if (v && v->weights) {
            dvw = v->weights_dev ? v->weights : e.upload(e.d_fp_vweights_, v->weights, static_cast<size_t>(v->ds->n), "H2D validation weights");
            Wv = e.check_weights("fit_prepared (valid_weights)", dvw, v->ds->n, true).sum;
        }
        if (goss && kern::obj_weighted(dw ? wmax : 1.0f, kern::goss_plan(n, opt.goss_top, opt.goss_other).amp) > kern::kWeightMax)
            throw InvalidArgument("fit_prepared: the largest weight times goss's amplification (1 - top_rate) / other_rate is above 65536: the Newton quantum has no room for it");
        if (opt.metric == kern::kMetricAuc) count_positives();
        if (opt.leaf_update == kern::kLeafNewton && opt.objective == kern::kObjLogistic) check_unit_targets();
        if (opt.objective == kern::kObjQuantile) check_finite_targets();
        if (opt.objective != kern::kObjSoftmax) return;
        e.check_labels("fit_prepared", reinterpret_cast<const int32_t *>(dtar), n, D, &class_counts);
        if (v) e.check_labels("fit_prepared (valid_targets)", reinterpret_cast<const int32_t *>(dvtar), v->ds->n, D, nullptr);
    }
    // newton + logistic: a training target outside [0, 1] (a NaN counts) is refused before anything changes (the sums' kernel would flag it too)
    void check_unit_targets() {
        hipStream_t s = e.stream_;
        unsigned long long flag = 0;
        unsigned long long *d = static_cast<unsigned long long *>(e.d_newton_acc_.ensure(sizeof(unsigned long long)));
        hip_check(hipMemsetAsync(d, 0, sizeof(unsigned long long), s), "zero target flag");
        kern::newton_check_targets(dtar, static_cast<size_t>(n) * D, d, s);
        hip_check(hipMemcpyAsync(&flag, d, sizeof(flag), hipMemcpyDeviceToHost, s), "D2H target flag");
        hip_check(hipStreamSynchronize(s), "sync");
        if (flag) throw InvalidArgument("fit_prepared: a logistic target is outside [0, 1] (or NaN): newton leaf values need targets in [0, 1]");
    }
    // quantile: a training target that is not finite is refused before anything changes (the bias and the leaf kernels would flag it too, a warm start
    // only after its first step)
    void check_finite_targets() {
        hipStream_t s = e.stream_;
        uint32_t flag = 0;
        uint32_t *d = static_cast<uint32_t *>(e.d_lq_res_.ensure(sizeof(uint32_t)));
        hip_check(hipMemsetAsync(d, 0, sizeof(uint32_t), s), "zero target flag");
        kern::leaf_quantile_check_targets(dtar, static_cast<size_t>(n) * D, d, s);
        hip_check(hipMemcpyAsync(&flag, d, sizeof(flag), hipMemcpyDeviceToHost, s), "D2H target flag");
        hip_check(hipStreamSynchronize(s), "sync");
        if (flag) throw InvalidArgument("fit_prepared: a target is not finite: the quantile objective needs finite targets");
    }
    // auc: the positives of every validation column; a column of one class is refused before anything changes
    void count_positives() {
        hipStream_t s = e.stream_;
        const int nv = v->ds->n;
        std::vector<unsigned long long> h(D, 0);
        unsigned long long *dc = static_cast<unsigned long long *>(e.d_met_counts_.ensure(sizeof(unsigned long long) * h.size()));
        hip_check(hipMemsetAsync(dc, 0, sizeof(unsigned long long) * h.size(), s), "zero metric counters");
        kern::metric_positives(dvtar, nv, D, dc, s);
        hip_check(hipMemcpyAsync(h.data(), dc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, s), "D2H positives");
        hip_check(hipStreamSynchronize(s), "sync");
        vpos.assign(h.begin(), h.end());
        for (int d = 0; d < D; ++d) check_auc_column("fit_prepared (valid_targets)", d, vpos[d], static_cast<uint64_t>(nv) - vpos[d]);
    }
    // A fresh model's bias by objective, and the feature counts as step_prepared latches them.
    // With weights: sum w y / W per column and the weight W_c of a class, from column_sums' own reduction with the weight as a per-row factor.
    void set_bias(ColumnStats &stats) {
        Model &model = e.model;
        if (ranking) {   // both ranking losses are invariant to a shift of the scores
            model.bias[0] = 0.0f;
        } else if (opt.objective == kern::kObjQuantile) {   // quantile_core.h: one leaf of every row at p = 0 -- the k-th smallest target of the column, k from n
            hipStream_t s = e.stream_;
            const size_t words = kern::leaf_quantile_result_words(1, D);
            uint32_t *dres = static_cast<uint32_t *>(e.d_lq_res_.ensure(sizeof(uint32_t) * words));
            void *scratch = e.d_lq_scratch_.ensure(kern::leaf_quantile_bias_scratch_bytes(n, D));
            hip_check(hipMemsetAsync(dres, 0, sizeof(uint32_t) * words, s), "zero bias quantiles");
            kern::leaf_quantile_bias(dtar, n, D, d_alpha, scratch, dres, s);
            e.lq_host_.resize(words);
            hip_check(hipMemcpyAsync(e.lq_host_.data(), dres, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, s), "D2H bias quantiles");
            hip_check(hipGetLastError(), "fit_prepared kernels");
            hip_check(hipStreamSynchronize(s), "sync");
            if (e.lq_host_[words - 1] & kern::kQuantileBadTarget)
                throw InvalidArgument("fit_prepared: a target is not finite: the quantile objective needs finite targets");
            for (int d = 0; d < D; ++d) model.bias[d] = -kern::quantile_key_value(e.lq_host_[d]);
        } else if (opt.objective == kern::kObjSoftmax && dw) {   // the weighted log prior, an empty class counted as half a mean row
            const std::vector<double> &hs = stats.weighted_sums(nullptr, reinterpret_cast<const int32_t *>(dtar), dw, n);
            const double floor_w = 0.5 * W / static_cast<double>(n);
            for (int d = 0; d < D; ++d) model.bias[d] = static_cast<float>(std::log(std::max(hs[d], floor_w) / W));
        } else if (opt.objective == kern::kObjSoftmax) {   // the log prior, an empty class counted as half a row
            for (int d = 0; d < D; ++d) model.bias[d] = static_cast<float>(std::log(std::max(static_cast<double>(class_counts[d]), 0.5) / static_cast<double>(n)));
        } else {
            const std::vector<double> &hs = dw ? stats.weighted_sums(dtar, nullptr, dw, n) : stats.sums(dtar, n, nullptr);
            const double lo = 0.5 / static_cast<double>(n);
            for (int d = 0; d < D; ++d) {
                const double mean = hs[d] / W;
                if (opt.objective == kern::kObjRmse) {   // the column means of the targets (gbrl.cpp:1075-1077)
                    model.bias[d] = static_cast<float>(mean);
                } else {                                  // logistic: the log odds of the column mean, kept off 0 and 1 by half a row
                    const double c = std::min(std::max(mean, lo), 1.0 - lo);
                    model.bias[d] = static_cast<float>(std::log(c / (1.0 - c)));
                }
            }
        }
        ++model.version;
        if (model.meta.iteration == 0) { model.meta.n_num_features = ds->F; model.meta.n_cat_features = 0; }
    }
    // The held predictions start as the tiled bias, through 0 trees everywhere.
    void hold_predictions() {
        hipStream_t s = e.stream_;
        e.sync_model_to_device();
        train.start(ds, static_cast<float *>(e.d_fp_pred_.ensure(sizeof(float) * static_cast<size_t>(n) * D)), bs);
        G = static_cast<float *>(e.d_fp_grads_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
        if (ranking && opt.leaf_update == kern::kLeafNewton) H = static_cast<float *>(e.d_fp_hess_.ensure(sizeof(float) * static_cast<size_t>(n)));
        kern::tile_rows(e.m_bias_.as<float>(), D, n, train.P, s);
        if (bs < n) {
            std::vector<int32_t> iota(n);
            std::iota(iota.begin(), iota.end(), 0);
            d_iota = e.upload(e.d_fp_iota_, iota.data(), iota.size(), "H2D iota");
            hip_check(hipStreamSynchronize(s), "sync");   // iota goes out of scope
        }
        if (v == nullptr) return;
        const int nv = v->ds->n;
        watched.start(v->ds, static_cast<float *>(e.d_fp_vpred_.ensure(sizeof(float) * static_cast<size_t>(nv) * D)), nv);
        d_vpart = static_cast<double *>(e.d_fp_vpart_.ensure(sizeof(double) * kern::staged_loss_partials(nv)));
        d_vsums = static_cast<double *>(e.d_fp_vsums_.ensure(sizeof(double) * (static_cast<size_t>(iterations) + 1)));
        kern::tile_rows(e.m_bias_.as<float>(), D, nv, watched.P, s);
        v->best_n_trees = T0;
        if (opt.metric == kern::kMetricNone) return;
        const size_t words = (static_cast<size_t>(iterations) + 1) * mC;
        d_vmetric = static_cast<unsigned long long *>(e.d_fp_vmetric_.ensure(sizeof(unsigned long long) * words));
        hip_check(hipMemsetAsync(d_vmetric, 0, sizeof(unsigned long long) * words, s), "zero metric counters");
        if (opt.metric == kern::kMetricAuc) d_mscratch = e.d_met_scratch_.ensure(kern::metric_auc_scratch_bytes(nv, D));
        h_mrow.assign(mC, 0);
        score.assign(static_cast<size_t>(iterations) + 1, 0.0);
    }
    // a loss from the sum its kernels left: the mean row loss, or a ranking objective's rule (rank_core.h)
    double loss_of(double sum, bool valid_set) const {
        if (ranking) return rank_loss(e.rk_sets_[valid_set ? 2 : 1], opt.objective, sum);
        return mean_loss(opt.objective, sum, valid_set ? Wv : W);
    }
    // ---- the validation watch
    // loss_out[k] after k iterations: one launch + the finishing sum on the device, then the metric's integers of the same held prediction; with
    // a stopping rule both also on the host (one read-back: 8 bytes and the metric's counters, one wait)
    void evaluate(int k) {
        const int nv = v->ds->n;
        v->done = k;
        double sum = 0.0;
        if (ranking) {   // the walk without a tail, then the rule's loss of the held scores (rank_gradient's, bit for bit)
            e.advance_held(watched, 0, nv, nullptr, nullptr, nullptr, nullptr, generic, kern::kObjRmse);
            e.rank_eval(e.rk_sets_[2], opt.objective, opt.ndcg_at, watched.P, reinterpret_cast<const int32_t *>(dvtar), nullptr, nullptr, nullptr, true, d_vsums + k,
                        v->rounds > 0 ? &sum : nullptr, nullptr);
            if (v->rounds > 0) {
                hip_check(hipStreamSynchronize(e.stream_), "sync");
                v->loss_out[k] = loss_of(sum, true);
            }
            return;
        }
        e.advance_held(watched, 0, nv, nullptr, nullptr, dvtar, d_vpart, generic, opt.objective, dvw, d_alpha);
        e.finish_loss_sum(d_vpart, kern::staged_loss_partials(nv), d_vsums + k, v->rounds > 0 ? &sum : nullptr);
        if (opt.metric != kern::kMetricNone) measure(k);
        if (v->rounds > 0) {
            hip_check(hipStreamSynchronize(e.stream_), "sync");
            v->loss_out[k] = loss_of(sum, true);
            if (opt.metric != kern::kMetricNone) record_metric(k, h_mrow.data());
        }
    }
    // the metric of the watched prediction into the counters of entry k; it reads the prediction and never writes it
    void measure(int k) {
        hipStream_t s = e.stream_;
        const int nv = v->ds->n;
        unsigned long long *row = d_vmetric + static_cast<size_t>(k) * mC;
        if (opt.metric == kern::kMetricAuc) kern::metric_auc(watched.P, dvtar, nv, D, d_mscratch, nullptr, row, s);
        else kern::metric_error(opt.objective, watched.P, dvtar, nv, D, row, s);
        if (v->rounds > 0) hip_check(hipMemcpyAsync(h_mrow.data(), row, sizeof(unsigned long long) * mC, hipMemcpyDeviceToHost, s), "D2H metric counters");
    }
    // metric_out[k] from entry k's integers, and what the stopping rule sees of it: the error as it is, the AUC negated (exact)
    void record_metric(int k, const unsigned long long *row) {
        const int nv = v->ds->n;
        const bool auc = opt.metric == kern::kMetricAuc;
        std::vector<uint64_t> c(static_cast<size_t>(mC) * kern::metric_count_width(opt.metric));
        for (int d = 0; d < mC; ++d) {
            if (!auc) { c[d] = row[d]; continue; }
            c[3 * d] = row[d]; c[3 * d + 1] = vpos[d]; c[3 * d + 2] = static_cast<uint64_t>(nv) - vpos[d];
        }
        const double value = kern::metric_value(opt.metric, c.data(), mC, static_cast<uint64_t>(nv) * (opt.objective == kern::kObjSoftmax ? 1 : D));
        v->metric_out[k] = value;
        score[k] = auc ? -value : value;
    }
    int best_of_curve() const {
        int stop_after = 0, best = 0;
        early_stop_scan(opt.metric != kern::kMetricNone ? score.data() : v->loss_out, v->done + 1, v->rounds, v->min_delta, &stop_after, &best);
        return best;
    }
    bool stops_early() const { return v->rounds > 0 && v->done - best_of_curve() >= v->rounds; }
    void finish_watch() {
        if (v->rounds == 0) {   // the sums stayed on the device
            std::vector<double> sums(static_cast<size_t>(v->done) + 1);
            hip_check(hipMemcpyAsync(sums.data(), d_vsums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, e.stream_), "D2H validation losses");
            hip_check(hipStreamSynchronize(e.stream_), "sync");
            for (int k = 0; k <= v->done; ++k) v->loss_out[k] = loss_of(sums[k], true);
            if (opt.metric != kern::kMetricNone) {   // and so did the metric's integers
                std::vector<unsigned long long> rows((static_cast<size_t>(v->done) + 1) * mC);
                hip_check(hipMemcpyAsync(rows.data(), d_vmetric, sizeof(unsigned long long) * rows.size(), hipMemcpyDeviceToHost, e.stream_), "D2H validation metric");
                hip_check(hipStreamSynchronize(e.stream_), "sync");
                for (int k = 0; k <= v->done; ++k) record_metric(k, rows.data() + static_cast<size_t>(k) * mC);
            }
        }
        v->best_n_trees = T0 + best_of_curve();
    }
    // ---- the iterations
    // The workspace of the draws.  subsample == 1.0: no sampler exists; colsample == 1.0, or k == F: step_prepared_run never sees cols.
    void prepare_draws() {
        sampled = opt.subsample < 1.0;
        colsampled = opt.colsample < 1.0 && kern::sample_cols_count(ds->F, opt.colsample) < ds->F;
        if (!sampled && !goss) return;
        const int cap = std::min(bs, n);
        d_srows = static_cast<int32_t *>(e.d_fp_srows_.ensure(sizeof(int32_t) * static_cast<size_t>(cap)));
        Gs = static_cast<float *>(e.d_fp_sgrads_.ensure(sizeof(float) * static_cast<size_t>(cap) * D));
        if (!goss) {
            d_sscratch = static_cast<int32_t *>(e.d_fp_sscratch_.ensure(sizeof(int32_t) * (static_cast<size_t>(kern::sample_rows_blocks(cap)) + 1)));
            return;
        }
        d_sscratch = static_cast<int32_t *>(e.d_fp_gscratch_.ensure(sizeof(int32_t) * kern::goss_scratch_words(cap)));
        d_sfactor = static_cast<float *>(e.d_fp_sfactor_.ensure(sizeof(float) * static_cast<size_t>(cap)));
        if (opt.leaf_update == kern::kLeafNewton) d_eff = static_cast<float *>(e.d_fp_eff_.ensure(sizeof(float) * static_cast<size_t>(n)));
    }
    // One tree on the batch under the cursor.  Both draws are those of the tree count before the step.
    void iterate() {
        hipStream_t s = e.stream_;
        const int trees = e.model.meta.n_trees;
        e.begin_step_profile();
        e.phase_begin();
        if (ranking) e.advance_held(train, start, bn, nullptr, nullptr, nullptr, nullptr, generic, kern::kObjRmse);   // (no fused gradient: predict_continue_prepared's launch)
        else e.advance_held(train, start, bn, dtar, G, nullptr, nullptr, generic, opt.objective, dw, d_alpha);
        e.phase_end("continue_codes");
        if (ranking) {   // the gradient (and hessian) of every row from the rows of its query; one batch holds them all
            e.phase_begin();
            e.rank_eval(e.rk_sets_[1], opt.objective, opt.ndcg_at, train.P, reinterpret_cast<const int32_t *>(dtar), nullptr, G, H, false, nullptr, nullptr, nullptr);
            unsigned long long flag = 0;
            hip_check(hipMemcpyAsync(&flag, e.d_rk_stat_.as<unsigned long long>(), sizeof(flag), hipMemcpyDeviceToHost, s), "D2H rank flags");
            e.phase_end("rank_gradient");
            hip_check(hipStreamSynchronize(s), "sync");
            if (flag & kern::kRankBadPred) throw InvalidArgument("fit_prepared: a prediction is not finite: no ranking gradient; the model keeps the trees grown so far");
        }
        const float *g = G;
        const int32_t *rows = bn == n ? nullptr : d_iota + start;
        int m = bn;
        if (sampled) {   // a draw that keeps no row takes the whole batch
            e.phase_begin();
            kern::sample_rows(start, bn, kern::sample_threshold(opt.subsample), opt.seed, trees, G, D, d_srows, Gs, d_sscratch, s);
            int32_t kept = 0;
            hip_check(hipMemcpyAsync(&kept, d_sscratch, sizeof(kept), hipMemcpyDeviceToHost, s), "D2H sample count");
            e.phase_end("sample_rows");
            hip_check(hipStreamSynchronize(s), "sync");
            if (kept > 0) { g = Gs; rows = d_srows; m = kept; }
        } else if (goss) {   // likewise; the selection's tau stays on the device
            e.phase_begin();
            const kern::GossPlan plan = kern::goss_plan(bn, opt.goss_top, opt.goss_other);
            const kern::GossScratch gs = kern::goss_scratch(d_sscratch, bn);
            kern::goss_select(bn, plan.k, G, D, gs, s);
            e.phase_end("goss_select"); e.phase_begin();
            kern::goss_sample_passes(start, bn, plan.thr, plan.amp, opt.seed, trees, gs, G, D, d_srows, d_sfactor, Gs, dw, d_eff, s);
            int32_t kept = 0;
            hip_check(hipMemcpyAsync(&kept, d_sscratch, sizeof(kept), hipMemcpyDeviceToHost, s), "D2H sample count");
            e.phase_end("sample_goss");
            hip_check(hipStreamSynchronize(s), "sync");
            if (kept > 0) { g = Gs; rows = d_srows; m = kept; }
        }
        if (colsampled) {
            kern::sample_cols(ds->F, opt.colsample, opt.seed, trees, e.fit_cols_);
            e.step_prepared_run(ds, g, rows, m, e.fit_cols_.data(), static_cast<int>(e.fit_cols_.size()));
        } else {
            e.step_prepared_run(ds, g, rows, m);
        }
        if (opt.leaf_update == kern::kLeafNewton && ranking) {   // the sums of the g and h the tree was grown on, from their buffers; room for the largest query
            e.newton_leaves_run("fit_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), nullptr, 0}, n, G, H, /*abs_index=*/true, kern::kObjGiven,
                                e.model.meta.n_trees - 1, opt.leaf_l2, generic, nullptr, nullptr, nullptr, nullptr, static_cast<float>(e.rk_sets_[1].max_group));
        } else if (opt.leaf_update == kern::kLeafNewton) {   // the new tree's leaves from the rows it was grown on, at the held prediction over the trees before it
            const bool kept = rows == d_srows && rows != nullptr;
            const bool amplified = kept && goss;   // the kept rows of a one-side draw carry fl32(w * factor), with room for fl32(wmax * amp)
            const float amp = amplified ? kern::goss_plan(bn, opt.goss_top, opt.goss_other).amp : 1.0f;
            e.newton_leaves_run("fit_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), kept ? d_srows : nullptr, kept ? 0 : start}, m, train.P,
                                dtar, /*abs_index=*/true, opt.objective, e.model.meta.n_trees - 1, opt.leaf_l2, generic, nullptr, nullptr, nullptr,
                                amplified ? d_eff : dw, amplified ? kern::obj_weighted(dw ? wmax : 1.0f, amp) : wmax);
        }
        if (opt.leaf_update == kern::kLeafQuantile) {   // likewise: the level's order statistic of the residuals of the rows the tree was grown on
            const bool kept = rows == d_srows && rows != nullptr;
            e.quantile_leaves_run("fit_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), kept ? d_srows : nullptr, kept ? 0 : start}, m, train.P,
                                  dtar, /*abs_index=*/true, d_alpha, e.model.meta.n_trees - 1, generic, nullptr, nullptr, nullptr);
        }
        start += bn;                                                                // fitter.cpp:228-231
        if (start >= n) start = 0;
        bn = start + bs < n ? bs : n - start;
    }
    // Every batch to the end; the loss on the whole data set (fitter.cpp:246-251).  rmse: from the gradient of every row, written by the same
    // launches, as fit() computes it; an objective: from the held prediction by the stand-alone kernel, the loss tail's partials and sum.  With
    // weights rmse takes the second way too (G would hold w g, and sum (w g)^2 is not the weighted loss): objective_gradient's loss, bit for bit.
    float final_loss(ColumnStats &stats) {
        const bool rmse = opt.objective == kern::kObjRmse && dw == nullptr;
        for (int b0 = 0; b0 < n; b0 += bs)
            e.advance_held(train, b0, std::min(bs, n - b0), rmse ? dtar : nullptr, rmse ? G + static_cast<size_t>(b0) * D : nullptr, nullptr, nullptr, generic,
                           ranking ? kern::kObjRmse : opt.objective, nullptr, d_alpha);
        if (ranking) {   // the rule's loss of the held scores
            double *d_sum = static_cast<double *>(e.d_obj_sum_.ensure(sizeof(double)));
            double sum = 0.0;
            e.rank_eval(e.rk_sets_[1], opt.objective, opt.ndcg_at, train.P, reinterpret_cast<const int32_t *>(dtar), nullptr, nullptr, nullptr, true, d_sum, &sum, nullptr);
            hip_check(hipGetLastError(), "fit_prepared kernels");
            hip_check(hipStreamSynchronize(e.stream_), "sync");
            return static_cast<float>(loss_of(sum, false));
        }
        if (rmse) {
            hip_check(hipGetLastError(), "fit_prepared kernels");
            return stats.rmse(G, n);
        }
        const int nb = kern::staged_loss_partials(n);
        double *d_part = static_cast<double *>(e.d_obj_part_.ensure(sizeof(double) * nb)), *d_sum = static_cast<double *>(e.d_obj_sum_.ensure(sizeof(double)));
        kern::objective_rows(opt.objective, train.P, dtar, n, D, nullptr, d_part, e.stream_, dw, d_alpha);
        double sum = 0.0;
        e.finish_loss_sum(d_part, nb, d_sum, &sum);
        hip_check(hipGetLastError(), "fit_prepared kernels");
        hip_check(hipStreamSynchronize(e.stream_), "sync");
        return static_cast<float>(mean_loss(opt.objective, sum, W));
    }
};

float Engine::fit_prepared(const PreparedDataset *ds, const void *targets, bool targets_dev, int iterations, const FitOptions &opt, FitValid *valid,
                           float *weight_max_out) {
    precheck_fit(targets, iterations, opt, valid);
    check_prepared_dataset("fit_prepared", ds);
    if (valid) {
        check_prepared_dataset("fit_prepared", valid->ds);
        if (valid->ds->thresholds_id != ds->thresholds_id)
            throw InvalidArgument("fit_prepared: the validation set does not share the training set's thresholds (create it with prepare_dataset(obs, reference=ds))");
        if (valid->loss_out == nullptr) throw InvalidArgument("fit_prepared: no place for the validation losses");
        if (opt.metric != kern::kMetricNone && valid->metric_out == nullptr) throw InvalidArgument("fit_prepared: no place for the validation metric");
        if (opt.metric == kern::kMetricAuc && !kern::metric_auc_fits(valid->ds->n, model.meta.output_dim))
            throw Unsupported("fit_prepared: auc needs validation rows * output_dim < 2^31 - 2048");
    }
    if (kern::rank_objective(opt.objective)) {   // what needs the row counts: whole queries in the one batch, sizes that cover the rows
        check_rank_group("fit_prepared", opt.group, opt.n_groups, ds->n, opt.objective, opt.ndcg_at, model.meta.output_dim);
        if (valid) check_rank_group("fit_prepared", valid->group, valid->n_groups, valid->ds->n, opt.objective, opt.ndcg_at, model.meta.output_dim, "valid_group");
        if (model.meta.batch_size < ds->n)
            throw InvalidArgument("fit_prepared: batch_size " + std::to_string(model.meta.batch_size) + " < " + std::to_string(ds->n) +
                                  " rows: a batch of a ranking objective must hold whole queries (set batch_size >= the row count)");
    }
    const bool fresh = model.meta.n_trees == 0;
    if (!fresh) check_code_range(*ds, "fit_prepared", 0, model.meta.n_trees);   // a warm start continues from every tree the model has
    ensure_device();
    FitRun run(*this, ds, iterations, opt, valid);
    run.stage_targets(targets, targets_dev);
    if (weight_max_out) *weight_max_out = run.wmax;
    ColumnStats stats(*this);
    if (fresh) run.set_bias(stats);
    run.hold_predictions();
    if (valid) run.evaluate(0);
    run.prepare_draws();
    for (int i = 0; i < iterations; ++i) {
        run.iterate();
        if (valid == nullptr) continue;
        run.evaluate(i + 1);
        if (run.stops_early()) break;
    }
    if (valid) run.finish_watch();
    return run.final_loss(stats);
}

}  // namespace gbrl

