// engine_objective.hip -- an objective and a metric of a prediction matrix, on the host and on the device (engine_step_detail.h lists the units beside it):
//   Engine::check_objective / check_alpha / check_labels   what is refused about an objective, its level table and its class labels
//   Engine::check_weights[_host]       row weights (objective_core.h, newton_core.h): a weight vector's refusals, its maximum and its float64 sum in a fixed order
//                                      (kern::weight_stats), once per call and vector
//   Engine::objective_gradient[_host]  the gradient and the loss of an objective (objective_core.h; kern::objective_rows), finish_loss_sum behind a loss tail
//   Engine::objective_hessian_host     the hessian rule on the host (newton_core.h)
//   Engine::check_metric / eval_metric[_host]   the error rate and the exact AUC (metric_core.h; kern::metric_error / kern::metric_auc) and the value from its integers
#include "engine_codes_detail.h"
#include "newton_core.h"
#include "quantile_core.h"
#include "rank_core.h"

namespace gbrl {

namespace {
void weigh_rows(float *x, const float *weights, int n, int D) {
    for (int r = 0; r < n; ++r)
        for (int d = 0; d < D; ++d) x[static_cast<size_t>(r) * D + d] = kern::obj_weighted(weights[r], x[static_cast<size_t>(r) * D + d]);
}
void check_labels_host(const char *what, const int32_t *labels, int n, int D) {
    for (int r = 0; r < n; ++r)
        if (labels[r] < 0 || labels[r] >= D)
            throw InvalidArgument(std::string(what) + ": label " + std::to_string(labels[r]) + " (row " + std::to_string(r) + ") is outside [0, " + std::to_string(D) + ")");
}
void metric_counts_out(const std::vector<uint64_t> &c, int64_t *counts) {
    if (counts) for (size_t i = 0; i < c.size(); ++i) counts[i] = static_cast<int64_t>(c[i]);
}
}  // namespace

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
    read_back(h.data(), d, sizeof(int32_t) * h.size(), "D2H label counts");
    if (h[D] != 0x7fffffff) {
        int32_t bad = 0;
        read_back(&bad, d_labels + h[D], sizeof(bad), "D2H label");
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
    read_back(&st.sum, d_sum, sizeof(double), "D2H weight sum");
    if (h[0] != 0x7fffffff) {
        float bad = 0.0f;
        read_back(&bad, d_weights + h[0], sizeof(bad), "D2H weight");
        throw InvalidArgument(std::string(what) + ": weight " + std::to_string(bad) + " (row " + std::to_string(h[0]) + ") is not a finite number in [0, 65536]");
    }
    std::memcpy(&st.max, &h[1], sizeof(float));
    if (need_sum && !(st.sum > 0.0)) throw InvalidArgument(std::string(what) + ": the weights sum to 0: no weighted loss or bias is defined");
    return st;
}


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
        check_labels_host("objective_gradient_host", labels, n, D);
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
    const float *dp = staged(d_obj_pred_, pred, pred_dev, n_el, "H2D predictions");
    const float *dt = staged(d_obj_targets_, static_cast<const float *>(targets), targets_dev, tar_el, "H2D targets");
    if (objective == kern::kObjSoftmax) check_labels("objective_gradient", reinterpret_cast<const int32_t *>(dt), n, D, nullptr);
    const float *dw = weights ? staged(d_obj_weights_, weights, weights_dev, static_cast<size_t>(n), "H2D weights") : nullptr;
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

// ---- classifier metrics: the checks, the host rule, the device pipeline (kern::metric_error / kern::metric_auc) and the value from its integers
void Engine::check_metric(const char *what, int objective, int metric) {
    if (metric != kern::kMetricError && metric != kern::kMetricAuc)
        throw InvalidArgument(std::string(what) + ": unknown metric " + std::to_string(metric) + " (error = 1, auc = 2)");
    if (objective == kern::kObjRmse || objective == kern::kObjQuantile)
        throw InvalidArgument(std::string(what) + ": the " + (objective == kern::kObjRmse ? "rmse" : "quantile") + " objective has no metric (error and auc are for logistic and softmax)");
    if (metric == kern::kMetricAuc && objective == kern::kObjSoftmax)
        throw Unsupported(std::string(what) + ": auc with the softmax objective (a multi-class AUC) is not supported");
}

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
        check_labels_host("eval_metric_host", labels, n, D);
        for (int r = 0; r < n; ++r) c[0] += kern::metric_argmax(pred + static_cast<size_t>(r) * D, D) != labels[r] ? 1 : 0;
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
    const float *dp = staged(d_obj_pred_, pred, pred_dev, n_el, "H2D predictions");
    const float *dt = staged(d_obj_targets_, static_cast<const float *>(targets), targets_dev, tar_el, "H2D targets");
    if (softmax) check_labels("eval_metric", reinterpret_cast<const int32_t *>(dt), n, D, nullptr);
    const int C = kern::metric_count_columns(softmax, D);
    std::vector<unsigned long long> h(static_cast<size_t>(C) * 2, 0);   // the counters, and behind them the positives per column (auc)
    unsigned long long *dc = zeroed<unsigned long long>(d_met_counts_, h.size(), "zero metric counters");
    if (auc) kern::metric_auc(dp, dt, n, D, d_met_scratch_.ensure(kern::metric_auc_scratch_bytes(n, D)), dc + C, dc, s);
    else kern::metric_error(objective, dp, dt, n, D, dc, s);
    hip_check(hipGetLastError(), "eval_metric kernels");
    read_back(h.data(), dc, sizeof(unsigned long long) * h.size(), "D2H metric counters");
    for (int d = 0; auc && d < C; ++d) check_auc_column("eval_metric", d, h[C + d], static_cast<uint64_t>(n) - h[C + d]);
    const std::vector<uint64_t> c = metric_counts(metric, C, h.data(), h.data() + C, n);
    if (value) *value = kern::metric_value(metric, c.data(), C, static_cast<uint64_t>(n) * (softmax ? 1 : D));
    metric_counts_out(c, counts);
}

}  // namespace gbrl
