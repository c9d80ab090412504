// engine_rank.hip -- the ranking objectives on query groups (see engine.h; rank_core.h has the rule, rank.hip the kernels):
//   Engine::check_rank_group     what is refused about the objective, the model's width, the group sizes and ndcg_at before anything runs
//   Engine::rank_gradient_host   the rule on the host, query by query: the reference the kernels are held to, byte for byte
//   Engine::rank_gradient        the same on the model's device: the label pass once (kern::rank_queries), then positions, pairs and NDCG
//                                (kern::rank_rows); two waits -- one after the label pass, whose refusal names a row, one for the results
#include "engine.h"
#include "hooks.h"
#include "rank_core.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace gbrl {

const double *Engine::rank_discounts() {
    static const std::vector<double> table = [] {
        std::vector<double> t(kern::kRankMaxQuery);
        kern::rank_discount_table(t.data());
        return t;
    }();
    return table.data();
}

void Engine::check_rank_group(const char *what, const int32_t *group, int n_groups, int n, int objective, int ndcg_at, int D, const char *name) {
    const std::string w(what), g(name);
    if (!kern::rank_objective(objective))
        throw InvalidArgument(w + ": unknown objective " + std::to_string(objective) + " for a ranking call (pairwise = 4, lambdarank = 5): group belongs to the ranking objectives");
    if (D != 1) throw InvalidArgument(w + ": a ranking objective scores a row with one number: it needs output_dim == 1, the model has " + std::to_string(D));
    if (group == nullptr || n_groups <= 0) throw InvalidArgument(w + ": a ranking objective needs " + g + ", the sizes of the queries' consecutive row runs");
    if (n == 0) throw InvalidArgument(w + ": no rows (n must be positive)");
    if (ndcg_at < 0) throw InvalidArgument(w + ": ndcg_at must be positive (or 0 / None for no truncation), got " + std::to_string(ndcg_at));
    if (ndcg_at > 0 && objective == kern::kObjPairwise) throw InvalidArgument(w + ": ndcg_at truncates lambdarank's discounts; the pairwise objective has none");
    long long sum = 0;
    for (int q = 0; q < n_groups; ++q) {
        if (group[q] < 1 || group[q] > kern::kRankMaxQuery)
            throw InvalidArgument(w + ": " + g + "[" + std::to_string(q) + "] = " + std::to_string(group[q]) + " (query " + std::to_string(q) + ") is outside [1, " +
                                  std::to_string(kern::kRankMaxQuery) + "]");
        sum += group[q];
    }
    if (n > 0 && sum != n) throw InvalidArgument(w + ": the " + g + " sizes sum to " + std::to_string(sum) + ", the call has " + std::to_string(n) + " rows");
}

namespace {
std::string bad_label_message(const char *what, int32_t label, long long row) {
    return std::string(what) + ": label " + std::to_string(label) + " (row " + std::to_string(row) + ") is outside [0, " + std::to_string(kern::kRankMaxLabel) + "]";
}
const char *kBadScore = ": a prediction is not finite: no ranking gradient; the model is unchanged";
}  // namespace

void Engine::rank_gradient_host(const float *pred, const int32_t *labels, const int32_t *group, int n_groups, int n, int objective, int ndcg_at, float *grad_out,
                                float *hess_out, double *loss_out, double *ndcg_out, int32_t *pos_out, int64_t *pairs_out) {
    const char *what = "rank_gradient_host";
    if (pred == nullptr || labels == nullptr) throw InvalidArgument("rank_gradient_host: null argument");
    if (n <= 0) throw InvalidArgument("rank_gradient_host: no rows (n must be positive)");
    check_rank_group(what, group, n_groups, n, objective, ndcg_at, 1);
    const bool lambdarank = objective == kern::kObjLambdarank;
    if (loss_out != nullptr && !lambdarank)
        throw InvalidArgument("rank_gradient_host: the pairwise loss is computed on the device only (a float64 libm expression, as the logistic loss is)");
    for (int r = 0; r < n; ++r)
        if (kern::rank_bad_label(labels[r])) throw InvalidArgument(bad_label_message(what, labels[r], r));
    for (int r = 0; r < n; ++r)
        if (kern::newton_bad_pred(pred[r])) throw InvalidArgument(std::string(what) + kBadScore);
    const double *disc = rank_discounts();
    std::vector<int> pos(kern::kRankMaxQuery);
    int64_t pairs = 0;
    double ndcg_sum = 0.0;
    int r0 = 0;
    for (int q = 0; q < n_groups; r0 += group[q], ++q) {
        const int m = group[q];
        const float *s = pred + r0;
        const int32_t *l = labels + r0;
        int counts[kern::kRankMaxLabel + 1] = {0};
        for (int i = 0; i < m; ++i) {
            ++counts[l[i]];
            int p = 0;
            for (int j = 0; j < m; ++j) p += kern::rank_before(s[j], j, s[i], i) ? 1 : 0;
            pos[i] = p;
        }
        double max_dcg = 0.0;
        long long same = 0;
        for (int v = kern::kRankMaxLabel, t = 0; v >= 0; --v) {
            same += static_cast<long long>(counts[v]) * counts[v];
            for (int c = 0; c < counts[v]; ++c, ++t) max_dcg = kern::rank_add(max_dcg, kern::rank_dcg_term(v, disc, t, ndcg_at));
        }
        pairs += (static_cast<long long>(m) * m - same) / 2;
        const double inv = kern::rank_inverse(max_dcg);
        double dcg = 0.0;
        for (int i = 0; i < m; ++i) {
            dcg = kern::rank_add(dcg, kern::rank_dcg_term(l[i], disc, pos[i], ndcg_at));
            if (grad_out == nullptr && hess_out == nullptr) continue;
            double acc_g = 0.0, acc_h = 0.0;
            for (int j = 0; j < m; ++j) {
                if (lambdarank) kern::rank_accumulate<true>(s[i], l[i], pos[i], s[j], l[j], pos[j], disc, ndcg_at, inv, acc_g, acc_h);
                else kern::rank_accumulate<false>(s[i], l[i], 0, s[j], l[j], 0, disc, ndcg_at, inv, acc_g, acc_h);
            }
            if (grad_out) grad_out[r0 + i] = static_cast<float>(acc_g);
            if (hess_out) hess_out[r0 + i] = static_cast<float>(acc_h);
        }
        const double ndcg = kern::rank_ndcg(dcg, max_dcg, inv);
        ndcg_sum += ndcg;
        if (ndcg_out) ndcg_out[q] = ndcg;
        if (pos_out) std::copy(pos.begin(), pos.begin() + m, pos_out + r0);
    }
    if (pairs_out) *pairs_out = pairs;
    if (loss_out) *loss_out = 1.0 - ndcg_sum / static_cast<double>(n_groups);   // (a plain ascending sum: the device's fixed-order tree may differ in the last bits)
}

// A label vector and its query groups on the device: offsets, the row-to-query map, maxDCG and its inverse per query, the pair count.  One wait;
// a label outside [0, kRankMaxLabel] is refused naming the first such row.  The caller has run check_rank_group.
void Engine::rank_prepare(const char *what, RankSet &set, const int32_t *d_labels, const int32_t *group, int n_groups, int n, int ndcg_at) {
    hipStream_t s = stream_;
    const int Q = n_groups;
    std::vector<int32_t> off(static_cast<size_t>(Q) + 1, 0);
    set.max_group = 0;
    for (int q = 0; q < Q; ++q) {
        off[q + 1] = off[q] + group[q];
        set.max_group = std::max(set.max_group, static_cast<int>(group[q]));
    }
    set.n = n; set.Q = Q;
    const int32_t *doff = upload(set.off, off.data(), off.size(), "H2D query offsets");
    const double *ddisc = upload(d_rk_disc_, rank_discounts(), static_cast<size_t>(kern::kRankMaxQuery), "H2D discounts");
    unsigned long long stat[3] = {0ull, ~0ull, 0ull};
    unsigned long long *dstat = upload(d_rk_stat_, stat, 3, "H2D rank statistics");
    int32_t *qid = static_cast<int32_t *>(set.qid.ensure(sizeof(int32_t) * n));
    int32_t *beats = static_cast<int32_t *>(d_rk_beats_.ensure(sizeof(int32_t) * n));
    double *ideal = static_cast<double *>(d_rk_ideal_.ensure(sizeof(double) * n));
    double *max_dcg = static_cast<double *>(set.max_dcg.ensure(sizeof(double) * Q));
    double *inv = static_cast<double *>(set.inv.ensure(sizeof(double) * Q));
    kern::rank_queries(d_labels, doff, n, Q, ddisc, ndcg_at, qid, ideal, beats, max_dcg, inv, dstat, s);
    hip_check(hipGetLastError(), "rank label pass");
    read_back(stat, dstat, sizeof(stat), "D2H rank statistics");   // (the wait: off goes out of scope)
    if (stat[1] != ~0ull) {
        int32_t bad = 0;
        read_back(&bad, d_labels + stat[1], sizeof(bad), "D2H label");
        throw InvalidArgument(bad_label_message(what, bad, static_cast<long long>(stat[1])));
    }
    set.pairs = static_cast<long long>(stat[2]);
}

// Positions, pairs and NDCG of a score vector on a prepared set, enqueued on the stream (no wait): d_pos (null: the engine's scratch), dg / dh
// (each nullable), the loss sum into *d_sum and on its way to *host_sum (want_loss), the per-query NDCG into d_ndcg (null: scratch).  The flag
// word (d_rk_stat_[0]) is zeroed first and collects kRankBadPred: the caller reads it behind its wait (rank_flag_readback).
void Engine::rank_eval(const RankSet &set, int objective, int ndcg_at, const float *d_scores, const int32_t *d_labels, int32_t *d_pos, float *dg, float *dh,
                       bool want_loss, double *d_sum, double *host_sum, double *d_ndcg, bool timed) {
    hipStream_t s = stream_;
    const int n = set.n, Q = set.Q;
    const bool pairwise = objective == kern::kObjPairwise;
    unsigned long long *dstat = d_rk_stat_.as<unsigned long long>();
    hip_check(hipMemsetAsync(dstat, 0, sizeof(unsigned long long), s), "zero rank flags");
    if (d_pos == nullptr) d_pos = static_cast<int32_t *>(d_rk_pos_.ensure(sizeof(int32_t) * n));
    double *term = static_cast<double *>(d_rk_term_.ensure(sizeof(double) * n));
    const int nb = kern::staged_loss_partials(n), nbq = kern::staged_loss_partials(Q);
    double *pair_part = want_loss && pairwise ? static_cast<double *>(d_rk_part_.ensure(sizeof(double) * nb)) : nullptr;
    const bool want_ndcg = d_ndcg != nullptr || (want_loss && !pairwise);
    if (want_ndcg && d_ndcg == nullptr) d_ndcg = static_cast<double *>(d_rk_ndcg_.ensure(sizeof(double) * Q));
    double *ndcg_part = want_ndcg ? static_cast<double *>(d_rk_qpart_.ensure(sizeof(double) * nbq)) : nullptr;
    const char *names[3] = {"rank_positions", "rank_pairs", "rank_ndcg"};
    for (int k = 0; k < (timed ? 3 : 1); ++k) {   // (timed: the three kernels one by one, a phase each)
        if (timed) phase_begin();
        kern::rank_rows(objective, d_scores, d_labels, set.off.as<int32_t>(), set.qid.as<int32_t>(), set.max_dcg.as<double>(), set.inv.as<double>(), n, Q,
                        d_rk_disc_.as<double>(), ndcg_at, d_pos, term, dg, dh, pair_part, want_ndcg ? d_ndcg : nullptr, ndcg_part, dstat, s, timed ? 1 << k : 7);
        if (timed) phase_end(names[k]);
    }
    if (!want_loss) return;
    if (pairwise) finish_loss_sum(pair_part, nb, d_sum, host_sum);
    else finish_loss_sum(ndcg_part, nbq, d_sum, host_sum);
}

double Engine::rank_loss(const RankSet &set, int objective, double sum) {
    if (objective == kern::kObjPairwise) return set.pairs > 0 ? sum / static_cast<double>(set.pairs) : 0.0;
    return 1.0 - sum / static_cast<double>(set.Q);
}

void Engine::rank_gradient(const float *pred, bool pred_dev, const int32_t *labels, bool labels_dev, const int32_t *group, int n_groups, int n, int objective,
                           int ndcg_at, float *grad_out, float *hess_out, double *loss_out, double *ndcg_out, int32_t *pos_out, int64_t *pairs_out) {
    const char *what = "rank_gradient";
    if (pred == nullptr || labels == nullptr) throw InvalidArgument("rank_gradient: null argument");
    if (n <= 0) throw InvalidArgument("rank_gradient: no rows (n must be positive)");
    check_rank_group(what, group, n_groups, n, objective, ndcg_at, model.meta.output_dim);
    ensure_device();
    hipStream_t s = stream_;
    const int Q = n_groups;
    const float *dp = staged(d_rk_pred_, pred, pred_dev, static_cast<size_t>(n), "H2D scores");
    const int32_t *dl = staged(d_rk_labels_, labels, labels_dev, static_cast<size_t>(n), "H2D labels");
    RankSet &set = rk_sets_[0];
    const bool timed = profiling_ >= 2;
    ev_used_ = 0;
    ev_names_.clear();
    phase_begin();
    rank_prepare(what, set, dl, group, Q, n, ndcg_at);
    phase_end("rank_queries");   // (the label pass with its uploads and its wait)
    int32_t *dpos = pos_out != nullptr && pred_dev ? pos_out : static_cast<int32_t *>(d_rk_pos_.ensure(sizeof(int32_t) * n));
    float *dg = grad_out == nullptr ? nullptr : (pred_dev ? grad_out : static_cast<float *>(d_rk_grad_.ensure(sizeof(float) * n)));
    float *dh = hess_out == nullptr ? nullptr : (pred_dev ? hess_out : static_cast<float *>(d_rk_hess_.ensure(sizeof(float) * n)));
    double *ndcg = ndcg_out ? static_cast<double *>(d_rk_ndcg_.ensure(sizeof(double) * Q)) : nullptr;
    double *dsum = static_cast<double *>(d_rk_sums_.ensure(sizeof(double)));
    double sum = 0.0;
    rank_eval(set, objective, ndcg_at, dp, dl, dpos, dg, dh, loss_out != nullptr, dsum, &sum, ndcg, timed);
    hip_check(hipGetLastError(), "rank_gradient kernels");
    unsigned long long flag = 0;
    hip_check(hipMemcpyAsync(&flag, d_rk_stat_.as<unsigned long long>(), sizeof(flag), hipMemcpyDeviceToHost, s), "D2H rank flags");
    if (grad_out && !pred_dev) hip_check(hipMemcpyAsync(grad_out, dg, sizeof(float) * n, hipMemcpyDeviceToHost, s), "D2H gradient");
    if (hess_out && !pred_dev) hip_check(hipMemcpyAsync(hess_out, dh, sizeof(float) * n, hipMemcpyDeviceToHost, s), "D2H hessian");
    if (pos_out && !pred_dev) hip_check(hipMemcpyAsync(pos_out, dpos, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s), "D2H positions");
    if (ndcg_out) hip_check(hipMemcpyAsync(ndcg_out, ndcg, sizeof(double) * Q, hipMemcpyDeviceToHost, s), "D2H ndcg");
    hip_check(hipStreamSynchronize(s), "sync");
    phases_resolve();
    if (flag & kern::kRankBadPred) throw InvalidArgument(std::string(what) + kBadScore);
    if (pairs_out) *pairs_out = set.pairs;
    if (loss_out) *loss_out = rank_loss(set, objective, sum);
}

}  // namespace gbrl
