// engine_fit_prepared.hip -- the fit on a prepared data set (engine_step_detail.h lists the units beside it):
//   Engine::early_stop_scan / precheck_fit   the stopping rule; the refusals that need no data set
//   Engine::advance_held               rows of a held prediction advanced to every tree by the code walk, with its gradient or its loss tail
//   Engine::fit_prepared               fit()'s loop with the running prediction held and the batch never binned again, in named stages over one FitRun
//                                      (engine.h has the options).  A validation set is a second held prediction advanced after every iteration by the
//                                      walk's loss tail; a row draw is kern::sample_rows or kern::goss_select + kern::goss_sample_passes (sample_core.h: 4
//                                      bytes come back, step_prepared's body grows on the subset), a column draw the host rule per iteration; newton and
//                                      quantile leaves are engine_leaves.hip's bodies after every step; with a ranking objective (rank_core.h;
//                                      engine_rank.hip) the walk runs without a gradient tail and the rank kernels write the gradient, the hessian and both losses
#include "engine_codes_detail.h"
#include "newton_core.h"
#include "quantile_core.h"
#include "rank_core.h"
#include "sample_core.h"

namespace gbrl {

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
    std::vector<unsigned long long> vpos;
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
        move_cursor(0);
    }

    const float *stage(DevBuf &buf, const void *host_or_dev, bool on_dev, int rows) {
        return e.staged(buf, static_cast<const float *>(host_or_dev), on_dev, static_cast<size_t>(rows) * (opt.objective == kern::kObjSoftmax ? 1 : D), "H2D targets");
    }
    // the walk without a tail (a ranking objective: the rank kernels take the held scores from there)
    void walk(Held &h, int from_row, int rows) { e.advance_held(h, from_row, rows, nullptr, nullptr, nullptr, nullptr, generic, kern::kObjRmse); }
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
            dw = e.staged(e.d_fp_weights_, opt.weights, opt.weights_dev, static_cast<size_t>(n), "H2D weights");
            const WeightStats st = e.check_weights("fit_prepared (weights)", dw, n, true);
            wmax = st.max; W = st.sum;
        }
        if (v && v->weights) {
            dvw = e.staged(e.d_fp_vweights_, v->weights, v->weights_dev, static_cast<size_t>(v->ds->n), "H2D validation weights");
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
        unsigned long long flag = 0, *d = e.zeroed<unsigned long long>(e.d_newton_acc_, 1, "zero target flag");
        kern::newton_check_targets(dtar, static_cast<size_t>(n) * D, d, e.stream_);
        e.read_back(&flag, d, sizeof(flag), "D2H target flag");
        if (flag) throw InvalidArgument("fit_prepared: a logistic target is outside [0, 1] (or NaN): newton leaf values need targets in [0, 1]");
    }
    // quantile: a training target that is not finite is refused before anything changes (the bias and the leaf kernels would flag it too, a warm start
    // only after its first step)
    void check_finite_targets() {
        uint32_t flag = 0, *d = e.zeroed<uint32_t>(e.d_lq_res_, 1, "zero target flag");
        kern::leaf_quantile_check_targets(dtar, static_cast<size_t>(n) * D, d, e.stream_);
        e.read_back(&flag, d, sizeof(flag), "D2H target flag");
        if (flag) throw InvalidArgument("fit_prepared: a target is not finite: the quantile objective needs finite targets");
    }
    // auc: the positives of every validation column; a column of one class is refused before anything changes
    void count_positives() {
        const int nv = v->ds->n;
        vpos.assign(D, 0);
        unsigned long long *dc = e.zeroed<unsigned long long>(e.d_met_counts_, vpos.size(), "zero metric counters");
        kern::metric_positives(dvtar, nv, D, dc, e.stream_);
        e.read_back(vpos.data(), dc, sizeof(unsigned long long) * vpos.size(), "D2H positives");
        for (int d = 0; d < D; ++d) check_auc_column("fit_prepared (valid_targets)", d, vpos[d], static_cast<uint64_t>(nv) - vpos[d]);
    }
    // A fresh model's bias by objective, and the feature counts as step_prepared latches them.
    // With weights: sum w y / W per column and the weight W_c of a class, from column_sums' own reduction with the weight as a per-row factor.
    void set_bias(ColumnStats &stats) {
        Model &model = e.model;
        if (ranking) {   // both ranking losses are invariant to a shift of the scores
            model.bias[0] = 0.0f;
        } else if (opt.objective == kern::kObjQuantile) {   // quantile_core.h: one leaf of every row at p = 0 -- the k-th smallest target of the column, k from n
            const size_t words = kern::leaf_quantile_result_words(1, D);
            uint32_t *dres = e.zeroed<uint32_t>(e.d_lq_res_, words, "zero bias quantiles");
            void *scratch = e.d_lq_scratch_.ensure(kern::leaf_quantile_bias_scratch_bytes(n, D));
            kern::leaf_quantile_bias(dtar, n, D, d_alpha, scratch, dres, e.stream_);
            e.lq_host_.resize(words);
            hip_check(hipGetLastError(), "fit_prepared kernels");
            e.read_back(e.lq_host_.data(), dres, sizeof(uint32_t) * words, "D2H bias quantiles");
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
        d_vmetric = e.zeroed<unsigned long long>(e.d_fp_vmetric_, words, "zero metric counters");
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
        if (ranking) {   // the walk without a tail, then the rule's loss of the held scores (rank_gradient's, bit for bit); no metric goes with it
            walk(watched, 0, nv);
            e.rank_eval(e.rk_sets_[2], opt.objective, opt.ndcg_at, watched.P, reinterpret_cast<const int32_t *>(dvtar), nullptr, nullptr, nullptr, true, d_vsums + k,
                        v->rounds > 0 ? &sum : nullptr, nullptr);
        } else {
            e.advance_held(watched, 0, nv, nullptr, nullptr, dvtar, d_vpart, generic, opt.objective, dvw, d_alpha);
            e.finish_loss_sum(d_vpart, kern::staged_loss_partials(nv), d_vsums + k, v->rounds > 0 ? &sum : nullptr);
            if (opt.metric != kern::kMetricNone) measure(k);
        }
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
        const std::vector<uint64_t> c = metric_counts(opt.metric, mC, row, vpos.data(), nv);
        const double value = kern::metric_value(opt.metric, c.data(), mC, static_cast<uint64_t>(nv) * (opt.objective == kern::kObjSoftmax ? 1 : D));
        v->metric_out[k] = value;
        score[k] = opt.metric == kern::kMetricAuc ? -value : value;
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
            e.read_back(sums.data(), d_vsums, sizeof(double) * sums.size(), "D2H validation losses");
            for (int k = 0; k <= v->done; ++k) v->loss_out[k] = loss_of(sums[k], true);
            if (opt.metric != kern::kMetricNone) {   // and so did the metric's integers
                std::vector<unsigned long long> rows((static_cast<size_t>(v->done) + 1) * mC);
                e.read_back(rows.data(), d_vmetric, sizeof(unsigned long long) * rows.size(), "D2H validation metric");
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
    // ---- one iteration, in its stages: what a stage hands on is its result
    void move_cursor(int to) {   // the cursor on the batch at row `to` (past the last row: the first batch again; fitter.cpp:120, 228-231)
        start = to >= n ? 0 : to;
        bn = start + bs < n ? bs : n - start;
    }
    // 1. The batch's held prediction advanced to every tree, with its gradient in G; a ranking objective: the walk alone, then the gradient (and hessian)
    // of every row from the rows of its query -- one batch holds them all.
    void gradient() {
        e.phase_begin();
        if (ranking) walk(train, start, bn);   // (no fused gradient: predict_continue_prepared's launch)
        else e.advance_held(train, start, bn, dtar, G, nullptr, nullptr, generic, opt.objective, dw, d_alpha);
        e.phase_end("continue_codes");
        if (!ranking) return;
        e.phase_begin();
        e.rank_eval(e.rk_sets_[1], opt.objective, opt.ndcg_at, train.P, reinterpret_cast<const int32_t *>(dtar), nullptr, G, H, false, nullptr, nullptr, nullptr);
        unsigned long long flag = 0;
        e.read_back(&flag, e.d_rk_stat_.as<unsigned long long>(), sizeof(flag), "D2H rank flags", "rank_gradient");
        if (flag & kern::kRankBadPred) throw InvalidArgument("fit_prepared: a prediction is not finite: no ranking gradient; the model keeps the trees grown so far");
    }
    // 2. The rows the tree is grown on with their gradient rows: the batch, or what a draw kept of it (kept: rows is d_srows).  A draw that keeps no
    // row takes the whole batch.  goss: the selection's tau stays on the device.
    struct Drawn { const float *g; const int32_t *rows; int m; bool kept; };
    Drawn draw(int trees, const kern::GossPlan &plan) {
        hipStream_t s = e.stream_;
        const Drawn batch{G, bn == n ? nullptr : d_iota + start, bn, false};
        if (!sampled && !goss) return batch;
        e.phase_begin();
        if (sampled) {
            kern::sample_rows(start, bn, kern::sample_threshold(opt.subsample), opt.seed, trees, G, D, d_srows, Gs, d_sscratch, s);
        } else {
            const kern::GossScratch gs = kern::goss_scratch(d_sscratch, bn);
            kern::goss_select(bn, plan.k, G, D, gs, s);
            e.phase_end("goss_select"); e.phase_begin();
            kern::goss_sample_passes(start, bn, plan.thr, plan.amp, opt.seed, trees, gs, G, D, d_srows, d_sfactor, Gs, dw, d_eff, s);
        }
        int32_t kept = 0;
        e.read_back(&kept, d_sscratch, sizeof(kept), "D2H sample count", sampled ? "sample_rows" : "sample_goss");
        return kept > 0 ? Drawn{Gs, d_srows, kept, true} : batch;
    }
    // 3. The step, on the columns of its own draw (none: every column).
    void step(const Drawn &d, int trees) {
        if (colsampled) kern::sample_cols(ds->F, opt.colsample, opt.seed, trees, e.fit_cols_);
        e.step_prepared_run(ds, d.g, d.rows, d.m, colsampled ? e.fit_cols_.data() : nullptr, colsampled ? static_cast<int>(e.fit_cols_.size()) : 0);
    }
    // 4. The new tree's leaves.  ranking + newton: the sums of the g and h the tree was grown on, from their buffers, with room for the largest query.
    // newton: from the rows it was grown on, at the held prediction over the trees before it; the kept rows of a one-side draw carry fl32(w * factor),
    // with room for fl32(wmax * amp).  quantile: the level's order statistic of the residuals of those rows.
    void update_leaves(const Drawn &d, float goss_amp) {
        const int t = e.model.meta.n_trees - 1;
        if (opt.leaf_update == kern::kLeafNewton && ranking)
            return e.newton_leaves_run("fit_prepared", ds, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), nullptr, 0}, n, G, H, /*abs_index=*/true,
                                       kern::kObjGiven, t, opt.leaf_l2, generic, nullptr, nullptr, nullptr, nullptr, static_cast<float>(e.rk_sets_[1].max_group));
        const kern::CodeRows cr{ds->prep.d_codes, ds->n, ds->code_groups(), d.kept ? d_srows : nullptr, d.kept ? 0 : start};
        if (opt.leaf_update == kern::kLeafNewton) {
            const bool amplified = d.kept && goss;
            e.newton_leaves_run("fit_prepared", ds, cr, d.m, train.P, dtar, /*abs_index=*/true, opt.objective, t, opt.leaf_l2, generic, nullptr, nullptr, nullptr,
                                amplified ? d_eff : dw, amplified ? kern::obj_weighted(dw ? wmax : 1.0f, goss_amp) : wmax);
        } else if (opt.leaf_update == kern::kLeafQuantile)
            e.quantile_leaves_run("fit_prepared", ds, cr, d.m, train.P, dtar, /*abs_index=*/true, d_alpha, t, generic, nullptr, nullptr, nullptr);
    }
    // One tree on the batch under the cursor.  Both draws are those of the tree count before the step.
    void iterate() {
        const int trees = e.model.meta.n_trees;
        const kern::GossPlan plan = goss ? kern::goss_plan(bn, opt.goss_top, opt.goss_other) : kern::GossPlan{};
        e.begin_step_profile();
        gradient();
        const Drawn d = draw(trees, plan);
        step(d, trees);
        update_leaves(d, plan.amp);
        move_cursor(start + bn);   // 5.
    }
    // Every batch to the end; the loss on the whole data set (fitter.cpp:246-251).  rmse: from the gradient of every row, written by the same
    // launches, as fit() computes it; an objective: from the held prediction by the stand-alone kernel, the loss tail's partials and sum.  With
    // weights rmse takes the second way too (G would hold w g, and sum (w g)^2 is not the weighted loss): objective_gradient's loss, bit for bit.
    float final_loss(ColumnStats &stats) {
        const bool rmse = opt.objective == kern::kObjRmse && dw == nullptr;
        for (int b0 = 0; b0 < n; b0 += bs)
            if (ranking) walk(train, b0, std::min(bs, n - b0));
            else e.advance_held(train, b0, std::min(bs, n - b0), rmse ? dtar : nullptr, rmse ? G + static_cast<size_t>(b0) * D : nullptr, nullptr, nullptr, generic,
                                opt.objective, nullptr, d_alpha);
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
