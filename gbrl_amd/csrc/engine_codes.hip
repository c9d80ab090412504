// engine_codes.hip -- a prepared data set's bin codes in the model's terms, from the host rule up to the walk (engine_step_detail.h lists the units beside it):
//   Engine::condition_bins             every numeric condition of the model as a bin index of a threshold table (host only)
//   sync_code_bins / check_code_range  the same for ONE data set, appended split row by split row, and the refusal of a range the codes cannot express
//   sync_code_tables                   device copies of the bins and of the mirror's packed conditions / greedy node records with the bin as
//                                      their second word (appended like the originals: a loop that adds a tree per iteration converts that tree only)
//   Engine::predict_continue_prepared  predict_continue without the observations (kern::predict_continue_codes)
//   Engine::predict_leaves_prepared / leaf_counts_prepared   where the rows of a data set land, and the rows per leaf (kern::predict_leaves_codes / leaf_counts_codes)
//   Engine::predict_staged_prepared / staged_loss_prepared   every prefix of the ensemble in one walk over the codes (kern::predict_staged_codes)
//   read_back / subset_rows / resolve_tree / join_tail_phase   what the calls on a data set share (engine.h)
//
// The rule.  code(r, f) = #{b : thr[f][b] < obs[r, f]} (-0.0 == +0.0; NaN lies below every threshold: code 0).  For a condition x > v whose v
// equals some thr[f][b] let bin = #{b : thr[f][b] < v}.  x > v: every threshold below v, and v itself, is below x, so code >= bin + 1.
// x <= v: only thresholds below v can be below x, so code <= bin.  Hence x > v <=> code > bin, with duplicated thresholds and in any order.
// It does not hold for a v that is not among the feature's thresholds: such a condition is refused (Unsupported), never approximated.
#include "engine_codes_detail.h"

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
    // the packed conditions of the mirror (cond_pack_host_, detail::packed_condition) with the threshold word replaced by the bin
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
        const size_t n_nodes = grd_.nodes.size() / 4;
        if (code_nodes_ > n_nodes) code_nodes_ = code_up_nodes_ = 0;
        code_nodes_host_.resize(n_nodes * 4);
        for (size_t k = code_nodes_; k < n_nodes; ++k) {
            int32_t *nd = &code_nodes_host_[k * 4];
            std::memcpy(nd, &grd_.nodes[k * 4], 16);
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

void Engine::read_back(void *host, const void *dev, size_t bytes, const char *what, const char *phase) {
    hip_check(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream_), what);
    if (phase) phase_end(phase);
    hip_check(hipStreamSynchronize(stream_), "sync");
}

const int32_t *Engine::subset_rows(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m) {
    return rows ? checked_rows(d_sub_rows_, d_rows_mm_, rows, rows_dev, m, ds->n, stream_) : nullptr;
}

int Engine::resolve_tree(const char *what, int tree) const {
    const int T = model.meta.n_trees;
    if (T == 0) throw InvalidArgument(std::string(what) + ": the model has no trees");
    if (tree < -1 || tree >= T) throw InvalidArgument(std::string(what) + ": tree " + std::to_string(tree) + " is outside the model's " + std::to_string(T) + " trees (-1: the last)");
    return tree == -1 ? T - 1 : tree;
}

void Engine::join_tail_phase(const char *name, const char *marker, bool value) {
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, ev_pool_[ev_used_ - 1].first, ev_pool_[ev_used_ - 1].second), "hipEventElapsedTime");
    --ev_used_;
    ev_names_.pop_back();
    phases_.emplace_back(name, ms);
    phases_.emplace_back(marker, value ? 1.f : 0.f);
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
    check_row_count("predict_continue_prepared", "base", rows, m, ds->n, "continue");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, "predict_continue_prepared", start_tree, stop);
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
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

// Extension: where the rows of a data set land (kern::predict_leaves_codes / kern::leaf_counts_codes).  The refusals that both forms share, in
// predict_continue_prepared's order and with its messages; returns the resolved stop.  Leaf routing reads no value: no output width limit.
int Engine::check_leaves_prepared(const char *what, const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int start_tree, int stop_tree) {
    const std::string w(what);
    const int T = model.meta.n_trees;
    check_prepared_dataset(what, ds);
    if (start_tree < 0 || stop_tree < 0) throw InvalidArgument("invalid tree range");
    if (T == 0) throw InvalidArgument(w + ": the model has no trees");
    const int stop = stop_tree == 0 ? T : stop_tree;   // (0 means n_trees)
    if (stop > T || start_tree >= stop) throw InvalidArgument(w + ": invalid tree range");
    check_row_count(what, "the call", rows, m, ds->n, "route");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, what, start_tree, stop);
    return stop;
}

void Engine::predict_leaves_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int start_tree, int stop_tree, int32_t *out,
                                     bool out_dev) {
    const char *what = "predict_leaves_prepared";
    if (out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const int stop = check_leaves_prepared(what, ds, rows, rows_dev, m, start_tree, stop_tree);
    if (static_cast<int64_t>(m) * (stop - start_tree) >= (int64_t(1) << 31))
        throw Unsupported(std::string(what) + ": rows x trees >= 2^31 indices: slice the tree range, or pass rows= to route a subset");
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const size_t out_bytes = sizeof(int32_t) * static_cast<size_t>(m) * (stop - start_tree);
    int32_t *dl = out_dev ? out : static_cast<int32_t *>(d_leaves_out_.ensure(out_bytes));
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::predict_leaves_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, start_tree, stop, dl,
                               hooks::on(hooks::LEAVES_GENERIC), stream_);
    finish("predict_leaves_prepared launch", "predict", {{out_dev ? nullptr : out, dl, out_bytes, "D2H leaves"}});
}

void Engine::leaf_counts_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int start_tree, int stop_tree, int64_t *counts_out) {
    const char *what = "leaf_counts_prepared";
    if (counts_out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const int stop = check_leaves_prepared(what, ds, rows, rows_dev, m, start_tree, stop_tree);
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const size_t L = static_cast<size_t>(model.meta.n_leaves);
    uint32_t *dcounts = zeroed<uint32_t>(d_leaf_counts_, std::max<size_t>(L, 1), "zero leaf counters");
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::leaf_counts_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, model.tree_indices.data(), m, start_tree,
                            stop, dcounts, hooks::on(hooks::LEAVES_GENERIC), stream_);
    std::vector<uint32_t> h(L);
    finish("leaf_counts_prepared launch", "predict", {{h.data(), dcounts, sizeof(uint32_t) * L, "D2H leaf counts"}});
    for (size_t l = 0; l < L; ++l) counts_out[l] = static_cast<int64_t>(h[l]);   // (m < 2^31 rows: a counter cannot wrap)
}

// Extension: every prefix [0, stops[s]) of the ensemble in one walk over the data set's codes (kern::predict_staged_codes).  The refusals that both
// forms share, in predict_continue_prepared's order; the walked range is [0, last stop).
void Engine::check_staged_prepared(const char *what, const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const int32_t *stops, int n_stops,
                                   const char *noun) {
    check_prepared_dataset(what, ds);
    if (model.meta.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    check_stops(stops, n_stops);
    check_row_count(what, noun, rows, m, ds->n, "evaluate");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, what, 0, stops[n_stops - 1]);
}

void Engine::predict_staged_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const int32_t *stops, int n_stops, float *out,
                                     bool out_dev) {
    const char *what = "predict_staged_prepared";
    if (out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    check_staged_prepared(what, ds, rows, rows_dev, m, stops, n_stops, "the call");
    const int D = model.meta.output_dim;
    if (static_cast<int64_t>(n_stops) * m * D >= (int64_t(1) << 31))
        throw Unsupported(std::string(what) + ": n_stops x rows x output_dim >= 2^31 elements: pass fewer stops, or rows= to evaluate a subset");
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const kern::StagedStops dstops = stage_stops(stops, n_stops);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(n_stops) * m * D;
    float *dout = out_dev ? out : static_cast<float *>(d_pout_.ensure(out_bytes));
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::StagedCodesOut o{};
    o.out = dout;
    kern::predict_staged_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, dstops, o, kern::kObjRmse,
                               hooks::on(hooks::STAGED_GENERIC), stream_);
    finish("predict_staged_prepared launch", "predict", {{out_dev ? nullptr : out, dout, out_bytes, "D2H preds"}});
}

void Engine::staged_loss_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const void *targets, bool targets_dev, int objective,
                                  const float *alpha, const float *weights, bool weights_dev, int metric, const int32_t *stops, int n_stops, double *loss_out,
                                  double *metric_out, int64_t *counts_out) {
    const char *what = "staged_loss_prepared";
    const std::string w(what);
    if (targets == nullptr) throw InvalidArgument("Cannot call " + w + " without targets!");
    if (loss_out == nullptr) throw InvalidArgument(w + ": no place for the result");
    check_staged_prepared(what, ds, rows, rows_dev, m, stops, n_stops, "targets");
    const int D = model.meta.output_dim;
    check_objective(what, objective, D);
    check_alpha(what, objective, alpha, D, weights != nullptr);
    if (metric != kern::kMetricNone) {
        check_metric(what, objective, metric);
        if (metric == kern::kMetricAuc)
            throw Unsupported(w + ": auc is not evaluated per stage (it needs a sort per stage): eval_metric on a stage of predict_staged_prepared gives it");
        if (weights != nullptr)
            throw Unsupported(w + ": weights with eval_metric is not supported (the metrics count rows; weighted metrics are not implemented)");
        if (metric_out == nullptr || counts_out == nullptr) throw InvalidArgument(w + ": no place for the metric");
    }
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const kern::StagedStops dstops = stage_stops(stops, n_stops);
    const size_t tar_el = objective == kern::kObjSoftmax ? static_cast<size_t>(m) : static_cast<size_t>(m) * D;
    const float *dt = staged(d_staged_targets_, static_cast<const float *>(targets), targets_dev, tar_el, "H2D targets");
    if (objective == kern::kObjSoftmax) check_labels(what, reinterpret_cast<const int32_t *>(dt), m, D, nullptr);
    const float *dw = weights ? staged(d_staged_weights_, weights, weights_dev, static_cast<size_t>(m), "H2D weights") : nullptr;
    const double W = dw ? check_weights("staged_loss_prepared (weights)", dw, m, true).sum : static_cast<double>(m);
    const int nb = kern::staged_loss_partials(m), C = kern::metric_count_columns(objective == kern::kObjSoftmax, D);
    kern::StagedCodesOut o{};
    o.targets = dt; o.weights = dw;
    o.alpha = alpha ? upload(d_lq_alpha_, alpha, static_cast<size_t>(D), "H2D levels") : nullptr;
    o.part = static_cast<double *>(d_staged_part_.ensure(sizeof(double) * static_cast<size_t>(n_stops) * nb));
    o.sums = static_cast<double *>(d_staged_sums_.ensure(sizeof(double) * n_stops));
    if (metric != kern::kMetricNone) {
        o.cnt_part = static_cast<unsigned long long *>(d_staged_cnt_.ensure(sizeof(unsigned long long) * static_cast<size_t>(n_stops) * C * nb));
        o.counts = static_cast<unsigned long long *>(d_staged_counts_.ensure(sizeof(unsigned long long) * static_cast<size_t>(n_stops) * C));
    }
    if (const size_t stored = kern::staged_codes_row_scratch(m, D, objective))
        o.row_scratch = static_cast<float *>(d_staged_rows_.ensure(sizeof(float) * stored));
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::predict_staged_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, dstops, o, objective,
                               hooks::on(hooks::STAGED_GENERIC), stream_);
    std::vector<double> sums(n_stops);
    std::vector<unsigned long long> counts(o.counts ? static_cast<size_t>(n_stops) * C : 0);
    finish("staged_loss_prepared launch", "predict", {{sums.data(), o.sums, sizeof(double) * n_stops, "D2H loss sums"},
                                                     {counts.empty() ? nullptr : counts.data(), o.counts, sizeof(unsigned long long) * counts.size(), "D2H metric counters"}});
    for (int i = 0; i < n_stops; ++i) loss_out[i] = mean_loss(objective, sums[i], W);
    if (o.counts == nullptr) return;
    const uint64_t cells = static_cast<uint64_t>(m) * (objective == kern::kObjSoftmax ? 1 : D);
    for (int i = 0; i < n_stops; ++i) {
        const std::vector<uint64_t> c = metric_counts(metric, C, counts.data() + static_cast<size_t>(i) * C, nullptr, m);
        metric_out[i] = kern::metric_value(metric, c.data(), C, cells);
        for (int d = 0; d < C; ++d) counts_out[static_cast<size_t>(i) * C + d] = static_cast<int64_t>(c[d]);
    }
}

}  // namespace gbrl
