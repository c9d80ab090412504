// engine_codes.hip -- a prepared data set's bin codes in the model's terms, from the host rule up to the walk (engine_step_detail.h lists the units beside it):
//   Engine::condition_bins             every numeric condition of the model as a bin index of a threshold table (host only)
//   sync_code_bins / check_code_range  the same for ONE data set, appended split row by split row, and the refusal of a range the codes cannot express
//   sync_code_tables                   device copies of the bins and of the mirror's packed conditions / greedy node records with the bin as
//                                      their second word (appended like the originals: a loop that adds a tree per iteration converts that tree only)
//   Engine::predict_continue_prepared  predict_continue without the observations (kern::predict_continue_codes)
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

}  // namespace gbrl
