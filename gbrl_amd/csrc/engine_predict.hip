// engine_predict.hip -- GBRL::predict with its family: predict_continue, predict_staged / staged_loss, predict_leaves / leaf_counts (and
// refit_leaves in engine_refit.hip).  The device mirror of the ensemble that they read is engine_mirror.hip's.  A call is a sequence of
// stages, each written once:
//   its own argument checks and check_batch, in the call's order (all of them before a device is needed)
//   stage_batch      device, event pool, mirror; then the `inputs` phase: observations up, ids checked and uploaded or cells encoded
//   stage_targets / stage_stops and the call's result buffer, still inside `inputs`
//   mirror_view      what the kernels read of the model (engine_mirror.hip); predict() alone adds the packed-code book, the partial sums and the chain slots
//   the call's kernel
//   finish           launch error, end of the key phase, read-backs, one wait, phase times
#include "engine.h"
#include "hooks.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace gbrl {

constexpr int kChainMinTrees = 512;   // below: the tiled kernels are as fast (measured, scripts/predict_latency.py)
constexpr int kChainMaxRows = 8192;   // 5000 rows x 20 000 trees: 1.58 -> 0.88 ms, 8192 x 5000: 0.39 -> 0.32 ms; beyond, the leaf search alone costs as much

// ============================================================================================ the stages of a call
// GBRL::predict, gbrl.cpp:378-390.  The feature counts are the caller's until the first tree exists.
void Engine::check_batch(const PredictBatch &b, bool has_result, bool width_limit) {
    gbrl_hip_metadata &md = model.meta;
    if (md.iteration == 0) { md.n_num_features = b.n_num; md.n_cat_features = b.n_cat; }
    if (b.n_num + b.n_cat != md.input_dim) throw InvalidArgument("Incompatible dataset");
    if (b.n_num != md.n_num_features || b.n_cat != md.n_cat_features) throw InvalidArgument("Incompatible dataset");
    if (b.n <= 0 || !has_result) throw InvalidArgument("Cannot call predict without observations!");
    if (b.n_num > 0 && b.obs == nullptr) throw InvalidArgument("Cannot call predict without observations!");
    if (b.n_cat > 0 && b.cat == nullptr && b.cat_ids == nullptr) throw InvalidArgument("Cannot call predict without observations!");
    if (md.output_dim > 128 && width_limit) throw Unsupported("predict: output_dim > 128");
}

// pre-encoded ids (encode_categorical): valid only for the dictionary they were made from
void Engine::check_dict_token(const PredictBatch &b) {
    if (b.n_cat <= 0 || b.cat_ids == nullptr) return;
    sync_cat_dict();   // (nothing to do behind sync_model_to_device)
    if (b.token == nullptr || *b.token != cat_dict_token())
        throw InvalidArgument("predict: the categorical ids were encoded for another category dictionary (the model has grown or is a different one): encode the batch again");
}

// like predict_continue, no reference behaviour to mirror: a stage the ensemble does not hold is an error, reported before the device is touched
void Engine::check_stops(const int32_t *stops, int n_stops) const {
    const int T = model.meta.n_trees;
    if (stops == nullptr || n_stops <= 0) throw InvalidArgument("staged evaluation: stops is empty");
    for (int i = 0; i < n_stops; ++i) {
        const int k = stops[i];
        if (k < 0 || k > T) throw InvalidArgument("staged evaluation: a stop is out of bounds! Got " + std::to_string(k) + ", but valid range is [0, " + std::to_string(T) + "]");
        if (i > 0 && k <= stops[i - 1]) throw InvalidArgument("staged evaluation: stops must be strictly ascending");
    }
}

// like predict_continue, no reference behaviour to mirror: a range the ensemble does not hold is an error, and so is an empty one (there is
// no index to return)
int Engine::check_leaves_range(int start_tree, int stop_tree) const {
    const int T = model.meta.n_trees;
    if (start_tree < 0 || stop_tree < 0) throw InvalidArgument("invalid tree range");
    if (T == 0) throw InvalidArgument("predict_leaves: the model has no trees");
    const int stop = stop_tree == 0 ? T : stop_tree;
    if (stop > T || start_tree >= stop) throw InvalidArgument("predict_leaves: invalid tree range");
    return stop;
}

Engine::StagedBatch Engine::stage_batch(const PredictBatch &b) {
    ensure_device();
    ev_used_ = 0;
    ev_names_.clear();
    sync_model_to_device();
    phase_begin();
    StagedBatch d{b.obs, nullptr};
    if (b.n_num > 0 && !b.obs_dev) d.obs = upload(d_pobs_, b.obs, static_cast<size_t>(b.n) * b.n_num, "H2D obs");
    if (b.n_cat > 0 && b.cat_ids != nullptr) {
        check_dict_token(b);   // (the _encoded predicts refuse a stale token here, behind the mirror; the leaf calls have refused it before the device)
        d.cat = b.ids_dev ? b.cat_ids : upload(d_pcat_in_, b.cat_ids, static_cast<size_t>(b.n) * b.n_cat, "H2D cat ids");
    } else if (b.n_cat > 0) {
        d.cat = encode_categorical_batch(b.cat, b.cat_dev, b.n, b.n_cat);
    }
    return d;
}

const float *Engine::stage_targets(const float *targets, bool on_device, int n) {
    return on_device ? targets : upload(d_staged_targets_, targets, static_cast<size_t>(n) * model.meta.output_dim, "H2D targets");
}

// the stops table lives on the device (the pageable copy has left the host array when the call returns)
kern::StagedStops Engine::stage_stops(const int32_t *stops, int n_stops) {
    return kern::StagedStops{upload(d_staged_stops_, stops, n_stops, "H2D stops"), n_stops, stops[n_stops - 1]};
}

void Engine::finish(const char *launch, const char *phase, std::initializer_list<ReadBack> results) {
    hipStream_t s = stream_;
    hip_check(hipGetLastError(), launch);
    phase_end(phase, /*key=*/true);
    for (const ReadBack &r : results)
        if (r.host != nullptr) hip_check(hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, s), r.what);
    hip_check(hipStreamSynchronize(s), "sync");
    phases_resolve();
}

// ======================================================================================================== the calls
void Engine::predict(const float *obs, bool obs_dev, const char *cat, bool cat_dev, int n, int n_num, int n_cat, int start_tree,
                     int stop_tree, float *out, bool out_dev) {
    run_predict(PredictBatch{obs, obs_dev, cat, cat_dev, nullptr, false, nullptr, n, n_num, n_cat}, start_tree, stop_tree, out, out_dev);
}

void Engine::predict_encoded(const float *obs, bool obs_dev, const int32_t *cat_ids, bool ids_dev, uint64_t token, int n, int n_num, int n_cat,
                             int start_tree, int stop_tree, float *out, bool out_dev) {
    if (n_cat > 0 && cat_ids == nullptr) throw InvalidArgument("Cannot call predict without observations!");
    run_predict(PredictBatch{obs, obs_dev, nullptr, false, cat_ids, ids_dev, &token, n, n_num, n_cat}, start_tree, stop_tree, out, out_dev);
}

void Engine::run_predict(const PredictBatch &b, int start_tree, int stop_tree, float *out, bool out_dev) {
    const gbrl_hip_metadata &md = model.meta;
    const int n = b.n, D = md.output_dim;
    check_batch(b, out != nullptr, /*width_limit=*/true);
    if (start_tree < 0 || stop_tree < 0) throw InvalidArgument("invalid tree range");   // the reference would index out of bounds
    // predict_cpu, predictor.cpp:127-141
    int stop = stop_tree;
    if (md.n_trees == 0 || stop > md.n_trees || model.opts.empty()) { start_tree = 0; stop = 0; }
    else if (stop == 0) stop = md.n_trees;
    // an empty or inverted range walks no tree: predict_cpu's loops run from start to stop (predictor.cpp:139-163), the result is the bias
    if (start_tree >= stop) { start_tree = 0; stop = 0; }
    const StagedBatch d = stage_batch(b);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(n) * D;
    float *dout = out_dev ? out : static_cast<float *>(d_pout_.ensure(out_bytes));
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::PredictModel pm = mirror_view();
    // Packed-code path: large batches of rows the fp32 register-tile kernel does not take (categorical columns, more than 128 or an
    // odd number of features, unaligned rows).  The code book follows the model; the rows are packed inside kern::predict.
    {
        const char *no_pc = hooks::raw(hooks::PREDICT_NO_PC), *no_reg = hooks::raw(hooks::PREDICT_NO_REG), *mr = hooks::raw(hooks::PREDICT_REG_MIN_ROWS);
        const int min_rows = mr ? std::atoi(mr) : 32768;
        const bool fp32_takes_it = b.n_cat == 0 && b.n_num <= 128 && (b.n_num & 3) == 0 && (reinterpret_cast<uintptr_t>(d.obs) & 15) == 0 && !(no_reg && no_reg[0] == '1');
        // (the levels of the swizzled records, whatever PREDICT_OBL1 has made of pm.obl2_maxd)
        if (!(no_pc && no_pc[0] == '1') && !in_fit_ && pm.values_sw != nullptr && model.oblivious() && n >= min_rows && !fp32_takes_it &&
            kern::predict_pc_shape_ok(kern::obl2_levels(md.max_depth), D) && ensure_pc_book(b.n_num, b.n_cat)) {
            pm.pc_cond = m_pc_cond_.as<int32_t>();
            pm.pc_thr = m_pc_thr_.as<float>();
            pm.pc_thr_off = m_pc_thr_off_.as<int32_t>();
            pm.pc_cat_slot = m_pc_cat_slot_.as<int32_t>();
            pm.pc_word_cols = m_pc_word_cols_.as<int32_t>();
            pm.pc_wn = pc_wn_; pm.pc_nw = pc_nw_; pm.pc_row_words = pc_row_words_; pm.pc_iters = pc_iters_;
            pm.pc_rows = static_cast<uint32_t *>(d_pc_rows_.ensure(static_cast<size_t>(n) * pc_row_words_ * sizeof(uint32_t)));
        }
    }
    // small batches: scratch for up to 64 partial sums per output (tree ranges spread over blocks, kern::predict)
    // (not inside fit(): its gradients follow the reference's per-row tree-order chain at every batch size)
    pm.par_th = md.par_th;
    // (nor for a model whose file cleared parallel_predict: the reference then runs the chain for every batch, predictor.cpp:144)
    const char *nosplit = hooks::raw(hooks::PREDICT_NOSPLIT);   // measurement hook: no partial sums over tree ranges
    if (!in_fit_ && model.parallel_predict && n <= 64 * 256 && stop - start_tree >= 128 && !(nosplit && nosplit[0] == '1')) {
        pm.partial_floats = std::min<size_t>(static_cast<size_t>(64) * n * D, size_t(16) << 20);
        pm.partial = static_cast<float *>(d_pred_partial_.ensure(pm.partial_floats * sizeof(float)));
    }
    // Up to 8192 rows against a large tree range: leaf search spread over the chip + one multiply-add chain per (row, output)
    // (kern::predict_chain: the bits of the one-chain-per-row kernels, so fit() uses it too).  Measured against the tiled kernels'
    // 80 ns per tree: 1024 rows x 20 000 trees 1.59 -> 0.27 ms, 4096 rows 1.58 -> 0.64 ms; beyond ~8192 rows the leaf search
    // alone costs what the tiled kernel does.  GBRL_HIP_PREDICT_CHAIN=0 / 1: never / whenever the shape is covered (tests).
    {
        const int trees = stop - start_tree;
        bool want = (n <= kChainMaxRows && trees >= kChainMinTrees) || (n <= 1024 && trees >= 128);
        if (const char *e = hooks::raw(hooks::PREDICT_CHAIN)) want = e[0] == '1' ? (n <= 64 * 256 && trees >= 1) : false;
        if (want) {
            const size_t ints = kern::predict_chain_slot_ints(n, trees);
            if (ints <= (size_t(1) << 27)) {
                pm.slot_ints = ints;
                pm.slots = static_cast<int32_t *>(d_pred_slots_.ensure(ints * sizeof(int32_t)));
            }
        }
    }
    kern::predict(pm, d.obs, b.n_num, d.cat, b.n_cat, n, start_tree, stop, dout, stream_);
    finish("predict launch", "predict", {{out_dev ? nullptr : out, dout, out_bytes, "D2H preds"}});
}

// Extension: `base` is the prediction over the trees [0, start_tree); `out` (which may be `base`) gets it carried through [start_tree, stop_tree).
// See kern::predict_continue for the arithmetic.
void Engine::predict_continue(const float *obs, bool obs_dev, const char *cat, bool cat_dev, int n, int n_num, int n_cat, int start_tree,
                              int stop_tree, const float *base, bool base_dev, float *out, bool out_dev) {
    run_continue(PredictBatch{obs, obs_dev, cat, cat_dev, nullptr, false, nullptr, n, n_num, n_cat}, start_tree, stop_tree, base, base_dev, out, out_dev);
}

void Engine::predict_continue_encoded(const float *obs, bool obs_dev, const int32_t *cat_ids, bool ids_dev, uint64_t token, int n, int n_num,
                                      int n_cat, int start_tree, int stop_tree, const float *base, bool base_dev, float *out, bool out_dev) {
    if (n_cat > 0 && cat_ids == nullptr) throw InvalidArgument("Cannot call predict without observations!");
    run_continue(PredictBatch{obs, obs_dev, nullptr, false, cat_ids, ids_dev, &token, n, n_num, n_cat}, start_tree, stop_tree, base, base_dev, out, out_dev);
}

void Engine::run_continue(const PredictBatch &b, int start_tree, int stop_tree, const float *base, bool base_dev, float *out, bool out_dev) {
    const gbrl_hip_metadata &md = model.meta;
    check_batch(b, out != nullptr, /*width_limit=*/true);
    if (start_tree < 0 || stop_tree < 0) throw InvalidArgument("invalid tree range");
    // predict_continue has no reference behaviour to mirror: a range the ensemble does not hold is an error, never a silent no-op (a cache
    // that is handed back unchanged is a stale prediction)
    if (base == nullptr) throw InvalidArgument("predict_continue: no base prediction");
    const int stop = stop_tree == 0 ? md.n_trees : stop_tree;   // (0 means n_trees)
    if (stop > md.n_trees || start_tree > stop) throw InvalidArgument("predict_continue: invalid tree range");
    const StagedBatch d = stage_batch(b);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(b.n) * md.output_dim;
    float *dout = out_dev ? out : static_cast<float *>(d_pout_.ensure(out_bytes));
    const float *dbase = base;
    if (!base_dev) {   // a base in host memory is copied into the output buffer and continued in place
        hip_check(hipMemcpyAsync(dout, base, out_bytes, hipMemcpyHostToDevice, stream_), "H2D base");
        dbase = dout;
    }
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::predict_continue(mirror_view(), d.obs, b.n_num, d.cat, b.n_cat, b.n, start_tree, stop, dbase, dout, hooks::on(hooks::CONTINUE_GENERIC), stream_);
    finish("predict_continue launch", "predict", {{out_dev ? nullptr : out, dout, out_bytes, "D2H preds"}});
}

// Extension: every prefix [0, stops[s]) of the ensemble in one walk (kern::predict_staged): one chain per (row, output), never sliced over
// tree ranges.  The stops table is the range.
void Engine::predict_staged(const float *obs, bool obs_dev, const char *cat, bool cat_dev, int n, int n_num, int n_cat, const int32_t *stops, int n_stops,
                            float *out, bool out_dev) {
    const PredictBatch b{obs, obs_dev, cat, cat_dev, nullptr, false, nullptr, n, n_num, n_cat};
    check_batch(b, out != nullptr, /*width_limit=*/true);
    check_stops(stops, n_stops);
    const StagedBatch d = stage_batch(b);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(n) * model.meta.output_dim * static_cast<size_t>(n_stops);
    float *dout = out_dev ? out : static_cast<float *>(d_pout_.ensure(out_bytes));
    const kern::StagedStops dstops = stage_stops(stops, n_stops);
    phase_end("inputs"); phase_begin(/*key=*/true);
    kern::predict_staged(mirror_view(), d.obs, n_num, d.cat, n_cat, n, dstops, dout, nullptr, nullptr, nullptr, hooks::on(hooks::STAGED_GENERIC), stream_);
    finish("predict_staged launch", "predict", {{out_dev ? nullptr : out, dout, out_bytes, "D2H preds"}});
}

void Engine::staged_loss(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *targets, bool targets_dev, int n, int n_num, int n_cat,
                         const int32_t *stops, int n_stops, double *loss_out) {
    const PredictBatch b{obs, obs_dev, cat, cat_dev, nullptr, false, nullptr, n, n_num, n_cat};
    check_batch(b, /*has_result=*/true, /*width_limit=*/true);   // (the results are n_stops doubles, checked below)
    check_stops(stops, n_stops);
    if (targets == nullptr) throw InvalidArgument("Cannot call staged_loss without targets!");
    if (loss_out == nullptr) throw InvalidArgument("staged_loss: no output array");
    const StagedBatch d = stage_batch(b);
    const kern::StagedStops dstops = stage_stops(stops, n_stops);
    const float *dtargets = stage_targets(targets, targets_dev, n);
    phase_end("inputs"); phase_begin(/*key=*/true);
    double *dpart = static_cast<double *>(d_staged_part_.ensure(sizeof(double) * static_cast<size_t>(n_stops) * kern::staged_loss_partials(n)));
    double *dsums = static_cast<double *>(d_staged_sums_.ensure(sizeof(double) * n_stops));
    kern::predict_staged(mirror_view(), d.obs, n_num, d.cat, n_cat, n, dstops, nullptr, dtargets, dpart, dsums, hooks::on(hooks::STAGED_GENERIC), stream_);
    std::vector<double> sums(n_stops);
    finish("predict_staged launch", "predict", {{sums.data(), dsums, sizeof(double) * n_stops, "D2H loss sums"}});
    for (int i = 0; i < n_stops; ++i) loss_out[i] = std::sqrt(0.5 * sums[i] / static_cast<double>(n));   // loss.cpp:42-56, in float64
}

// Extension: the leaf every tree of [start_tree, stop_tree) routes a row to, or the rows per leaf (kern::predict_leaves / kern::leaf_counts).
// Leaf routing reads no value: there is no output width limit.  The dictionary is host state: a stale token is refused before a device is needed.
void Engine::predict_leaves(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const int32_t *cat_ids, bool ids_dev, const uint64_t *token,
                            int n, int n_num, int n_cat, int start_tree, int stop_tree, int32_t *out, bool out_dev) {
    const PredictBatch b{obs, obs_dev, cat, cat_dev, cat_ids, ids_dev, token, n, n_num, n_cat};
    check_batch(b, out != nullptr, /*width_limit=*/false);
    const int stop = check_leaves_range(start_tree, stop_tree);
    if (static_cast<int64_t>(n) * (stop - start_tree) >= (int64_t(1) << 31))
        throw Unsupported("predict_leaves: n_samples x trees >= 2^31 indices: slice the tree range");
    check_dict_token(b);
    const StagedBatch d = stage_batch(b);
    phase_end("inputs"); phase_begin(/*key=*/true);
    const size_t out_bytes = sizeof(int32_t) * static_cast<size_t>(n) * (stop - start_tree);
    int32_t *dl = out_dev ? out : static_cast<int32_t *>(d_leaves_out_.ensure(out_bytes));
    kern::predict_leaves(mirror_view(), d.obs, n_num, d.cat, n_cat, n, start_tree, stop, dl, hooks::on(hooks::LEAVES_GENERIC), stream_);
    finish("predict_leaves launch", "predict", {{out_dev ? nullptr : out, dl, out_bytes, "D2H leaves"}});
}

void Engine::leaf_counts(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const int32_t *cat_ids, bool ids_dev, const uint64_t *token, int n,
                         int n_num, int n_cat, int start_tree, int stop_tree, int64_t *counts_out) {
    const PredictBatch b{obs, obs_dev, cat, cat_dev, cat_ids, ids_dev, token, n, n_num, n_cat};
    check_batch(b, counts_out != nullptr, /*width_limit=*/false);
    const int stop = check_leaves_range(start_tree, stop_tree);
    check_dict_token(b);
    const StagedBatch d = stage_batch(b);
    phase_end("inputs"); phase_begin(/*key=*/true);
    const size_t L = static_cast<size_t>(model.meta.n_leaves);
    uint32_t *dcounts = static_cast<uint32_t *>(d_leaf_counts_.ensure(sizeof(uint32_t) * std::max<size_t>(L, 1)));
    hip_check(hipMemsetAsync(dcounts, 0, sizeof(uint32_t) * L, stream_), "zero leaf counters");
    kern::leaf_counts(mirror_view(), model.tree_indices.data(), d.obs, n_num, d.cat, n_cat, n, start_tree, stop, dcounts, hooks::on(hooks::LEAVES_GENERIC), stream_);
    std::vector<uint32_t> h(L);
    finish("leaf_counts launch", "predict", {{h.data(), dcounts, sizeof(uint32_t) * L, "D2H leaf counts"}});
    for (size_t l = 0; l < L; ++l) counts_out[l] = static_cast<int64_t>(h[l]);   // (n < 2^31 rows: a counter cannot wrap)
}

}  // namespace gbrl
