// engine_explain.hip -- Linear TreeSHAP of the ensemble on the device (see shap.hip; host evaluation: explain.cpp).
//   Engine::shap_on_device             tree_shap / ensemble_shap: host observations in, the [n][F][D] matrix back to the host
//   Engine::shap_prepared              the same matrix from a prepared data set's bin codes, for the rows of a row list; it stays on the device when
//                                      the caller binds it there
//   Engine::shap_importance_prepared   its column sums and sums of absolute values in float64 (shap_core.h's rule), the matrix never held whole:
//                                      chunks of rows into a float32 scratch, every chunk reduced to its tile partials, ONE finishing launch and ONE
//                                      read-back of 2 F D doubles
// Both forms build their program -- ops, node records, leaf values -- through build_shap_program; the codes form hands it the data set's bins
// (engine_codes.hip: x > v <=> code > bin) and keeps its program in buffers of its own, keyed on (model.version, thresholds id): neither form ever
// evicts or overwrites the other's cache.  The checks of the data-set calls are the ones that family shares: check_prepared_dataset,
// check_row_count / check_host_rows / subset_rows, check_code_range.  Neither the model nor the data set is written.
#include "engine_codes_detail.h"
#include "hooks.h"
#include "explain.h"
#include "shap_core.h"

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace gbrl {

namespace {

// depth-first emission of the uniform program: ENTER n; [left subtree; AFTER_LEFT n; right subtree; AFTER_RIGHT n;] EXIT n
void emit(const ShapTree &t, int n, int level, int via, int base, std::vector<kern::ShapOp> &ops) {
    const ShapNode &nd = t.nodes[n];
    ops.push_back({kern::SHAP_ENTER, base + n, level, via});
    if (nd.left >= 0) {
        emit(t, nd.left, level + 1, nd.feature, base, ops);
        ops.push_back({kern::SHAP_AFTER_LEFT, base + n, level, via});
        emit(t, nd.right, level + 1, nd.feature, base, ops);
        ops.push_back({kern::SHAP_AFTER_RIGHT, base + n, level, via});
    }
    if (via >= 0) ops.push_back({kern::SHAP_EXIT, base + n, level, via});
}

// What k_shap executes for the trees [t0, t1): the ops, the node records (indices global over the program) and the cover-weighted leaf values.
// cat_ids: the dictionary ids of the categorical conditions, by condition slot (null: a model without them).  bins: null for the float form -- a
// numeric record then holds its threshold; else a table shaped like feature_values (every walked numeric slot expressible: the caller has checked)
// and the record holds the slot's bin, bit cast into the same four bytes.
struct ShapProgram {
    std::vector<kern::ShapOp> ops;
    std::vector<kern::ShapNodeRec> recs;
    std::vector<float> leaf_value;
};

ShapProgram build_shap_program(const Model &model, int t0, int t1, const int32_t *cat_ids, const int32_t *bins) {
    ShapProgram p;
    for (int t = t0; t < t1; ++t) {
        const ShapTree st = build_shap_tree(model, t);
        const int node_base = static_cast<int>(p.recs.size()), value_base = static_cast<int>(p.leaf_value.size());
        for (size_t i = 0; i < st.nodes.size(); ++i) {
            const ShapNode &nd = st.nodes[i];
            kern::ShapNodeRec r{};
            const bool leaf = nd.left < 0 && nd.right < 0, tied = nd.tied_to >= 0;
            const bool right_child = nd.parent >= 0 && st.nodes[nd.parent].right == static_cast<int>(i);
            r.feature = nd.feature;
            r.flags = (nd.numeric ? 1 : 0) | (tied ? 2 : 0) | (leaf ? 4 : 0) | (right_child ? 8 : 0);
            r.cat_id = (!leaf && !nd.numeric) ? cat_ids[nd.cond] : 0;
            r.pred = leaf ? value_base + nd.pred : 0;
            r.n_unique = nd.n_unique;
            r.n_unique_parent = tied ? st.nodes[nd.tied_to].n_unique : 0;
            r.deg_left = leaf ? 0 : nd.n_unique - st.nodes[nd.left].n_unique;
            r.deg_right = leaf ? 0 : nd.n_unique - st.nodes[nd.right].n_unique;
            r.threshold = nd.threshold;
            if (bins != nullptr && !leaf && nd.numeric) std::memcpy(&r.threshold, &bins[nd.cond], sizeof(float));
            r.weight = nd.weight;
            r.weight_parent = tied ? st.nodes[nd.tied_to].weight : 0.0f;
            p.recs.push_back(r);
        }
        p.leaf_value.insert(p.leaf_value.end(), st.leaf_value.begin(), st.leaf_value.end());
        emit(st, 0, 0, -1, node_base, p.ops);
    }
    p.leaf_value.push_back(0.0f);
    return p;
}

struct ReleaseAtEnd { DevBuf &buf; ~ReleaseAtEnd() { buf.release(); } };

}  // namespace

// the program on the device, in the buffers of one form; waits for the copies (the host vectors go out of scope)
int Engine::upload_shap_program(int t0, int t1, const int32_t *bins, DevBuf &ops, DevBuf &nodes, DevBuf &values) {
    const ShapProgram p = build_shap_program(model, t0, t1, cat_ids_host_.data(), bins);
    upload(ops, p.ops.data(), p.ops.size(), "H2D shap program");
    upload(nodes, p.recs.data(), p.recs.size(), "H2D shap nodes");
    upload(values, p.leaf_value.data(), p.leaf_value.size(), "H2D shap leaf values");
    hip_check(hipStreamSynchronize(stream_), "sync");
    return static_cast<int>(p.ops.size());
}

// norm [(depth+1)][depth], base [depth], offset [depth][depth] behind one another in one buffer
Engine::ShapPoly Engine::upload_shap_poly(DevBuf &buf, const float *norm, const float *base_poly, const float *offset) {
    const size_t depth = static_cast<size_t>(model.meta.max_depth);
    float *dpoly = static_cast<float *>(buf.ensure(((depth + 1) * depth + depth + depth * depth) * 4));
    ShapPoly p{dpoly, dpoly + (depth + 1) * depth, dpoly + (depth + 1) * depth + depth};
    hip_check(hipMemcpyAsync(dpoly, norm, sizeof(float) * (depth + 1) * depth, hipMemcpyHostToDevice, stream_), "H2D norm");
    hip_check(hipMemcpyAsync(const_cast<float *>(p.base), base_poly, sizeof(float) * depth, hipMemcpyHostToDevice, stream_), "H2D base");
    hip_check(hipMemcpyAsync(const_cast<float *>(p.offset), offset, sizeof(float) * depth * depth, hipMemcpyHostToDevice, stream_), "H2D offset");
    return p;
}

bool Engine::shap_on_device(int tree_idx, const float *obs, const char *cat, int n, const float *norm, const float *base_poly,
                            const float *offset, float *out) {
    const gbrl_hip_metadata &md = model.meta;
    const int D = md.output_dim, depth = md.max_depth, n_num = md.n_num_features, n_cat = md.n_cat_features;
    if (const char *e = hooks::raw(hooks::SHAP_HOST)) { if (e[0] == '1') return false; }   // test hook: host evaluation
    const bool only = hooks::on(hooks::SHAP_DEVICE_ONLY);   // test hook: raise where the host would silently take over
    if (kern::shap_block_threads(depth, D) == 0) {
        if (only) throw std::runtime_error("GBRL_HIP_SHAP_DEVICE_ONLY=1: k_shap has no launch plan for max_depth " + std::to_string(depth) +
                                           ", output_dim " + std::to_string(D) + " (the host evaluation would take this shape)");
        return false;
    }
    try { ensure_device(); } catch (const NoDeviceError &e) {   // inspection also works on a machine without a GPU
        if (only) throw std::runtime_error(std::string("GBRL_HIP_SHAP_DEVICE_ONLY=1: no device for k_shap (the host evaluation would run): ") + e.what());
        return false;
    }
    if (md.n_trees == 0 || n <= 0) return true;
    hipStream_t s = stream_;
    reset_events();
    sync_model_to_device();   // categorical conditions -> dictionary ids
    // ---- the program: one tree, or the whole ensemble (cached until the model changes) ----
    const bool whole = tree_idx < 0;
    if (!whole || shap_prog_version_ != model.version) {
        shap_n_ops_ = upload_shap_program(whole ? 0 : tree_idx, whole ? md.n_trees : tree_idx + 1, nullptr, d_shap_ops_, d_shap_nodes_, d_shap_values_);
        shap_prog_version_ = whole ? model.version : ~0ull;
    }
    // ---- inputs ----
    const float *dobs = nullptr;
    if (n_num > 0) {
        float *p = static_cast<float *>(d_pobs_.ensure(sizeof(float) * static_cast<size_t>(n) * n_num));
        hip_check(hipMemcpyAsync(p, obs, sizeof(float) * static_cast<size_t>(n) * n_num, hipMemcpyHostToDevice, s), "H2D obs");
        dobs = p;
    }
    const int32_t *dcat = n_cat > 0 ? encode_categorical_batch(cat, false, n, n_cat) : nullptr;
    const ShapPoly poly = upload_shap_poly(d_shap_poly_, norm, base_poly, offset);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(n) * (n_num + n_cat) * D;
    float *dout = static_cast<float *>(d_shap_out_.ensure(out_bytes));
    hip_check(hipMemsetAsync(dout, 0, out_bytes, s), "memset shap");
    phase_begin(/*key=*/true);   // the kernel alone (set_profiling: the phase `shap` of last_phase_times, as the codes form names it)
    kern::shap_values(d_shap_ops_.as<kern::ShapOp>(), shap_n_ops_, d_shap_nodes_.as<kern::ShapNodeRec>(), d_shap_values_.as<float>(), dobs, n_num,
                      dcat, n_cat, n, D, depth, poly.norm, poly.base, poly.offset, dout, s);
    hip_check(hipGetLastError(), "shap launch");
    phase_end("shap", /*key=*/true);
    hip_check(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, s), "D2H shap");
    hip_check(hipStreamSynchronize(s), "sync");
    phases_resolve();
    return true;
}

// ---- the calls on a data set.  Everything that can be refused is refused here, before the device is touched.
void Engine::check_shap_prepared(const char *what, const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int tree_idx, const float *norm,
                                 const float *base_poly, const float *offset) {
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    check_prepared_dataset(what, ds);
    if (md.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    if (norm == nullptr || base_poly == nullptr || offset == nullptr)
        throw InvalidArgument(w + ": " + (norm == nullptr ? "norm_values" : base_poly == nullptr ? "base_poly" : "offset") +
                              " is missing (the three polynomial arrays ensemble_shap takes, built for the model's max_depth)");
    const std::string tree_error = kern::shap_tree_error(tree_idx, md.n_trees);
    if (!tree_error.empty()) throw InvalidArgument(w + ": " + tree_error);
    check_row_count(what, "the call", rows, m, ds->n, "explain");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    if (kern::shap_block_threads(md.max_depth, md.output_dim) == 0)   // the codes live on the device: there is no host evaluation to hand over to
        throw Unsupported(w + ": k_shap has no launch plan for max_depth " + std::to_string(md.max_depth) + ", output_dim " + std::to_string(md.output_dim));
    check_code_range(*ds, what, tree_idx < 0 ? 0 : tree_idx, tree_idx < 0 ? md.n_trees : tree_idx + 1);
}

// device, mirror, the row list, the program of the codes form (cached for the whole ensemble) and the polynomial arrays: the `inputs` phase
Engine::ShapPreparedRun Engine::stage_shap_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int tree_idx, const float *norm,
                                                    const float *base_poly, const float *offset) {
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const bool whole = tree_idx < 0;
    if (!whole || shapc_prog_version_ != model.version || shapc_ds_id_ != ds->thresholds_id) {
        shapc_n_ops_ = upload_shap_program(whole ? 0 : tree_idx, whole ? model.meta.n_trees : tree_idx + 1, code_bins_host_.data(), d_shapc_ops_, d_shapc_nodes_,
                                           d_shapc_values_);
        shapc_prog_version_ = whole ? model.version : ~0ull;
        shapc_ds_id_ = ds->thresholds_id;
    }
    ShapPreparedRun r;
    r.rows = subset_rows(ds, rows, rows_dev, m);
    r.poly = upload_shap_poly(d_shapc_poly_, norm, base_poly, offset);
    phase_end("inputs");
    return r;
}

// positions [p0, p0 + count) of the row list into out [count][F][D] (zeroed here: the kernel accumulates over the trees); phases `zero` and,
// the kernel alone, `shap`
void Engine::launch_shap_codes(const PreparedDataset *ds, const ShapPreparedRun &r, int p0, int count, float *out) {
    const gbrl_hip_metadata &md = model.meta;
    phase_begin();
    hip_check(hipMemsetAsync(out, 0, sizeof(float) * static_cast<size_t>(count) * ds->F * md.output_dim, stream_), "memset shap");
    phase_end("zero"); phase_begin(/*key=*/true);
    kern::shap_values_codes(d_shapc_ops_.as<kern::ShapOp>(), shapc_n_ops_, d_shapc_nodes_.as<kern::ShapNodeRec>(), d_shapc_values_.as<float>(),
                            kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), r.rows, p0}, ds->F, count, md.output_dim, md.max_depth, r.poly.norm,
                            r.poly.base, r.poly.offset, out, stream_);
    phase_end("shap", /*key=*/true);
}

// the end of both data-set calls: the launch error, the result on its way to the host (host == nullptr: it stays on the device), ONE wait, phase times
void Engine::finish_shap_prepared(const char *launch, void *host, const void *dev, size_t bytes, const char *what) {
    hip_check(hipGetLastError(), launch);
    if (host != nullptr) hip_check(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream_), what);
    hip_check(hipStreamSynchronize(stream_), "sync");
    phases_resolve();
}

void Engine::shap_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int tree_idx, const float *norm, const float *base_poly,
                           const float *offset, float *out, bool out_dev) {
    const char *what = "shap_prepared";
    check_shap_prepared(what, ds, rows, rows_dev, m, tree_idx, norm, base_poly, offset);
    if (out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const std::string too_large = kern::shap_matrix_error(m, ds->F, model.meta.output_dim);
    if (!too_large.empty()) throw Unsupported(std::string(what) + ": " + too_large);
    const ShapPreparedRun r = stage_shap_prepared(ds, rows, rows_dev, m, tree_idx, norm, base_poly, offset);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(m) * ds->F * model.meta.output_dim;
    if (out_dev) {
        launch_shap_codes(ds, r, 0, m, out);
        finish_shap_prepared("shap_prepared launch", nullptr, out, out_bytes, "D2H shap");
        return;
    }
    const ReleaseAtEnd release_out{d_shapc_out_};   // a host-bound matrix (up to 8 GiB) does not outlive the call; the importance call's scratch is another buffer
    float *dout = static_cast<float *>(d_shapc_out_.ensure(out_bytes));
    launch_shap_codes(ds, r, 0, m, dout);
    finish_shap_prepared("shap_prepared launch", out, dout, out_bytes, "D2H shap");
}

void Engine::shap_importance_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *norm, const float *base_poly,
                                      const float *offset, int chunk_rows, double *sum_out, double *abs_out, int *chunk_rows_used) {
    const char *what = "shap_importance_prepared";
    check_shap_prepared(what, ds, rows, rows_dev, m, -1, norm, base_poly, offset);
    if (sum_out == nullptr || abs_out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const std::string bad_chunk = kern::shap_chunk_rows_error(chunk_rows);
    if (!bad_chunk.empty()) throw InvalidArgument(std::string(what) + ": " + bad_chunk);
    const int F = ds->F, D = model.meta.output_dim, C = F * D;   // (F <= 2^20 groups of 16, D <= 128: 2 C fits an int)
    const kern::ShapChunkPlan plan = kern::shap_chunk_plan(m, F, D, chunk_rows);
    if (chunk_rows_used) *chunk_rows_used = plan.chunk_rows;
    const ShapPreparedRun r = stage_shap_prepared(ds, rows, rows_dev, m, -1, norm, base_poly, offset);
    float *d_scratch = static_cast<float *>(d_shapc_scratch_.ensure(plan.scratch_bytes));   // at most 64 MiB (or one tile): kept for the next call
    const ReleaseAtEnd release_part{d_shapc_part_};   // 16 F D bytes per tile: 256 MiB at 2^20 rows x 128 features x 8 outputs
    double *d_part = static_cast<double *>(d_shapc_part_.ensure(plan.partial_bytes));
    double *d_sums = static_cast<double *>(d_shapc_sums_.ensure(sizeof(double) * 2 * C));
    for (long long p0 = 0; p0 < m; p0 += plan.chunk_rows) {
        const int count = static_cast<int>(std::min<long long>(plan.chunk_rows, m - p0));
        launch_shap_codes(ds, r, static_cast<int>(p0), count, d_scratch);
        phase_begin();
        kern::shap_reduce_tiles(d_scratch, count, C, d_part, static_cast<int>(p0 / kern::kShapTileRows), stream_);
        phase_end("reduce");
    }
    phase_begin();
    kern::shap_reduce_finish(d_part, plan.tiles, C, d_sums, stream_);
    phase_end("reduce");
    std::vector<double> sums(static_cast<size_t>(2) * C, 0.0);
    finish_shap_prepared("shap_importance_prepared launch", sums.data(), d_sums, sizeof(double) * sums.size(), "D2H sums");
    std::copy_n(sums.data(), C, sum_out);
    std::copy_n(sums.data() + C, C, abs_out);
}

}  // namespace gbrl
