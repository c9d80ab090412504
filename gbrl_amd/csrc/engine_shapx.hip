// engine_shapx.hip -- SHAP interaction values on a prepared data set (shapx_core.h has the rule, the records and the plans, shap_interactions.hip the
// kernels, explain.cpp the host evaluation on float observations):
//   Engine::shap_interactions_prepared             the float32 matrix [m][K][K][D] of the trees [0, n_trees) for the rows of a row list, K the features
//                                                  those trees test; it stays on the device when the caller binds it there
//   Engine::shap_interaction_importance_prepared   its sums and sums of absolute values over the rows in float64 by shap_core.h's rule: chunk_rows rows
//                                                  at a time into a float32 scratch within 64 MiB, each chunk reduced to tile partials, ONE finishing
//                                                  launch; the matrix is never held whole
// The records depend on the tree range: they are kept on the host per (model version, range) and uploaded per call (the `inputs` phase; leaves x depth
// words); the streaming kernel's
// weight table is computed on the device by one launch (phase `shapx_table`).  A shape the streaming plan declines, a refused LDS opt-in and
// GBRL_HIP_SHAPX_GENERIC=1 take the one-thread-per-row kernel, cut into launches whose float64 scratch stays within 64 MiB.  The checks are the ones the
// calls on a data set share.  Everything that can be refused is refused before the device is touched; neither the model nor the data set is written.
#include "engine_codes_detail.h"
#include "hooks.h"
#include "shap_core.h"
#include "shapx_core.h"

namespace gbrl {

namespace {
struct ReleaseAtEnd { DevBuf &buf; ~ReleaseAtEnd() { buf.release(); } };
}  // namespace

const kern::ShapxRecords &Engine::shapx_records(int n_trees) {
    const std::string bad = kern::shapx_model_error(model, n_trees);
    if (!bad.empty()) throw InvalidArgument("shap_interactions: " + bad);
    const int stop = n_trees == -1 ? model.meta.n_trees : n_trees;
    if (shapx_rec_version_ != model.version || shapx_rec_stop_ != stop) {
        shapx_rec_ = kern::ShapxRecords();
        shapx_rec_.build(model, stop);
        shapx_rec_version_ = model.version;
        shapx_rec_stop_ = stop;
    }
    const std::string wide = kern::shapx_width_error(static_cast<int>(shapx_rec_.features.size()), model.meta.output_dim);
    if (!wide.empty()) throw Unsupported("shap_interactions: " + wide);
    return shapx_rec_;
}

int Engine::check_shapx_prepared(const char *what, const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int n_trees) {
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    check_prepared_dataset(what, ds);
    const std::string bad = kern::shapx_model_error(model, n_trees);
    if (!bad.empty()) throw InvalidArgument(w + ": " + bad);
    const int stop = n_trees == -1 ? md.n_trees : n_trees;
    check_row_count(what, "the call", rows, m, ds->n, "explain");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, what, 0, stop);
    return stop;
}

// device, mirror, code tables, the row list, the records and -- when the plan takes the shape -- the weight table
Engine::ShapxRun Engine::stage_shapx_prepared(const PreparedDataset *ds, const kern::ShapxRecords &rec, const int32_t *rows, bool rows_dev, int m) {
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    ShapxRun r;
    r.pm = mirror_view();
    r.ct = sync_code_tables(*ds);
    r.rows = subset_rows(ds, rows, rows_dev, m);
    const std::vector<double> wtab = kern::shapx_w_table();
    kern::ShapxTables &st = r.st;
    st.leaf = upload(d_shapx_leaf_, rec.leaf.data(), rec.leaf.size(), "H2D shapx records");
    st.mslot = upload(d_shapx_mslot_, rec.mslot.data(), rec.mslot.size(), "H2D shapx records");
    st.mz = upload(d_shapx_mz_, rec.mz.data(), rec.mz.size(), "H2D shapx records");
    st.cond_e = upload(d_shapx_cond_e_, rec.cond_e.data(), rec.cond_e.size(), "H2D shapx records");
    st.ent = upload(d_shapx_ent_, rec.ent.data(), rec.ent.size(), "H2D shapx records");
    st.ent_first = upload(d_shapx_ent_first_, rec.ent_first.data(), rec.ent_first.size(), "H2D shapx records");
    st.tree = upload(d_shapx_tree_, rec.tree.data(), rec.tree.size(), "H2D shapx records");
    st.tmap = upload(d_shapx_tmap_, rec.tmap.data(), rec.tmap.size(), "H2D shapx records");
    st.wtab = upload(d_shapx_wtab_, wtab.data(), wtab.size(), "H2D shapx records");
    st.K = static_cast<int>(rec.features.size());
    st.nt_max = rec.nt_max; st.n_max = rec.n_max; st.n_leaves = static_cast<int>(rec.leaf.size());
    const kern::ShapxPlan plan = kern::shapx_plan(st.K, st.nt_max, st.n_max, ds->code_groups(), model.meta.output_dim, rec.table_doubles);
    r.stream = !hooks::on(hooks::SHAPX_GENERIC) && plan.fits;
    r.block_rows = r.stream ? plan.rows : 0;
    st.table_doubles = r.stream ? rec.table_doubles : 0;
    st.table = r.stream ? static_cast<double *>(d_shapx_table_.ensure(sizeof(double) * rec.table_doubles)) : nullptr;
    hip_check(hipStreamSynchronize(stream_), "sync");   // (the host vectors go out of scope)
    phase_end("inputs");
    if (r.stream) {
        phase_begin();
        kern::shapx_build_table(st, stream_);
        phase_end("shapx_table");
    }
    return r;
}

// positions [p0, p0 + count) of the row list into out [count][K][K][D]; the kernels alone are the phase `shapx_rows`
bool Engine::launch_shapx_matrix(const PreparedDataset *ds, const ShapxRun &r, int p0, int count, int stop, float *out) {
    if (count <= 0 || r.st.K == 0) return r.stream;
    const int D = model.meta.output_dim;
    const size_t KKD = static_cast<size_t>(r.st.K) * r.st.K * D;
    phase_begin(/*key=*/true);
    const bool streamed = r.stream && kern::shapx_rows_stream(r.pm, r.ct, r.st, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), r.rows, p0}, count, stop, out, stream_);
    if (!streamed) {
        const size_t row_doubles = kern::shapx_general_row_doubles(r.st.K, r.st.nt_max, r.st.n_max, D);
        const int per_launch = kern::shapx_general_rows(row_doubles);
        double *scratch = static_cast<double *>(d_shapx_scratch_.ensure(sizeof(double) * row_doubles * static_cast<size_t>(std::min(per_launch, count))));
        for (int q0 = 0; q0 < count; q0 += per_launch)
            kern::shapx_rows_general(r.pm, r.ct, r.st, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), r.rows, p0 + q0}, std::min(per_launch, count - q0), stop,
                                     scratch, out + static_cast<size_t>(q0) * KKD, stream_);
    }
    phase_end("shapx_rows", /*key=*/true);
    return streamed;
}

void Engine::shap_interactions_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int n_trees, float *out, bool out_dev,
                                        int *block_rows_out) {
    const char *what = "shap_interactions_prepared";
    const int stop = check_shapx_prepared(what, ds, rows, rows_dev, m, n_trees);
    if (out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const kern::ShapxRecords &rec = shapx_records(stop);
    const int K = static_cast<int>(rec.features.size());
    const std::string too_large = kern::shapx_matrix_error(m, K, model.meta.output_dim);
    if (!too_large.empty()) throw Unsupported(std::string(what) + ": " + too_large);
    const ShapxRun r = stage_shapx_prepared(ds, rec, rows, rows_dev, m);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(m) * K * K * model.meta.output_dim;
    // a host-bound matrix (up to 8 GiB), the weight table (up to 256 MiB) and the general kernel's scratch (64 MiB) do not outlive the call
    const ReleaseAtEnd release_out{d_shapx_out_}, release_table{d_shapx_table_}, release_scratch{d_shapx_scratch_};
    float *dout = out_dev ? out : static_cast<float *>(d_shapx_out_.ensure(std::max<size_t>(out_bytes, 4)));
    const bool streamed = launch_shapx_matrix(ds, r, 0, m, stop, dout);
    if (block_rows_out) *block_rows_out = streamed ? r.block_rows : 0;
    hip_check(hipGetLastError(), "shap_interactions_prepared launch");
    if (!out_dev && out_bytes > 0) hip_check(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, stream_), "D2H shap interactions");
    hip_check(hipStreamSynchronize(stream_), "sync");
    phases_resolve();
}

void Engine::shap_interaction_importance_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int n_trees, int chunk_rows, double *sum_out,
                                                  double *abs_out, int *chunk_rows_used, int *block_rows_out) {
    const char *what = "shap_interaction_importance_prepared";
    const int stop = check_shapx_prepared(what, ds, rows, rows_dev, m, n_trees);
    if (sum_out == nullptr || abs_out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const std::string bad_chunk = kern::shap_chunk_rows_error(chunk_rows);
    if (!bad_chunk.empty()) throw InvalidArgument(std::string(what) + ": " + bad_chunk);
    const kern::ShapxRecords &rec = shapx_records(stop);   // (K * K * D < 2^31: shapx_width_error)
    const int K = static_cast<int>(rec.features.size()), D = model.meta.output_dim, C = K * K * D;
    const kern::ShapChunkPlan plan = kern::shap_chunk_plan(m, K * K, D, chunk_rows);
    if (chunk_rows_used) *chunk_rows_used = plan.chunk_rows;
    if (block_rows_out) *block_rows_out = 0;
    if (C == 0) return;
    const ShapxRun r = stage_shapx_prepared(ds, rec, rows, rows_dev, m);
    const ReleaseAtEnd release_out{d_shapx_out_}, release_part{d_shapx_part_}, release_table{d_shapx_table_}, release_scratch{d_shapx_scratch_};
    float *d_chunk = static_cast<float *>(d_shapx_out_.ensure(plan.scratch_bytes));
    double *d_part = static_cast<double *>(d_shapx_part_.ensure(plan.partial_bytes));
    double *d_sums = static_cast<double *>(d_shapx_sums_.ensure(sizeof(double) * 2 * C));
    for (long long p0 = 0; p0 < m; p0 += plan.chunk_rows) {
        const int count = static_cast<int>(std::min<long long>(plan.chunk_rows, m - p0));
        const bool streamed = launch_shapx_matrix(ds, r, static_cast<int>(p0), count, stop, d_chunk);
        if (block_rows_out) *block_rows_out = streamed ? r.block_rows : 0;
        phase_begin();
        kern::shap_reduce_tiles(d_chunk, count, C, d_part, static_cast<int>(p0 / kern::kShapTileRows), stream_);
        phase_end("reduce");
    }
    phase_begin();
    kern::shap_reduce_finish(d_part, plan.tiles, C, d_sums, stream_);
    phase_end("reduce");
    std::vector<double> sums(static_cast<size_t>(2) * C, 0.0);
    hip_check(hipGetLastError(), "shap_interaction_importance_prepared launch");
    hip_check(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, stream_), "D2H sums");
    hip_check(hipStreamSynchronize(stream_), "sync");
    std::copy_n(sums.data(), C, sum_out);
    std::copy_n(sums.data() + C, C, abs_out);
    phases_resolve();
}

}  // namespace gbrl
