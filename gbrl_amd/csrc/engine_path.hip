// engine_path.hip -- path attribution (Saabas) on a prepared data set (path_core.h has the rule and the plans, path_rows.hip the kernels, explain.cpp
// the host evaluation on float observations):
//   Engine::path_contrib_prepared      the float32 matrix [m][F][D] of the trees [0, n_trees) for the rows of a row list; it stays on the device when
//                                      the caller binds it there
//   Engine::path_importance_prepared   its column sums and sums of absolute values in float64 by shap_core.h's rule (tiles of 64 positions, summed in
//                                      tile order by ONE finishing launch), and the expected value.  Streaming kernel: no float32 matrix at any point --
//                                      a tile's contributions are reduced in LDS to partials [tiles][2][n_used * D]; launches are cut by tiles so that the
//                                      partials a launch writes stay within 64 MiB, never by trees.  General kernel (D > 64, a model that is not
//                                      streamable, GBRL_HIP_PATH_GENERIC=1): chunks of rows into a float32 scratch within the same budget, each reduced
//                                      by shap_prepared's tile kernel.  The same bytes either way.
// The delta table is kept on the host under the mirror's marks (appended tree by tree; rewind_values / invalidate_mirror take it back) and uploaded
// when it has changed.  The checks are the ones the calls on a data set share: check_prepared_dataset, check_row_count / check_host_rows /
// subset_rows, check_code_range.  Everything that can be refused is refused before the device is touched; neither the model nor the data set is written.
#include "engine_codes_detail.h"
#include "hooks.h"
#include "path_core.h"
#include "shap_core.h"

namespace gbrl {

namespace {
struct ReleaseAtEnd { DevBuf &buf; ~ReleaseAtEnd() { buf.release(); } };
}  // namespace

// the host half of both calls: the refusals in order, the delta table brought up to the model, the slots of the range; returns the tree count
int Engine::check_path_prepared(const char *what, const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int n_trees) {
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    check_prepared_dataset(what, ds);
    if (md.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    const std::string bad_trees = kern::path_trees_error(n_trees, md.n_trees);
    if (!bad_trees.empty()) throw InvalidArgument(w + ": " + bad_trees);
    const int stop = n_trees == -1 ? md.n_trees : n_trees;
    check_row_count(what, "the call", rows, m, ds->n, "explain");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, what, 0, stop);
    if (path_version_ != model.version) {   // (rewind_values / invalidate_mirror have lowered the mark; an ensemble shrunk below it starts over)
        path_.extend(model, path_trees_);
        path_trees_ = static_cast<size_t>(md.n_trees);
        path_version_ = model.version;
    }
    const std::string bad_model = kern::path_model_error(model, path_, stop);
    if (!bad_model.empty()) throw Unsupported(w + ": " + bad_model);
    return stop;
}

// device, mirror, code tables, the row list, the delta table (when the model has changed) and the slot tables of the range: the `inputs` phase
Engine::PathRun Engine::stage_path_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int stop) {
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    PathRun r;
    r.pm = mirror_view();
    r.ct = sync_code_tables(*ds);
    r.rows = subset_rows(ds, rows, rows_dev, m);
    const size_t rec = static_cast<size_t>(model.meta.max_depth) * model.meta.output_dim, L = static_cast<size_t>(model.meta.n_leaves);
    if (path_dev_version_ != model.version) {   // (one copy of the whole table: the buffer may have moved)
        path_.delta.resize(std::max<size_t>(L * rec, 1));
        upload(m_path_delta_, path_.delta.data(), path_.delta.size(), "H2D path deltas");
        path_dev_version_ = model.version;
    }
    const std::vector<int32_t> used = kern::path_used(model, stop, ds->F);
    std::vector<int32_t> slot_of(static_cast<size_t>(ds->F), -1);
    for (size_t s = 0; s < used.size(); ++s) slot_of[used[s]] = static_cast<int32_t>(s);
    r.used = used;
    r.pt.delta = m_path_delta_.as<float>();
    r.pt.used = upload(d_path_used_, used.data(), std::max<size_t>(used.size(), 1), "H2D path slots");
    r.pt.slot_of = upload(d_path_slot_of_, slot_of.data(), slot_of.size(), "H2D path slots");
    r.pt.n_used = static_cast<int>(used.size());
    hip_check(hipStreamSynchronize(stream_), "sync");   // (the host vectors go out of scope)
    phase_end("inputs");
    return r;
}

// positions [p0, p0 + count) of the row list into out [count][F][D], zeroed here; the kernel alone is the phase `path_rows`
void Engine::launch_path_matrix(const PreparedDataset *ds, const PathRun &r, int p0, int count, int stop, bool generic, float *out) {
    phase_begin();
    hip_check(hipMemsetAsync(out, 0, sizeof(float) * static_cast<size_t>(count) * ds->F * model.meta.output_dim, stream_), "memset path");
    phase_end("zero"); phase_begin(/*key=*/true);
    const kern::CodeRows cr{ds->prep.d_codes, ds->n, ds->code_groups(), r.rows, p0};
    if (generic || !kern::path_rows_stream(r.pm, r.ct, r.pt, cr, ds->F, count, stop, out, nullptr, 0, stream_))
        kern::path_rows_general(r.pm, r.ct, r.pt.delta, cr, ds->F, count, stop, out, stream_);
    phase_end("path_rows", /*key=*/true);
}

void Engine::path_contrib_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int n_trees, float *out, bool out_dev) {
    const char *what = "path_contrib_prepared";
    const int stop = check_path_prepared(what, ds, rows, rows_dev, m, n_trees);
    if (out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const std::string too_large = kern::path_matrix_error(m, ds->F, model.meta.output_dim);
    if (!too_large.empty()) throw Unsupported(std::string(what) + ": " + too_large);
    const bool generic = hooks::on(hooks::PATH_GENERIC);
    const PathRun r = stage_path_prepared(ds, rows, rows_dev, m, stop);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(m) * ds->F * model.meta.output_dim;
    const ReleaseAtEnd release_out{d_path_out_};   // a host-bound matrix (up to 8 GiB) does not outlive the call
    float *dout = out_dev ? out : static_cast<float *>(d_path_out_.ensure(out_bytes));
    launch_path_matrix(ds, r, 0, m, stop, generic, dout);
    hip_check(hipGetLastError(), "path_contrib_prepared launch");
    if (!out_dev) hip_check(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, stream_), "D2H path");
    hip_check(hipStreamSynchronize(stream_), "sync");
    phases_resolve();
}

void Engine::path_importance_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int n_trees, double *sum_out, double *abs_out,
                                      double *expected_out, int *passes_out) {
    const char *what = "path_importance_prepared";
    const int stop = check_path_prepared(what, ds, rows, rows_dev, m, n_trees);
    if (sum_out == nullptr || abs_out == nullptr) throw InvalidArgument(std::string(what) + ": no place for the result");
    const int F = ds->F, D = model.meta.output_dim, C = F * D, tiles = kern::path_tiles(m);
    if (expected_out != nullptr) path_.expected(model, stop, expected_out);
    const bool generic = hooks::on(hooks::PATH_GENERIC);
    const PathRun r = stage_path_prepared(ds, rows, rows_dev, m, stop);
    const int U = r.pt.n_used, CU = U * D;
    const ReleaseAtEnd release_part{d_path_part_};   // the partials of every tile live until the finishing launch, then go
    std::fill(sum_out, sum_out + C, 0.0);
    std::fill(abs_out, abs_out + C, 0.0);
    const kern::PathSlotPlan plan = kern::path_slot_plan(U, ds->code_groups(), D);
    if (passes_out) *passes_out = 0;
    std::vector<double> sums;
    bool streamed = false;
    if (!generic && U > 0) {   // ---- streaming: partials [tiles][2][U * D], launches of at most the budget's tiles
        double *d_part = static_cast<double *>(d_path_part_.ensure(sizeof(double) * static_cast<size_t>(tiles) * 2 * CU));
        const int per_launch = kern::path_launch_tiles(sizeof(double) * 2 * static_cast<size_t>(CU));
        streamed = true;
        phase_begin(/*key=*/true);
        for (int t0 = 0; t0 < tiles && streamed; t0 += per_launch) {
            const int p0 = t0 * kern::kPathRows, count = static_cast<int>(std::min<long long>(static_cast<long long>(per_launch) * kern::kPathRows, static_cast<long long>(m) - p0));
            streamed = kern::path_rows_stream(r.pm, r.ct, r.pt, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), r.rows, p0}, F, count, stop, nullptr, d_part,
                                              t0, stream_);   // (refused at the first launch or never: nothing was launched then)
        }
        phase_end("path_rows", /*key=*/true);
        if (streamed) {
            phase_begin();
            double *d_sums = static_cast<double *>(d_path_sums_.ensure(sizeof(double) * 2 * CU));
            kern::shap_reduce_finish(d_part, tiles, CU, d_sums, stream_);
            phase_end("reduce");
            sums.assign(static_cast<size_t>(2) * CU, 0.0);
            hip_check(hipGetLastError(), "path_importance_prepared launch");
            hip_check(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, stream_), "D2H sums");
            hip_check(hipStreamSynchronize(stream_), "sync");
            for (int s = 0; s < U; ++s) {   // slot s is column used[s]; a column no tree tests keeps its zeros
                std::copy_n(sums.data() + static_cast<size_t>(s) * D, D, sum_out + static_cast<size_t>(r.used[s]) * D);
                std::copy_n(sums.data() + CU + static_cast<size_t>(s) * D, D, abs_out + static_cast<size_t>(r.used[s]) * D);
            }
            if (passes_out) *passes_out = plan.passes;
        }
    }
    if (!streamed && U > 0) {   // ---- general: chunks of the matrix into the scratch, shap_prepared's tile reduction, partials [tiles][2][F * D]
        const int chunk_rows = kern::path_launch_tiles(sizeof(float) * kern::kPathRows * static_cast<size_t>(C)) * kern::kPathRows;
        const size_t alloc_rows = static_cast<size_t>(std::min<long long>(chunk_rows, static_cast<long long>(tiles) * kern::kPathRows));
        float *d_scratch = static_cast<float *>(d_path_scratch_.ensure(sizeof(float) * alloc_rows * C));
        double *d_part = static_cast<double *>(d_path_part_.ensure(sizeof(double) * static_cast<size_t>(tiles) * 2 * C));
        double *d_sums = static_cast<double *>(d_path_sums_.ensure(sizeof(double) * 2 * C));
        for (long long p0 = 0; p0 < m; p0 += chunk_rows) {
            const int count = static_cast<int>(std::min<long long>(chunk_rows, m - p0));
            launch_path_matrix(ds, r, static_cast<int>(p0), count, stop, /*generic=*/true, d_scratch);
            phase_begin();
            kern::shap_reduce_tiles(d_scratch, count, C, d_part, static_cast<int>(p0 / kern::kPathRows), stream_);
            phase_end("reduce");
        }
        phase_begin();
        kern::shap_reduce_finish(d_part, tiles, C, d_sums, stream_);
        phase_end("reduce");
        sums.assign(static_cast<size_t>(2) * C, 0.0);
        hip_check(hipGetLastError(), "path_importance_prepared launch");
        hip_check(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, stream_), "D2H sums");
        hip_check(hipStreamSynchronize(stream_), "sync");
        std::copy_n(sums.data(), C, sum_out);
        std::copy_n(sums.data() + C, C, abs_out);
    }
    phases_resolve();
}

}  // namespace gbrl
