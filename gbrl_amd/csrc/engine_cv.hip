// engine_cv.hip -- control variates as a call of its own (cv_core.h has the rule, control_variates.hip the kernels, cv_host.cpp the host evaluation):
//   Engine::control_variates            float rows of a numeric-only model, on the stages of engine_predict.hip
//   Engine::control_variates_prepared   the rows of a prepared data set, on the stages of engine_codes.hip (check_code_range, sync_code_tables, subset_rows)
// Both refuse everything they can before the device is touched (check_cv), stage their inputs in the `inputs` phase, enqueue at most four launches
// (run_cv) and wait once (finish).  The scratch -- the scaled averages [n][D], the slot arrays and the statistics -- is the engine's workspace.
#include "cv_core.h"
#include "engine_codes_detail.h"
#include "hooks.h"

#include <cmath>

namespace gbrl {

float Engine::check_cv(const char *what, int n, const CvArgs &a) const {
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    if (has_coll_ || rccl_comm_ != nullptr)
        throw Unsupported(w + ": not available on a model with a communicator or collective hooks (the column statistics would need an exchange)");
    if (md.iteration > 0 && md.n_cat_features > 0) throw Unsupported(w + ": not available on a model with categorical columns");
    if (md.output_dim > kern::kCvMaxD) throw Unsupported(w + ": output_dim > 128");
    if (a.grads == nullptr) throw InvalidArgument("Cannot call " + w + " without grads!");
    if (a.grads_out == nullptr || a.momentum_out == nullptr || a.stats_out == nullptr) throw InvalidArgument(w + ": no place for the result");
    if (n < 2) throw InvalidArgument(w + ": the statistics need at least 2 rows, got " + std::to_string(n));
    const float beta = a.beta ? *a.beta : md.cv_beta;
    if (!kern::cv_beta_ok(beta)) throw InvalidArgument(w + ": beta must lie in (0, 1), got " + std::to_string(beta));
    if (a.start_tree < 0 || a.start_tree > md.n_trees)
        throw InvalidArgument(w + ": start_tree_idx " + std::to_string(a.start_tree) + " is outside [0, " + std::to_string(md.n_trees) + "]");
    return beta;
}

// behind the staged rows: inputs up, the launches through `walk(scale, buffers)`, the results down, one wait
template <typename Walk>
void Engine::run_cv(const char *what, int n, const CvArgs &a, float beta, Walk &&walk) {
    const gbrl_hip_metadata &md = model.meta;
    const int D = md.output_dim, T = md.n_trees;
    const size_t n_el = static_cast<size_t>(n) * D, bytes = sizeof(float) * n_el;
    const float scale = kern::cv_scale(beta, T);
    if (a.scale_out) *a.scale_out = scale;
    if (a.n_trees_out) *a.n_trees_out = T;
    kern::CvBuffers b{};
    b.grads = staged(d_cv_grads_, a.grads, a.grads_dev, n_el, "H2D grads");
    b.momentum_in = a.momentum ? staged(d_cv_mom_in_, a.momentum, a.momentum_dev, n_el, "H2D momentum") : nullptr;
    b.grads_out = a.out_dev ? a.grads_out : static_cast<float *>(d_cv_grads_out_.ensure(bytes));
    b.momentum_out = a.out_dev ? a.momentum_out : static_cast<float *>(d_cv_mom_out_.ensure(bytes));
    const bool walks = T > 0 && (a.momentum != nullptr || a.start_tree < T);
    std::vector<float> stats(static_cast<size_t>(kern::kCvStats) * D, 0.0f);
    if (!walks) {   // the reference skips the correction: the gradients as they are, zero momentum, zero statistics
        hip_check(hipMemcpyAsync(b.grads_out, b.grads, bytes, hipMemcpyDeviceToDevice, stream_), "copy grads");
        hip_check(hipMemsetAsync(b.momentum_out, 0, bytes, stream_), "zero momentum");
        phase_end("inputs"); phase_begin(/*key=*/true);
        finish(what, "control_variates", {{a.out_dev ? nullptr : a.grads_out, b.grads_out, bytes, "D2H grads"},
                                          {a.out_dev ? nullptr : a.momentum_out, b.momentum_out, bytes, "D2H momentum"}});
        std::copy(stats.begin(), stats.end(), a.stats_out);
        return;
    }
    const int S1 = kern::cv_walk_slots(n), S2 = kern::cv_moment_slots(n), C = 2 * D;
    b.ms = static_cast<float *>(d_cv_ms_.ensure(bytes));
    double *part = static_cast<double *>(d_cv_part_.ensure(sizeof(double) * (static_cast<size_t>(S1) + S2 + 1) * C));
    b.slots = part;
    b.moments = part + static_cast<size_t>(S1) * C;
    b.totals = b.moments + static_cast<size_t>(S2) * C;
    b.stats = static_cast<float *>(d_cv_stats_.ensure(sizeof(float) * stats.size()));
    phase_end("inputs"); phase_begin(/*key=*/true);
    walk(scale, b);
    finish(what, "control_variates", {{stats.data(), b.stats, sizeof(float) * stats.size(), "D2H statistics"},
                                      {a.out_dev ? nullptr : a.grads_out, b.grads_out, bytes, "D2H grads"},
                                      {a.out_dev ? nullptr : a.momentum_out, b.momentum_out, bytes, "D2H momentum"}});
    for (int j = 0; j < D; ++j)
        if (!std::isfinite(stats[static_cast<size_t>(kern::kCvAlpha) * D + j]))
            throw InvalidArgument(std::string(what) + ": the coefficient of output " + std::to_string(j) + " is not finite (gradients or momentum hold a NaN or an infinity)");
    std::copy(stats.begin(), stats.end(), a.stats_out);
}

void Engine::control_variates(const float *obs, bool obs_dev, int n, int n_num, const CvArgs &a) {
    const char *what = "control_variates";
    const float beta = check_cv(what, n, a);
    const PredictBatch pb{obs, obs_dev, nullptr, false, nullptr, false, nullptr, n, n_num, 0};
    check_batch(pb, /*has_result=*/true, /*width_limit=*/true);
    const StagedBatch d = stage_batch(pb);
    const bool generic = hooks::on(hooks::CV_GENERIC);
    run_cv(what, n, a, beta, [&](float scale, const kern::CvBuffers &b) {
        kern::control_variates(mirror_view(), d.obs, n_num, n, a.start_tree, model.meta.n_trees, beta, scale, b, generic, stream_);
    });
}

void Engine::control_variates_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const CvArgs &a) {
    const char *what = "control_variates_prepared";
    check_prepared_dataset(what, ds);
    const float beta = check_cv(what, m, a);
    check_row_count(what, "grads", rows, m, ds->n, "correct");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    check_code_range(*ds, what, a.start_tree, model.meta.n_trees);
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const bool generic = hooks::on(hooks::CV_GENERIC);
    run_cv(what, m, a, beta, [&](float scale, const kern::CvBuffers &b) {
        kern::control_variates_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, a.start_tree, model.meta.n_trees,
                                     beta, scale, b, generic, stream_);
    });
}

}  // namespace gbrl
