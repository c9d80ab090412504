// engine_gram.hip -- the Gram matrix of the per-tree outputs (gram_core.h has the rule and the plan, tree_gram.hip the kernels):
//   Engine::tree_gram_prepared   the rows of a prepared data set, on the stages of engine_codes.hip (check_leaves_prepared, sync_code_tables, subset_rows):
//                                everything refused before the device is touched, one enqueue of two launches, one wait, the mirror on the host
//   Engine::tree_gram_host       gram_host_rule on host float rows from the host copy of the model; no device
//   Engine::scale_trees          the write side of the loop tree_gram_prepared -> solve -> scale_trees: leaf values times a weight per tree, host only
#include "engine_codes_detail.h"
#include "gram_core.h"
#include "hooks.h"

#include <cmath>

namespace gbrl {

namespace {
void check_gram_size(const std::string &w, int T, int D) {
    if (T > kern::kGramMaxTrees)
        throw Unsupported(w + ": " + std::to_string(T) + " trees; at most " + std::to_string(kern::kGramMaxTrees) + " per call (slice the tree range)");
    if (D > kern::kGramMaxD) throw Unsupported(w + ": output_dim > 128");
}
void check_gram_status(const std::string &w, int status) {
    if (status & kern::kGramBadValue) throw InvalidArgument(w + ": a leaf value of the range is not finite");
    if (status & kern::kGramBadTarget) throw InvalidArgument(w + ": targets hold a NaN or an infinity");
}
}  // namespace

void Engine::tree_gram_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *targets, bool targets_dev, int start_tree,
                                int stop_tree, double *gram_out, double *moment_out, int *route_out) {
    const char *what = "tree_gram_prepared";
    const std::string w(what);
    if (gram_out == nullptr || (targets != nullptr) != (moment_out != nullptr)) throw InvalidArgument(w + ": no place for the result");
    const int stop = check_leaves_prepared(what, ds, rows, rows_dev, m, start_tree, stop_tree);
    const int T = stop - start_tree, D = model.meta.output_dim;
    check_gram_size(w, T, D);
    const kern::GramPlan plan = kern::gram_plan(m, T, D, ds->code_groups());
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const float *d_y = targets ? staged(d_gram_y_, targets, targets_dev, static_cast<size_t>(m) * D, "H2D targets") : nullptr;
    double *part = static_cast<double *>(d_gram_part_.ensure(plan.scratch_bytes));
    double *tiles = static_cast<double *>(d_gram_tiles_.ensure(sizeof(double) * plan.per_block));
    int *status = zeroed<int>(d_gram_status_, 1, "zero gram status");
    phase_end("inputs"); phase_begin(/*key=*/true);
    const bool streamed = kern::tree_gram_codes(mirror_view(), ct, kern::CodeRows{ds->prep.d_codes, ds->n, ds->code_groups(), d_rows, 0}, m, start_tree, stop, d_y,
                                                part, tiles, status, hooks::on(hooks::GRAM_GENERIC), stream_);
    const size_t n_out = targets ? plan.per_block : plan.per_block - static_cast<size_t>(plan.chunks) * kern::kGramChunk;
    std::vector<double> h(plan.per_block, 0.0);
    int h_status = 0;
    finish("tree_gram_prepared launch", "predict", {{h.data(), tiles, sizeof(double) * n_out, "D2H gram tiles"}, {&h_status, status, sizeof(int), "D2H gram status"}});
    check_gram_status(w, h_status);
    kern::gram_assemble(h.data(), T, gram_out, moment_out);
    if (route_out) *route_out = streamed ? 1 : 0;
}

void Engine::tree_gram_host(const float *obs, int n, int n_num, const float *targets, int start_tree, int stop_tree, double *gram_out, double *moment_out) const {
    const std::string w("tree_gram_host");
    const gbrl_hip_metadata &md = model.meta;
    if (md.iteration > 0 && md.n_cat_features > 0) throw Unsupported(w + ": not available on a model with categorical columns");
    if (gram_out == nullptr || (targets != nullptr) != (moment_out != nullptr)) throw InvalidArgument(w + ": no place for the result");
    if (obs == nullptr) throw InvalidArgument("Cannot call tree_gram_host without observations!");
    if (n < 1) throw InvalidArgument(w + ": no rows");
    const int F = md.iteration > 0 ? md.n_num_features : md.input_dim;
    if (n_num != F) throw InvalidArgument("Incompatible dataset");
    if (start_tree < 0 || stop_tree < 0) throw InvalidArgument("invalid tree range");
    if (md.n_trees == 0) throw InvalidArgument(w + ": the model has no trees");
    const int stop = stop_tree == 0 ? md.n_trees : stop_tree;
    if (stop > md.n_trees || start_tree >= stop) throw InvalidArgument(w + ": invalid tree range");
    const int T = stop - start_tree, D = md.output_dim;
    check_gram_size(w, T, D);
    std::vector<double> g(static_cast<size_t>(T) * T), mo(static_cast<size_t>(T));
    const int status = kern::gram_host_rule(n, T, D, model.values.data(), [&](int r, int t) { return host_leaf(model, obs + static_cast<size_t>(r) * F, start_tree + t); },
                                            targets, g.data(), targets ? mo.data() : nullptr);
    check_gram_status(w, status);
    std::copy(g.begin(), g.end(), gram_out);
    if (moment_out) std::copy(mo.begin(), mo.end(), moment_out);
}

void Engine::scale_trees(const float *weights, int n_weights, int start_tree) {
    const std::string w("scale_trees");
    const int T = model.meta.n_trees, D = model.meta.output_dim;
    if (weights == nullptr || n_weights < 1) throw InvalidArgument("Cannot call scale_trees without weights!");
    if (start_tree < 0 || start_tree > T || n_weights > T - start_tree)
        throw InvalidArgument(w + ": the trees [" + std::to_string(start_tree) + ", " + std::to_string(static_cast<long long>(start_tree) + n_weights) +
                              ") are outside the model's " + std::to_string(T));
    for (int k = 0; k < n_weights; ++k)
        if (!std::isfinite(weights[k])) throw InvalidArgument(w + ": weight " + std::to_string(k) + " is not finite");
    for (int k = 0; k < n_weights; ++k) {
        const int t = start_tree + k;
        const size_t lo = static_cast<size_t>(model.tree_indices[t]) * D;
        const size_t hi = static_cast<size_t>(t + 1 < T ? model.tree_indices[t + 1] : model.meta.n_leaves) * D;
        for (size_t i = lo; i < hi; ++i) model.values[i] = model.values[i] * weights[k];
    }
    ++model.version;
    invalidate_mirror();
}

}  // namespace gbrl
