// engine_importance.hip -- permutation importance on a prepared data set (engine_step_detail.h lists the units beside it):
//   Engine::permutation_host                 perm_core.h's rule on the host: the row a variant's row reads its shuffled column from
//   Engine::permutation_importance_prepared  the loss of the trees [0, n_trees) on the data set's rows as they are (the baseline) and with one
//                                            column shuffled, for every (column, repeat): kern::perm_loss in launches of at most
//                                            kern::kPermLaunchVariants variants, each finished by kern::staged_loss_finish_rows (the loss paths'
//                                            fixed order), ONE read-back of the sums at the end.  A column that no condition of the walked trees
//                                            tests is never read by the walk: its variants are not launched and report the baseline.
// The checks are the ones the calls on a data set share: check_prepared_dataset, check_code_range (the refusal, naming the tree, of a model the
// thresholds cannot express), the objective's checks of engine_objective.hip, check_cols.  Neither the model nor the data set is written.
#include "engine_codes_detail.h"
#include "perm_core.h"

namespace gbrl {

void Engine::permutation_host(int n, uint64_t seed, int col, int repeat, int32_t *out) {
    if (out == nullptr) throw InvalidArgument("permutation_host: null output");
    if (n < 1) throw InvalidArgument("permutation_host: no rows (n must be positive)");
    if (col < 0) throw InvalidArgument("permutation_host: col must be >= 0");
    if (repeat < 0) throw InvalidArgument("permutation_host: repeat must be >= 0");
    const kern::PermPlan pp = kern::perm_plan(static_cast<uint32_t>(n), seed, col, repeat);
    for (int i = 0; i < n; ++i) out[i] = static_cast<int32_t>(kern::perm_at(pp, static_cast<uint32_t>(i)));
}

void Engine::permutation_importance_prepared(const PreparedDataset *ds, const void *targets, bool targets_dev, int objective, const float *alpha, int n_repeats,
                                             uint64_t seed, const int32_t *cols, int n_cols, int n_trees, double *baseline_out, double *loss_out) {
    const char *what = "permutation_importance_prepared";
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    check_prepared_dataset(what, ds);
    if (md.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    if (baseline_out == nullptr || loss_out == nullptr) throw InvalidArgument(w + ": no place for the result");
    if (n_repeats < 1) throw InvalidArgument(w + ": n_repeats must be >= 1, got " + std::to_string(n_repeats));
    if (cols != nullptr) check_cols(what, cols, n_cols, ds->F);
    else n_cols = ds->F;
    const int T = md.n_trees, D = md.output_dim, n = ds->n, F = ds->F;
    if (T == 0) throw InvalidArgument(w + ": the model has no trees");
    if (n_trees != -1 && (n_trees < 1 || n_trees > T))
        throw InvalidArgument(w + ": n_trees " + std::to_string(n_trees) + " is outside [1, " + std::to_string(T) + "], the model's trees (None / -1: all)");
    const int stop = n_trees == -1 ? T : n_trees;
    if (targets == nullptr) throw InvalidArgument("Cannot call " + w + " without targets!");
    check_objective(what, objective, D);
    check_alpha(what, objective, alpha, D, false);
    const long long total = static_cast<long long>(n_cols) * n_repeats;
    if (total > (1ll << 24)) throw InvalidArgument(w + ": " + std::to_string(total) + " variants (columns x n_repeats): at most 2^24 in one call");
    check_code_range(*ds, what, 0, stop);
    // the columns the walk of [0, stop) reads (greedy: through the trees a trailing run of one-leaf trees runs on into, as check_code_range counts them)
    const std::vector<uint8_t> used = walked_columns(model, stop, F);
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::PredictModel pm = mirror_view();
    const bool walks = pm.n_opts > 0;   // no optimizer owns an output: no tree applies a value, every variant is the baseline
    const kern::CodeTables ct = sync_code_tables(*ds);
    const size_t tar_el = objective == kern::kObjSoftmax ? static_cast<size_t>(n) : static_cast<size_t>(n) * D;
    const float *dt = staged(d_pi_targets_, static_cast<const float *>(targets), targets_dev, tar_el, "H2D targets");
    if (objective == kern::kObjSoftmax) check_labels(what, reinterpret_cast<const int32_t *>(dt), n, D, nullptr);
    const float *da = alpha ? upload(d_lq_alpha_, alpha, static_cast<size_t>(D), "H2D levels") : nullptr;
    // variant 0 is the baseline; then (column, repeat) for every named column the walk reads, columns in the caller's order
    std::vector<kern::PermVariant> variants;
    std::vector<int> first_of(static_cast<size_t>(n_cols), -1);   // the column's first variant (-1: not launched)
    variants.push_back(kern::PermVariant{-1, 0});
    for (int c = 0; c < n_cols; ++c) {
        const int col = cols ? cols[c] : c;
        if (!walks || !used[col]) continue;
        first_of[c] = static_cast<int>(variants.size());
        for (int r = 0; r < n_repeats; ++r) variants.push_back(kern::PermVariant{col, r});
    }
    const int V = static_cast<int>(variants.size()), nb = kern::staged_loss_partials(n);
    const kern::PermVariant *d_var = upload(d_pi_variants_, variants.data(), variants.size(), "H2D variants");
    double *d_part = static_cast<double *>(d_pi_part_.ensure(sizeof(double) * static_cast<size_t>(std::min(V, kern::kPermLaunchVariants)) * nb));
    double *d_sums = static_cast<double *>(d_pi_sums_.ensure(sizeof(double) * static_cast<size_t>(V)));
    phase_end("inputs"); phase_begin(/*key=*/true);
    const bool generic = hooks::on(hooks::PERM_GENERIC) || !walks;
    for (int v0 = 0; v0 < V; v0 += kern::kPermLaunchVariants) {
        const int count = std::min(kern::kPermLaunchVariants, V - v0);
        kern::perm_loss(pm, ct, ds->prep.d_codes, n, ds->code_groups(), stop, objective, dt, da, seed, d_var + v0, count, d_part, generic, stream_);
        kern::staged_loss_finish_rows(d_part, nb, count, d_sums + v0, stream_);
    }
    std::vector<double> sums(static_cast<size_t>(V), 0.0);
    finish("permutation_importance_prepared launch", "perm_loss", {{sums.data(), d_sums, sizeof(double) * sums.size(), "D2H losses"}});
    const double rows = static_cast<double>(n);
    const double baseline = mean_loss(objective, sums[0], rows);
    *baseline_out = baseline;
    for (int c = 0; c < n_cols; ++c)
        for (int r = 0; r < n_repeats; ++r)
            loss_out[static_cast<size_t>(c) * n_repeats + r] = first_of[c] < 0 ? baseline : mean_loss(objective, sums[static_cast<size_t>(first_of[c]) + r], rows);
}

}  // namespace gbrl
