// engine_pd.hip -- partial dependence and ICE curves on a prepared data set (engine_step_detail.h lists the units beside it):
//   Engine::partial_dependence_codes     pd_core.h's break rule for one column of a threshold table, on the host: the codes at which the walked
//                                        trees can change their answer, [0] first
//   Engine::partial_dependence_prepared  the predictions of the trees [0, n_trees), walked from the bias, on the data set's rows with up to two
//                                        columns held at a constant code, for every variant of the caller's list: kern::pd_rows in launches of at
//                                        most kern::pd_launch_variants(m, D) variants, each finished by kern::staged_loss_finish_rows with
//                                        (variant, output) as its row axis, ONE read-back of the sums at the end (and of the ICE rows, when they
//                                        are bound for the host).  A column no condition of the walked trees tests is never read by the walk: it is
//                                        dropped from its variants, and a variant without a column is the baseline -- launched once.
// The checks are the ones the calls on a data set share: check_prepared_dataset, check_row_count / check_host_rows / subset_rows, check_code_range
// (the refusal, naming the tree, of a model the thresholds cannot express).  Neither the model nor the data set is written.
#include "engine_codes_detail.h"
#include "pd_core.h"

namespace gbrl {

namespace {

int resolve_stop(const std::string &w, int n_trees, int T) {
    if (T == 0) throw InvalidArgument(w + ": the model has no trees");
    if (n_trees != -1 && (n_trees < 1 || n_trees > T))
        throw InvalidArgument(w + ": n_trees " + std::to_string(n_trees) + " is outside [1, " + std::to_string(T) + "], the model's trees (None / -1: all)");
    return n_trees == -1 ? T : n_trees;
}

}  // namespace

void Engine::partial_dependence_codes(const float *thresholds, int F, int B, int col, int n_trees, int32_t *out, int *count) const {
    const std::string w("partial_dependence_codes");
    const gbrl_hip_metadata &md = model.meta;
    if (thresholds == nullptr || out == nullptr || count == nullptr) throw InvalidArgument(w + ": null argument");
    const int want_f = md.iteration > 0 ? md.n_num_features : md.input_dim;   // (condition_bins' checks of the table's shape)
    if (F != want_f) throw InvalidArgument(w + ": thresholds of " + std::to_string(F) + " features, the model has " + std::to_string(want_f) + " numeric features");
    if (B != md.n_bins) throw InvalidArgument(w + ": " + std::to_string(B) + " thresholds per feature, the model has n_bins = " + std::to_string(md.n_bins));
    if (col < 0 || col >= F) throw InvalidArgument(w + ": column " + std::to_string(col) + " is outside [0, " + std::to_string(F) + ")");
    const int stop = resolve_stop(w, n_trees, md.n_trees);
    // condition_bins' rule for the walked conditions on col alone: the cost is the column's conditions, not the model's
    const size_t S = walked_split_rows(model, stop), MD = md.max_depth;
    const float *thr = thresholds + static_cast<size_t>(col) * B;
    std::vector<int32_t> bins(std::max<size_t>(S * MD, 1), -1);
    for (size_t s = 0; s < S; ++s)
        for (size_t d = 0; d < MD && static_cast<int>(d) < model.depths[s]; ++d) {
            const size_t c = s * MD + d;
            if (!model.is_numerics[c] || model.feature_indices[c] != col) continue;
            const float v = model.feature_values[c];
            int32_t below = 0;
            bool found = false;
            for (int b = 0; b < B; ++b) {
                below += thr[b] < v ? 1 : 0;
                found = found || thr[b] == v;   // (NaN equals nothing)
            }
            if (!found) {
                const int tree = model.oblivious() ? static_cast<int>(s)
                                                   : static_cast<int>(std::upper_bound(model.tree_indices.begin(), model.tree_indices.end(), static_cast<int32_t>(s)) - model.tree_indices.begin()) - 1;
                throw Unsupported(w + ": tree " + std::to_string(tree) + ", condition " + std::to_string(d) + " (feature " + std::to_string(col) + " > " + std::to_string(v) +
                                  ") does not compare against one of the data set's thresholds of that feature: the bin codes cannot express it");
            }
            bins[c] = below;
        }
    const kern::PdConditions pc{model.depths.data(), model.feature_indices.data(), model.is_numerics.data(), bins.data(), static_cast<int>(MD)};
    const std::vector<int32_t> codes = kern::pd_break_codes(pc, S, col);
    std::copy(codes.begin(), codes.end(), out);   // (at most B + 1: a bin lies in [0, B))
    *count = static_cast<int>(codes.size());
}

void Engine::partial_dependence_prepared(const PreparedDataset *ds, const int32_t *variants, int V, const int32_t *rows, bool rows_dev, int m, int n_trees,
                                         double *sums_out, float *ice_out, bool ice_dev) {
    const char *what = "partial_dependence_prepared";
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    check_prepared_dataset(what, ds);
    if (md.output_dim > 128) throw Unsupported("predict: output_dim > 128");
    if (sums_out == nullptr) throw InvalidArgument(w + ": no place for the result");
    if (variants == nullptr || V < 1) throw InvalidArgument(w + ": no variants (at least one {col0, code0, col1, code1} is needed)");
    const int T = md.n_trees, D = md.output_dim, n = ds->n, F = ds->F, B = ds->n_bins;
    const int stop = resolve_stop(w, n_trees, T);
    check_row_count(what, "the call", rows, m, n, "evaluate");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, n);
    for (int v = 0; v < V; ++v) {
        const int32_t *q = variants + 4 * static_cast<size_t>(v);
        const std::string at = w + ": variant " + std::to_string(v);
        if (q[0] < -1 || q[0] >= F || q[2] < -1 || q[2] >= F)
            throw InvalidArgument(at + " names column " + std::to_string((q[0] < -1 || q[0] >= F) ? q[0] : q[2]) + ", outside [0, " + std::to_string(F) + ") (-1: none)");
        if (q[0] == -1 && q[2] != -1) throw InvalidArgument(at + ": col1 without col0 (the baseline is {-1, 0, -1, 0})");
        if (q[0] >= 0 && q[0] == q[2]) throw InvalidArgument(at + " names column " + std::to_string(q[0]) + " twice: a pair needs two distinct columns");
        for (int k = 0; k < 2; ++k)
            if (q[2 * k] >= 0 && (q[2 * k + 1] < 0 || q[2 * k + 1] > B))
                throw InvalidArgument(at + ": code " + std::to_string(q[2 * k + 1]) + " of column " + std::to_string(q[2 * k]) + " is outside [0, " + std::to_string(B) + "], the data set's codes");
    }
    const size_t row_el = static_cast<size_t>(m) * D;
    if (ice_out != nullptr && static_cast<unsigned long long>(V) * row_el >= (1ull << 31))
        throw Unsupported(w + ": the ICE rows of " + std::to_string(V) + " variants x " + std::to_string(m) + " rows x " + std::to_string(D) +
                          " outputs are 2^31 elements or more: pass rows= to evaluate fewer rows, or fewer features per call");
    check_code_range(*ds, what, 0, stop);
    const std::vector<uint8_t> used = walked_columns(model, stop, F);   // the columns the walk of [0, stop) reads: permutation importance's rule
    const bool walks = !model.opts.empty();   // no optimizer owns an output (PredictModel::n_opts == 0): no tree applies a value, every variant is the baseline
    // what is launched: every variant with its unread columns dropped; the variants left without a column share ONE baseline
    std::vector<kern::PdVariant> launched;
    std::vector<int32_t> slots;                                   // the caller's variant whose ICE block a launched variant writes
    std::vector<int> launch_of(static_cast<size_t>(V), -1);
    int baseline = -1;
    for (int v = 0; v < V; ++v) {
        const int32_t *q = variants + 4 * static_cast<size_t>(v);
        kern::PdVariant pv{-1, 0, -1, 0};
        if (walks && q[0] >= 0 && used[q[0]]) { pv.col0 = q[0]; pv.code0 = q[1]; }
        if (walks && q[2] >= 0 && used[q[2]]) {
            if (pv.col0 < 0) { pv.col0 = q[2]; pv.code0 = q[3]; }
            else { pv.col1 = q[2]; pv.code1 = q[3]; }
        }
        if (pv.col0 < 0 && baseline >= 0) { launch_of[v] = baseline; continue; }
        if (pv.col0 < 0) baseline = static_cast<int>(launched.size());
        launch_of[v] = static_cast<int>(launched.size());
        launched.push_back(pv);
        slots.push_back(v);
    }
    const long long L = static_cast<long long>(launched.size());
    if (L > kern::kPdMaxVariants) throw InvalidArgument(w + ": " + std::to_string(L) + " launched variants: at most 2^20 in one call");
    ensure_device();
    reset_events();
    sync_model_to_device();
    phase_begin();
    const kern::PredictModel pm = mirror_view();
    const kern::CodeTables ct = sync_code_tables(*ds);
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    const int nb = kern::pd_partials(m), per_launch = kern::pd_launch_variants(m, D);
    const kern::PdVariant *d_var = upload(d_pd_variants_, launched.data(), launched.size(), "H2D variants");
    const int32_t *d_slots = ice_out ? upload(d_pd_slots_, slots.data(), slots.size(), "H2D slots") : nullptr;
    double *d_part = static_cast<double *>(d_pd_part_.ensure(sizeof(double) * static_cast<size_t>(std::min<long long>(L, per_launch)) * D * nb));
    double *d_sums = static_cast<double *>(d_pd_sums_.ensure(sizeof(double) * static_cast<size_t>(L) * D));
    const size_t ice_bytes = sizeof(float) * static_cast<size_t>(V) * row_el;
    struct Release { DevBuf &buf; ~Release() { buf.release(); } } release_ice{d_pd_ice_};   // the host-bound ICE block (up to 8 GiB) does not outlive the call
    float *d_ice = ice_out == nullptr ? nullptr : ice_dev ? ice_out : static_cast<float *>(d_pd_ice_.ensure(ice_bytes));
    phase_end("inputs"); phase_begin(/*key=*/true);
    const bool generic = hooks::on(hooks::PD_GENERIC) || !walks;
    const kern::CodeRows cr{ds->prep.d_codes, n, ds->code_groups(), d_rows, 0};
    for (long long v0 = 0; v0 < L; v0 += per_launch) {
        const int count = static_cast<int>(std::min<long long>(per_launch, L - v0));
        kern::pd_rows(pm, ct, cr, m, stop, d_var + v0, d_slots ? d_slots + v0 : nullptr, count, d_part, d_ice, generic, stream_);
        kern::staged_loss_finish_rows(d_part, nb, count * D, d_sums + v0 * D, stream_);
    }
    if (d_ice != nullptr)   // a variant that was not launched holds the rows of the one that stands for it
        for (int v = 0; v < V; ++v)
            if (slots[launch_of[v]] != v)
                hip_check(hipMemcpyAsync(d_ice + static_cast<size_t>(v) * row_el, d_ice + static_cast<size_t>(slots[launch_of[v]]) * row_el, sizeof(float) * row_el,
                                         hipMemcpyDeviceToDevice, stream_), "D2D ICE rows");
    std::vector<double> sums(static_cast<size_t>(L) * D, 0.0);
    finish("partial_dependence_prepared launch", "pd_rows",
           {{sums.data(), d_sums, sizeof(double) * sums.size(), "D2H sums"}, {ice_dev ? nullptr : ice_out, d_ice, ice_bytes, "D2H ICE rows"}});
    for (int v = 0; v < V; ++v) std::copy_n(sums.data() + static_cast<size_t>(launch_of[v]) * D, D, sums_out + static_cast<size_t>(v) * D);
}

}  // namespace gbrl
