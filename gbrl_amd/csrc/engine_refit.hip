// engine_refit.hip -- GBRL::refit_leaves (see engine.h).  The call goes through the stages of engine_predict.hip like every predict-family call; what
// is its own is the order of its checks, its kernels, its three read-backs and the booking of the new values.
#include "engine.h"
#include "hooks.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace gbrl {

// The checks that are refit_leaves' own; returns the resolved stop (stop_tree == 0: n_trees).
int Engine::check_refit(int start_tree, int stop_tree, const float *targets, double decay_rate, const double *loss_out) const {
    const gbrl_hip_metadata &md = model.meta;
    if (md.n_trees == 0) throw InvalidArgument("refit_leaves: the model has no trees");
    const int stop = stop_tree == 0 ? md.n_trees : stop_tree;
    if (start_tree < 0 || stop_tree < 0 || stop > md.n_trees || start_tree >= stop)
        throw InvalidArgument("refit_leaves: invalid tree range [" + std::to_string(start_tree) + ", " + std::to_string(stop_tree) + ") for " + std::to_string(md.n_trees) + " trees");
    if (targets == nullptr) throw InvalidArgument("Cannot call refit_leaves without targets!");
    if (loss_out == nullptr) throw InvalidArgument("refit_leaves: no place for the loss");
    if (!(decay_rate >= 0.0 && decay_rate <= 1.0)) throw InvalidArgument("refit_leaves: decay_rate must be in [0, 1]");
    // the leaf sums of a row-sharded model would need an exchange per tree: out of scope
    if (has_coll_ || rccl_comm_ != nullptr) throw Unsupported("refit_leaves: not available on a model with a communicator or collective hooks (row-sharded refit)");
    // A greedy leaf of depth 0 never passes (Q7): predict_continue's walk then applies a leaf of the NEXT tree at this tree's rate, a value the
    // refit has not computed yet when it gets there.  The chain the contract names cannot be followed through such a tree, so the call is
    // refused when one lies in [start - 1, stop): inside the range, or right in front of it, where the prefix prediction would apply an OLD value
    // of tree `start`.  Further in front the walk touches unchanged trees only.  (An oblivious stump is routed to and simply keeps its value.)
    if (!model.oblivious())
        for (int t = std::max(0, start_tree - 1); t < stop; ++t) {
            const int l0 = model.tree_indices[t], l1 = t + 1 < md.n_trees ? model.tree_indices[t + 1] : md.n_leaves;
            for (int l = l0; l < l1; ++l)
                if (model.depths[l] == 0)
                    throw Unsupported("refit_leaves: greedy tree " + std::to_string(t) + " has a leaf of depth 0, which no row reaches: the prediction walks on into the next tree there, whose new values are not known yet");
        }
    return stop;
}

// Extension: the leaf values of [start_tree, stop_tree) fitted again on this batch (kern::refit_leaves).  The checks that are the call's own come
// first -- a model without trees must not be touched by check_batch's first-use bookkeeping.
void Engine::refit_leaves(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *targets, bool targets_dev, int n, int n_num, int n_cat,
                          int start_tree, int stop_tree, double decay_rate, double *loss_out) {
    const gbrl_hip_metadata &md = model.meta;
    const int stop = check_refit(start_tree, stop_tree, targets, decay_rate, loss_out);
    const PredictBatch b{obs, obs_dev, cat, cat_dev, nullptr, false, nullptr, n, n_num, n_cat};
    check_batch(b, /*has_result=*/true, /*width_limit=*/true);
    const StagedBatch d = stage_batch(b);
    const float *dtargets = stage_targets(targets, targets_dev, n);
    phase_end("inputs"); phase_begin(/*key=*/true);
    hipStream_t s = stream_;
    const int D = md.output_dim;
    // the whole range is ONE enqueue: nothing is read back between the trees, the host waits once, and the model -- host copy and mirror -- is
    // written only after every gmax of the run has been seen finite
    const size_t T = static_cast<size_t>(stop - start_tree);
    const size_t l0 = static_cast<size_t>(model.tree_indices[start_tree]);
    const size_t l1 = stop < md.n_trees ? static_cast<size_t>(model.tree_indices[stop]) : static_cast<size_t>(md.n_leaves);
    const size_t NL = l1 - l0, acc_bytes = sizeof(unsigned long long) * NL * (D + 1);
    float *dP = static_cast<float *>(d_refit_p_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
    int32_t *dleaf = static_cast<int32_t *>(d_refit_leaf_.ensure(sizeof(int32_t) * static_cast<size_t>(n)));
    unsigned long long *dacc = static_cast<unsigned long long *>(d_refit_acc_.ensure(std::max<size_t>(acc_bytes, 8)));
    float *dvals = static_cast<float *>(d_refit_values_.ensure(sizeof(float) * std::max<size_t>(NL * D, 1)));
    uint32_t *dgmax = static_cast<uint32_t *>(d_refit_gmax_.ensure(sizeof(uint32_t) * (T + 1)));   // before each tree, and of the final prediction
    double *dpart = static_cast<double *>(d_staged_part_.ensure(sizeof(double) * kern::staged_loss_partials(n)));
    double *dsum = static_cast<double *>(d_staged_sums_.ensure(sizeof(double)));
    hip_check(hipMemsetAsync(dacc, 0, acc_bytes, s), "zero leaf sums");
    hip_check(hipMemsetAsync(dgmax, 0, sizeof(uint32_t) * (T + 1), s), "zero gradient maxima");
    const int streamed = kern::refit_leaves(mirror_view(), model.tree_indices.data(), d.obs, n_num, d.cat, n_cat, n, start_tree, stop, decay_rate, dtargets, dP, dleaf, dacc, dvals, dgmax,
                                            hooks::on(hooks::REFIT_GENERIC), s);
    kern::staged_loss_of_predictions(dP, dtargets, n, D, dpart, dsum, s);
    std::vector<float> hvals(NL * D);
    std::vector<uint32_t> hgmax(T + 1);
    double sum = 0.0;
    finish("refit_leaves launch", "refit", {{hvals.data(), dvals, sizeof(float) * NL * D, "D2H refitted values"},
                                            {hgmax.data(), dgmax, sizeof(uint32_t) * (T + 1), "D2H gradient maxima"},
                                            {&sum, dsum, sizeof(double), "D2H loss sum"}});
    if (profiling_) phases_.emplace_back("refit_streamed_trees", static_cast<float>(streamed));   // (not a time: trees whose sums the streaming kernel took)
    for (size_t i = 0; i <= T; ++i)
        if (hgmax[i] >= 0x7f800000u)
            throw InvalidArgument((i < T ? "refit_leaves: the gradient of tree " + std::to_string(start_tree + static_cast<int>(i)) : std::string("refit_leaves: the final prediction")) +
                                  " is not finite (non-finite targets or an overflowing prediction); the model is unchanged");
    std::copy(hvals.begin(), hvals.end(), model.values.begin() + static_cast<long>(l0 * D));
    ++model.version;
    invalidate_mirror();
    *loss_out = std::sqrt(0.5 * sum / static_cast<double>(n));   // staged_loss's expression
}

}  // namespace gbrl
