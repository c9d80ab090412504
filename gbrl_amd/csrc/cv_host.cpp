// cv_host.cpp -- Engine::control_variates_host: cv_core.h's rule on host float32 rows from the host copy of the model, no device.  The walk is
// predict_rowwalk.h's general_leaf restated for the host: the bytes control_variates.hip must produce.
#include "cv_core.h"
#include "engine.h"

#include <cmath>
#include <vector>

namespace gbrl {

// the global leaf of (row, tree t); greedy: the first leaf in storage order from the tree's first on whose conditions all hold (a depth-0 leaf never
// passes, so the search walks on into the next tree); -1 when it runs off the ensemble.  Declared in engine.h: tree_gram_host walks with it too.
int host_leaf(const Model &m, const float *x, int t) {
    const int md = m.meta.max_depth;
    if (m.oblivious()) {
        const int depth = m.depths[t], cond = t * md;
        int l = 0;
        for (int d = 0; d < depth; ++d) l |= (x[m.feature_indices[cond + d]] > m.feature_values[cond + d] ? 1 : 0) << (depth - 1 - d);
        return m.tree_indices[t] + l;
    }
    for (int leaf = m.tree_indices[t]; leaf < m.meta.n_leaves; ++leaf) {
        const int depth = m.depths[leaf], cond = leaf * md;
        bool passed = false;
        for (int d = depth - 1; d >= 0; --d) {
            passed = (x[m.feature_indices[cond + d]] > m.feature_values[cond + d]) == (m.inequality_directions[cond + d] != 0);
            if (!passed) break;
        }
        if (passed) return leaf;
    }
    return -1;
}

void Engine::control_variates_host(const float *obs, int n, int n_num, const CvArgs &a) const {
    const char *what = "control_variates_host";
    const gbrl_hip_metadata &md = model.meta;
    const float beta = check_cv(what, n, a);
    const int F = md.iteration > 0 ? md.n_num_features : md.input_dim;
    if (obs == nullptr) throw InvalidArgument("Cannot call control_variates_host without observations!");
    if (n_num != F) throw InvalidArgument("Incompatible dataset");
    const int D = md.output_dim, T = md.n_trees;
    const size_t n_el = static_cast<size_t>(n) * D;
    const float scale = kern::cv_scale(beta, T), c = kern::cv_sub(1.0f, beta);
    if (a.scale_out) *a.scale_out = scale;
    if (a.n_trees_out) *a.n_trees_out = T;
    std::fill(a.stats_out, a.stats_out + static_cast<size_t>(kern::kCvStats) * D, 0.0f);
    if (!(T > 0 && (a.momentum != nullptr || a.start_tree < T))) {
        std::copy(a.grads, a.grads + n_el, a.grads_out);
        std::fill(a.momentum_out, a.momentum_out + n_el, 0.0f);
        return;
    }
    for (int r = 0; r < n; ++r) {
        float *m = a.momentum_out + static_cast<size_t>(r) * D;
        for (int j = 0; j < D; ++j) m[j] = a.momentum ? a.momentum[static_cast<size_t>(r) * D + j] : 0.0f;
        const float *x = obs + static_cast<size_t>(r) * F;
        for (int t = a.start_tree; t < T; ++t) {
            const int leaf = host_leaf(model, x, t);
            if (leaf < 0) break;
            const float *v = model.values.data() + static_cast<size_t>(leaf) * D;
            for (int j = 0; j < D; ++j) m[j] = kern::cv_chain(m[j], beta, c, v[j]);
        }
    }
    std::vector<float> ms(n_el), stats(static_cast<size_t>(kern::kCvStats) * D);
    std::vector<double> part(static_cast<size_t>(kern::cv_walk_slots(n)) * 2 * D);
    kern::cv_finish_host(a.grads, a.momentum_out, n, D, scale, ms.data(), part.data(), a.grads_out, stats.data());
    for (int j = 0; j < D; ++j)
        if (!std::isfinite(stats[static_cast<size_t>(kern::kCvAlpha) * D + j]))
            throw InvalidArgument(std::string(what) + ": the coefficient of output " + std::to_string(j) + " is not finite (gradients or momentum hold a NaN or an infinity)");
    std::copy(stats.begin(), stats.end(), a.stats_out);
}

}  // namespace gbrl
