// Host-only check of gbrl_amd/csrc/path_core.h (compiled with the address and undefined-behaviour sanitizers and run by tests/test_path_host.py):
// the delta table built tree by tree under the engine's mark (with rewind_values-style steps back) against the table built in one go, and the
// invariants of the slot plan.
#include "path_core.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace gbrl;
using namespace gbrl::kern;

#define CHECK(cond, what) do { if (!(cond)) { std::printf("MISMATCH %s (line %d)\n", what, __LINE__); std::exit(1); } } while (0)

using Rng = std::mt19937_64;
static size_t pick(Rng &rng, size_t n) { return static_cast<size_t>(rng() % n); }

static Model new_model(bool greedy, int MD, int D, int F) {
    Model m;
    m.meta.max_depth = MD; m.meta.output_dim = D; m.meta.n_num_features = F; m.meta.input_dim = F;
    m.meta.grow_policy = greedy ? GBRL_HIP_GROW_GREEDY : GBRL_HIP_GROW_OBLIVIOUS;
    m.bias.assign(D, 0.25f);
    gbrl_hip_optimizer a{}, b{};
    a.algo = GBRL_HIP_ALGO_SGD; a.scheduler = GBRL_HIP_SCHED_CONST; a.init_lr = 0.1f; a.start_idx = 0; a.stop_idx = std::max(1, D - 1);
    b = a; b.scheduler = GBRL_HIP_SCHED_LINEAR; b.init_lr = 0.3f; b.stop_lr = 0.01f; b.T = 7; b.start_idx = a.stop_idx; b.stop_idx = D;
    m.opts = {a, b};
    return m;
}
static void add_split_row(Model &m) { m.depths.push_back(0); m.feature_indices.resize(m.depths.size() * m.meta.max_depth, 0); }
// a random proper binary shape (greedy) or a full tree of `depth` levels (oblivious): leaves depth-first and left first, every leaf with the
// directions and edge weights of its path (the two edges of a node sum to 1) and, greedy, the features of its path
static void grow(Model &m, Rng &rng, int depth, std::vector<int> &feat, std::vector<uint8_t> &dirs, std::vector<float> &w) {
    const bool greedy = !m.oblivious();
    const size_t d = dirs.size(), MD = m.meta.max_depth, D = m.meta.output_dim;
    if (greedy ? (d == MD || (d >= 1 && pick(rng, 3) == 0)) : static_cast<int>(d) == depth) {
        if (greedy) { add_split_row(m); m.depths.back() = static_cast<int>(d); }
        const size_t l = static_cast<size_t>(m.meta.n_leaves++);
        for (size_t j = 0; j < D; ++j) m.values.push_back(static_cast<float>(static_cast<int>(pick(rng, 4001)) - 2000) / 128.0f);
        m.inequality_directions.resize((l + 1) * MD, 0);
        m.edge_weights.resize((l + 1) * MD, 0.0f);
        for (size_t k = 0; k < d; ++k) {
            if (greedy) m.feature_indices[l * MD + k] = feat[k];
            m.inequality_directions[l * MD + k] = dirs[k];
            m.edge_weights[l * MD + k] = w[k];
        }
        return;
    }
    feat.push_back(static_cast<int>(pick(rng, m.meta.n_num_features)));
    const float left = static_cast<float>(1 + pick(rng, 9)) / 10.0f;
    for (uint8_t dir = 0; dir < 2; ++dir) {
        dirs.push_back(dir); w.push_back(dir == 0 ? left : 1.0f - left);
        grow(m, rng, depth, feat, dirs, w);
        dirs.pop_back(); w.pop_back();
    }
    feat.pop_back();
}
static void add_tree(Model &m, Rng &rng) {
    const size_t t = static_cast<size_t>(m.meta.n_trees++), MD = m.meta.max_depth;
    m.tree_indices.push_back(m.meta.n_leaves);
    int depth = 0;
    if (m.oblivious()) {
        add_split_row(m);
        m.depths[t] = depth = static_cast<int>(pick(rng, MD + 1));   // (depth 0: one leaf, no decision)
        for (int k = 0; k < depth; ++k) m.feature_indices[t * MD + k] = static_cast<int>(pick(rng, m.meta.n_num_features));
    }
    std::vector<int> feat; std::vector<uint8_t> dirs; std::vector<float> w;
    grow(m, rng, depth, feat, dirs, w);
}

static void same_tables(const PathTable &a, const PathTable &b) {
    CHECK(a.delta.size() == b.delta.size() && a.root.size() == b.root.size() && a.bad_tree == b.bad_tree, "table sizes");
    CHECK(a.delta.empty() || std::memcmp(a.delta.data(), b.delta.data(), a.delta.size() * sizeof(float)) == 0, "delta bytes");
    CHECK(a.root.empty() || std::memcmp(a.root.data(), b.root.data(), a.root.size() * sizeof(double)) == 0, "root bytes");
}

int main() {
    for (uint64_t seed = 1; seed <= 40; ++seed) {
        Rng rng(seed);
        Model m = new_model(seed % 2 == 0, 1 + static_cast<int>(pick(rng, 6)), 1 + static_cast<int>(pick(rng, 9)), 1 + static_cast<int>(pick(rng, 20)));
        PathTable inc, whole;
        size_t mark = 0;
        for (int round = 0; round < 6; ++round) {
            for (size_t k = pick(rng, 4); k > 0; --k) add_tree(m, rng);
            if (m.meta.n_trees > 0 && pick(rng, 3) == 0) {   // the values of one tree change: the mark goes back to it (rewind_values)
                const int t = static_cast<int>(pick(rng, m.meta.n_trees));
                for (size_t l = m.first_leaf(t); l < m.first_leaf(t) + m.leaf_count(t); ++l) m.values[l * m.meta.output_dim] += 1.5f;
                mark = std::min(mark, static_cast<size_t>(t));
            }
            if (round == 4) m.opts[0].init_lr = 0.2f;        // other optimizers: the table starts over by itself
            inc.extend(m, mark);
            mark = static_cast<size_t>(m.meta.n_trees);
            whole = PathTable();
            whole.extend(m, 0);
            same_tables(inc, whole);
            CHECK(whole.bad_tree == -1, "a proper tree was refused");
        }
    }
    std::printf("incremental table: 40 ensembles, tables equal\n");
    for (int D = 1; D <= 70; ++D)
        for (int G : {1, 2, 8, 63, 400, 1000})
            for (int n_used : {0, 1, 2, 9, 10, 61, 62, 63, 128, 1000, 16000}) {
                const PathSlotPlan p = path_slot_plan(n_used, G, D);
                const size_t tile = path_code_tile_bytes(G), slot = path_slot_bytes(D);
                CHECK(p.fits == (D <= 64 && tile + slot <= kStreamLdsBudget), "fits");
                if (!p.fits) { CHECK(p.slots == 0 && p.passes == 0, "no plan"); continue; }
                CHECK(p.slots >= 1 && p.lds == tile + p.slots * slot && p.lds <= kStreamLdsBudget, "LDS within the opt-in limit");
                CHECK(p.slots == std::max(n_used, 1) || tile + (p.slots + 1) * slot > kStreamLdsBudget, "as many slots as fit");
                CHECK(n_used == 0 ? p.passes == 0 : (p.passes >= 1 && static_cast<long>(p.passes) * p.slots >= n_used && static_cast<long>(p.passes - 1) * p.slots < n_used),
                      "every used feature in exactly one pass, none without a used feature");
            }
    std::printf("slot plan: invariants hold\nall sections passed\n");
    return 0;
}
