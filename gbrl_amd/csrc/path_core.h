// path_core.h -- path attribution (Saabas) of the ensemble, the rule written once for host and device (engine_path.hip calls it, path_rows.hip has
// the kernels, explain.cpp the host evaluation; the host half needs no device and no HIP header: tests/cxx/path_core_check.cpp compiles it alone).
//
// The rule.  A row's prediction is split among the features tested on its root-to-leaf paths.  For tree t and a leaf l of depth k the path nodes
// are n_0 (root) .. n_k (the leaf), the condition at depth j tests feature f_j, and E(n) is the cover-weighted mean of the leaf values below n
// (float64; the cover of a leaf is the product of its edge weights, the weights TreeSHAP reads; E of a leaf is its value).
//   delta[l][j][d] = fl32(-lr_d(t) * (E(n_{j+1})[d] - E(n_j)[d]))   j < k, float32 [n_leaves][max_depth][D], the product rounded once from float64
//   lr_d(t)        = the float64 sum of scheduler_lr(o, t) over the optimizers o that own output d, in order: what predict applies; 0 without owner
//   phi[r][f][d]   = the float32 sum, in tree order and then depth order, of delta[leaf_t(r)][j][d] over the trees of the range and the depths j with
//                    f_j == f; plain float32 adds (path_add: nothing can contract)
//   expected[d]    = bias[d] + sum_t -lr_d(t) * E(root_t)[d] in float64
// so that sum_f phi[r][f][d] + expected[d] is the prediction of the range up to float32 rounding.
//
//   PathTable      the delta table and the root terms, appended tree by tree like the mirror's records (mirror_records.h)
//   path_used      the features a tree range tests, ascending: the dense SLOTS of the streaming kernel (an untested column costs nothing)
//   path_slot_plan how many slots a pass of the streaming kernel keeps in LDS behind the code tile, and how many passes the used features need
//   path_launch_tiles  how many tiles of 64 rows a launch of the importance form takes, from the scratch budget
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_accum.h"
#include "model.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_PATH_HD __host__ __device__
#else
#define GBRL_PATH_HD
#endif

namespace gbrl {
namespace kern {

// one term joins a contribution: a float32 add, never part of a fused multiply-add
GBRL_PATH_HD inline float path_add(float acc, float delta) {
#pragma clang fp contract(off)
    return acc + delta;
}

constexpr int kPathRows = 64;                           // rows per tile = one wave = one float64 partial (kShapTileRows)
constexpr size_t kPathScratchBudget = size_t(64) << 20;   // bytes of partials (streaming) or of float32 scratch (general) per launch (= kPdScratchBudget)

// ------------------------------------------------------------------------------------------------------------ the delta table
struct PathTable {
    std::vector<float> delta;    // [n_leaves][max_depth][D]; 0 at and below a leaf's depth
    std::vector<double> root;    // [n_trees][D]: -lr_d(t) * E(root_t)[d]
    std::vector<gbrl_hip_optimizer> opts;   // the optimizers the table was built from
    int bad_tree = -1;           // the first tree whose leaves do not form a proper binary tree (or a greedy tree of one leaf, Q7): no rule for it

    // `built` trees are current; the rows of [built, n_trees) are (re)built.  Starts over when the optimizers are not the ones the table was built
    // from or the ensemble has shrunk below the mark.  Returns the first tree that was (re)built.
    size_t extend(const Model &model, size_t built) {
        const size_t T = model.meta.n_trees, MD = model.meta.max_depth, D = model.meta.output_dim, NO = model.opts.size();
        const bool same = opts.size() == NO && std::equal(opts.begin(), opts.end(), model.opts.begin(), [](const gbrl_hip_optimizer &a, const gbrl_hip_optimizer &b) {
                              return std::memcmp(&a, &b, sizeof(a)) == 0;
                          });
        if (!same || built > T) { built = 0; opts = model.opts; }
        if (bad_tree >= static_cast<int>(built)) bad_tree = -1;
        delta.resize(static_cast<size_t>(model.meta.n_leaves) * MD * D);
        root.resize(T * D);
        for (size_t t = built; t < T; ++t)
            if (!put_tree(model, static_cast<int>(t)) && bad_tree < 0) bad_tree = static_cast<int>(t);
        return built;
    }

    // expected[d] of the trees [0, n_trees)
    void expected(const Model &model, int n_trees, double *out) const {
#pragma clang fp contract(off)
        const size_t D = model.meta.output_dim;
        for (size_t d = 0; d < D; ++d) {
            double e = static_cast<double>(model.bias[d]);
            for (int t = 0; t < n_trees; ++t) e = e + root[static_cast<size_t>(t) * D + d];
            out[d] = e;
        }
    }

    static double rate(const Model &model, int t, int d) {
        double lr = 0.0;
        for (const gbrl_hip_optimizer &o : model.opts)
            if (d >= o.start_idx && d < o.stop_idx) lr += static_cast<double>(scheduler_lr(o, t));
        return lr;
    }

   private:
    struct Build {
        const Model &m;
        int t, l0, MD, D;
        std::vector<double> E;   // [leaves of the tree][MD + 1][D]: E of the node at depth j above (or at) the leaf
        bool ok = true;
    };

    static int leaf_depth(const Build &b, int leaf) { return b.m.oblivious() ? b.m.depths[b.t] : b.m.depths[leaf]; }

    // the leaves [lo, hi) share their first d decisions; writes the node's E into the rows of its leaves, returns its cover, adds cover * E to sum
    static double walk(Build &b, int lo, int hi, int d, double *sum) {
#pragma clang fp contract(off)
        const Model &m = b.m;
        const size_t MD = b.MD, D = b.D;
        std::vector<double> mine(D, 0.0);
        double cover = 0.0;
        if (hi - lo == 1) {
            if (leaf_depth(b, lo) != d) { b.ok = false; return 0.0; }
            cover = 1.0;
            for (int k = 0; k < d; ++k) cover *= static_cast<double>(m.edge_weights[static_cast<size_t>(lo) * MD + k]);
            double *e = &b.E[(static_cast<size_t>(lo - b.l0) * (MD + 1) + d) * D];
            for (size_t j = 0; j < D; ++j) {
                e[j] = static_cast<double>(m.values[static_cast<size_t>(lo) * D + j]);
                sum[j] += cover * e[j];
            }
            return cover;
        }
        if (d >= b.MD) { b.ok = false; return 0.0; }
        int mid = lo;
        if (m.oblivious()) mid = lo + (hi - lo) / 2;
        else
            for (int q = lo; q < hi; ++q) {   // left leaves first, contiguous (GreedyNodes::build has the same test)
                if (leaf_depth(b, q) <= d) { b.ok = false; return 0.0; }
                if (m.inequality_directions[static_cast<size_t>(q) * MD + d] == 0) { if (q != mid) { b.ok = false; return 0.0; } ++mid; }
            }
        if (mid == lo || mid == hi) { b.ok = false; return 0.0; }
        cover = walk(b, lo, mid, d + 1, mine.data());
        cover += walk(b, mid, hi, d + 1, mine.data());
        if (!b.ok) return 0.0;
        for (size_t j = 0; j < D; ++j) {
            sum[j] += mine[j];
            mine[j] = cover > 0.0 ? mine[j] / cover : 0.0;
        }
        for (int l = lo; l < hi; ++l) std::copy(mine.begin(), mine.end(), &b.E[(static_cast<size_t>(l - b.l0) * (MD + 1) + d) * D]);
        return cover;
    }

    bool put_tree(const Model &m, int t) {
#pragma clang fp contract(off)
        const size_t MD = m.meta.max_depth, D = m.meta.output_dim;
        const int l0 = static_cast<int>(m.first_leaf(t)), nl = static_cast<int>(m.leaf_count(t));
        std::fill(delta.begin() + static_cast<long>(static_cast<size_t>(l0) * MD * D), delta.begin() + static_cast<long>(static_cast<size_t>(l0 + nl) * MD * D), 0.0f);
        std::fill(root.begin() + static_cast<long>(t * D), root.begin() + static_cast<long>((t + 1) * D), 0.0);
        if (nl < 1 || (nl == 1 && !m.oblivious())) return false;
        Build b{m, t, l0, static_cast<int>(MD), static_cast<int>(D), std::vector<double>(static_cast<size_t>(nl) * (MD + 1) * D, 0.0)};
        std::vector<double> sum(D, 0.0);
        walk(b, l0, l0 + nl, 0, sum.data());
        if (!b.ok) return false;
        for (size_t d = 0; d < D; ++d) {
            const double lr = rate(m, t, static_cast<int>(d));
            root[static_cast<size_t>(t) * D + d] = -lr * b.E[d];
            for (int l = 0; l < nl; ++l) {
                const int depth = leaf_depth(b, l0 + l);
                const double *e = &b.E[static_cast<size_t>(l) * (MD + 1) * D + d];
                for (int j = 0; j < depth; ++j) delta[(static_cast<size_t>(l0 + l) * MD + j) * D + d] = static_cast<float>(-lr * (e[(j + 1) * D] - e[j * D]));
            }
        }
        return true;
    }
};

// the split row that holds the conditions of (tree t, leaf l): the tree's when oblivious, the leaf's when greedy
inline size_t path_cond_row(const Model &m, int t, int leaf) { return m.oblivious() ? static_cast<size_t>(t) : static_cast<size_t>(leaf); }

// the features the trees [0, n_trees) test, ascending: slot s of the streaming kernel is used[s]
inline std::vector<int32_t> path_used(const Model &m, int n_trees, int F) {
    std::vector<uint8_t> seen(static_cast<size_t>(std::max(F, 0)), 0);
    const size_t MD = m.meta.max_depth;
    const size_t rows = m.oblivious() ? static_cast<size_t>(n_trees)
                                      : (n_trees < m.meta.n_trees ? static_cast<size_t>(m.tree_indices[n_trees]) : static_cast<size_t>(m.meta.n_leaves));
    for (size_t s = 0; s < rows; ++s)
        for (int d = 0; d < m.depths[s]; ++d) {
            const int f = m.feature_indices[s * MD + d];
            if (f >= 0 && f < F) seen[f] = 1;
        }
    std::vector<int32_t> used;
    for (int f = 0; f < F; ++f)
        if (seen[f]) used.push_back(f);
    return used;
}

// ------------------------------------------------------------------------------------------------------------ the launch plans
// LDS of a block of the streaming kernel: the code tile [64][(G * 8) | 1] words, then acc[slot][64][D | 1] float32 -- the stride of a row is odd, so the
// D adds of the 64 lanes (lane = row) meet 64 different banks
inline size_t path_code_tile_bytes(int G) { return static_cast<size_t>(kPathRows) * ((static_cast<size_t>(G) * 8) | 1) * sizeof(uint32_t); }
GBRL_PATH_HD inline int path_row_stride(int D) { return D | 1; }
inline size_t path_slot_bytes(int D) { return static_cast<size_t>(kPathRows) * path_row_stride(D) * sizeof(float); }

struct PathSlotPlan {
    bool fits;        // the code tile and at least one slot fit the budget (and D <= 64); false: the general kernel
    int slots;        // slots per pass
    int passes;       // walks of the trees over a staged tile: ceil(n_used / slots); 0 without a used feature
    size_t lds;       // dynamic LDS of a block
};
inline PathSlotPlan path_slot_plan(int n_used, int G, int D, size_t budget = kStreamLdsBudget) {
    PathSlotPlan p{false, 0, 0, 0};
    const size_t tile = path_code_tile_bytes(G), slot = path_slot_bytes(D);
    if (D < 1 || D > 64 || tile + slot > budget) return p;
    p.fits = true;
    p.slots = static_cast<int>(std::min<size_t>((budget - tile) / slot, static_cast<size_t>(std::max(n_used, 1))));
    p.passes = n_used <= 0 ? 0 : (n_used + p.slots - 1) / p.slots;
    p.lds = tile + static_cast<size_t>(p.slots) * slot;
    return p;
}

// tiles per launch: `tile_bytes` of scratch per tile (streaming importance: its 2 * n_used * D float64 partials; general importance: its 64 rows
// of the float32 matrix) within the budget, and at least one
inline int path_launch_tiles(size_t tile_bytes, size_t budget = kPathScratchBudget) {
    return static_cast<int>(std::min<size_t>(std::max<size_t>(budget / std::max<size_t>(tile_bytes, 1), 1), size_t(1) << 24));
}
inline int path_tiles(long long m) { return static_cast<int>((m + kPathRows - 1) / kPathRows); }

// ---- the argument checks that need no device: an empty string, or the refusal's text behind "<call>: "
inline std::string path_trees_error(int n_trees, int T) {
    if (T == 0) return "the model has no trees";
    if (n_trees != -1 && (n_trees < 1 || n_trees > T))
        return "n_trees " + std::to_string(n_trees) + " is outside [1, " + std::to_string(T) + "], the model's trees (None / -1: all)";
    return std::string();
}
inline std::string path_matrix_error(long long m, int F, int D) {
    if (static_cast<unsigned long long>(m) * static_cast<unsigned long long>(F) * static_cast<unsigned long long>(D) >= (1ull << 31))
        return "the matrix of " + std::to_string(m) + " rows x " + std::to_string(F) + " features x " + std::to_string(D) +
               " outputs has 2^31 elements or more: pass rows= to explain fewer rows, or use path_importance_prepared";
    return std::string();
}
inline std::string path_model_error(const Model &m, const PathTable &table, int n_trees) {
    if (m.meta.n_cat_features > 0) return "not available on a model with categorical columns";
    if (table.bad_tree >= 0 && table.bad_tree < n_trees)
        return "tree " + std::to_string(table.bad_tree) + " is not a proper binary tree with a split (a greedy tree of one leaf, or leaves out of depth-first order): its paths have no attribution";
    return std::string();
}

}  // namespace kern
}  // namespace gbrl
