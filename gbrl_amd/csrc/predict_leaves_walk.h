// predict_leaves_walk.h -- the leaf routing of predict_leaves.hip, shared with refit.hip so that a refit sums the gradients of exactly the rows
// predict_leaves reports for a leaf: the model view, the general walk (one thread per row, rows in global memory) and the streaming walk
// (k_continue's: the lane's row in an LDS tile, wave-uniform condition reads), and the host-side choice between the two families.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "kernels_common.h"

namespace gbrl {
namespace kern {
namespace {

struct LeavesModel {
    const int32_t *tree_indices, *depths, *feature_indices, *cat_ids, *cond_pack, *grd_nodes, *grd_node_off;
    const float *feature_values;
    const uint8_t *is_numerics, *inequality_directions;
    int n_leaves, max_depth, oblivious;
};

constexpr size_t kLeavesLdsBudget = 156 * 1024;    // the opt-in the streaming kernels of this library ask for

// ------------------------------------------------------------------------------------------------------------ the walks
// general: global leaf of (row, tree t), -1 when a greedy search runs off the ensemble
struct GeneralRow {
    const float *x;
    const int32_t *xc;
};
__device__ __forceinline__ bool general_test(const LeavesModel &cm, const GeneralRow &r, int c) {
    const int f = cm.feature_indices[c];
    return cm.is_numerics[c] ? (r.x[f] > cm.feature_values[c]) : (r.xc != nullptr && r.xc[f] == cm.cat_ids[c]);
}
__device__ __forceinline__ int general_leaf(const LeavesModel &cm, const GeneralRow &r, int t) {
    const int md = cm.max_depth;
    if (cm.oblivious) {
        const int depth = cm.depths[t], cond = t * md;
        int l = 0;
        for (int d = 0; d < depth; ++d) l |= (general_test(cm, r, cond + d) ? 1 : 0) << (depth - 1 - d);
        return cm.tree_indices[t] + l;
    }
    for (int leaf = cm.tree_indices[t]; leaf < cm.n_leaves; ++leaf) {
        const int depth = cm.depths[leaf], cond = leaf * md;
        bool passed = false;
        for (int d = depth - 1; d >= 0; --d) {
            passed = (general_test(cm, r, cond + d) == (cm.inequality_directions[cond + d] != 0));
            if (!passed) break;
        }
        if (passed) return leaf;
    }
    return -1;
}

// streaming: k_continue's walk of tree t (wave-uniform t); x is the lane's row in the LDS tile
template <bool GREEDY>
__device__ __forceinline__ int stream_leaf(const LeavesModel &cm, const float *x, const int32_t *xc, int t) {
    // feature word >= 0: numeric feature against a threshold; < 0: ~categorical feature against a dictionary id
    auto pass = [&](int fi, int tv) -> bool { return fi >= 0 ? (x[fi] > __int_as_float(tv)) : (xc != nullptr && xc[~fi] == tv); };
    const int md = cm.max_depth;
    if (!GREEDY) {
        const int depth = cm.depths[t];
        const int32_t *cp = cm.cond_pack + static_cast<size_t>(t) * 2 * md;
        int l = 0;
        for (int d = 0; d < depth; ++d) l |= pass(cp[2 * d], cp[2 * d + 1]) ? (1 << (depth - 1 - d)) : 0;
        return cm.tree_indices[t] + l;
    } else {
        // descent of the rebuilt binary tree: a child >= 0 is a node of the tree, < 0 is ~(leaf within the tree); a leaf lies at most
        // max_depth steps below the root
        const int4 *nodes = reinterpret_cast<const int4 *>(cm.grd_nodes) + cm.grd_node_off[t];
        int node = 0;
        for (int d = 0; d < md && node >= 0; ++d) {
            const int4 nd = nodes[node];
            node = pass(nd.x, nd.y) ? nd.w : nd.z;
        }
        return cm.tree_indices[t] + (node < 0 ? ~node : 0);
    }
}

LeavesModel leaves_model(const PredictModel &pm) {
    LeavesModel cm{};
    cm.tree_indices = pm.tree_indices; cm.depths = pm.depths; cm.feature_indices = pm.feature_indices; cm.cat_ids = pm.cat_ids;
    cm.cond_pack = pm.cond_pack; cm.grd_nodes = pm.grd_nodes; cm.grd_node_off = pm.grd_node_off;
    cm.feature_values = pm.feature_values;
    cm.is_numerics = pm.is_numerics; cm.inequality_directions = pm.inequality_directions;
    cm.n_leaves = pm.n_leaves; cm.max_depth = pm.max_depth; cm.oblivious = pm.oblivious;
    return cm;
}

// the streaming family: the packed conditions / rebuilt node records (no depth-0 greedy tree then), at least one level
bool leaves_streamable(const PredictModel &pm, bool generic) {
    return !generic && pm.max_depth >= 1 &&
           (pm.oblivious ? pm.cond_pack != nullptr : (pm.grd_ok && pm.grd_nodes != nullptr && pm.grd_node_off != nullptr));
}

// dynamic LDS above the default 64 KiB needs an opt-in per kernel and device; false: this device refuses it and `lds` needs it
template <typename K>
bool leaves_lds_ok(K kernel, PerDeviceOnce &attr, uint64_t &unsupported, size_t lds) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0;
    if (attr.first() && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLeavesLdsBudget)) != hipSuccess) {
        (void)hipGetLastError();
        unsupported |= bit;
    }
    return !((unsupported & bit) && lds > 64 * 1024);
}

int leaves_cu_count() {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    return c;
}

}  // namespace
}  // namespace kern
}  // namespace gbrl
