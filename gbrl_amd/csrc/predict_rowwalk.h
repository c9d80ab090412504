// predict_rowwalk.h -- the one row walk behind predict_continue.hip, predict_continue_codes.hip, predict_staged.hip, predict_leaves.hip and refit.hip.  All route a
// row to the same leaf and, where they apply values, run the same chain p = fma(-rate(t, optimizer of the output), value(leaf), p), because
// every piece of that exists once, here:
//   model views    LeavesModel (routing: leaves_model) and ChainModel (routing + values, rates, bias: chain_model); the rate rule is chain_rates
//   row accessors  how a walk reads a numeric condition of its row: floats against the threshold (GeneralRow, a float tile row) or a prepared
//                  data set's bin codes against the condition's bin (GeneralCodeRow, StreamCodeRow; x > v <=> code > bin, engine_codes.hip).
//                  Every walk below takes the row as a template parameter; the staging of a code tile is stream_stage_code_tile / _groups
//   general side   one thread per row, rows in global memory, anything the file format can hold: general_test, general_leaf (the reference's
//                  walk; greedy: leaf by leaf, Q7), general_apply (every optimizer that owns the output, in order) and general_chain_tree
//                  (one tree of the chain: k_continue_general's loop body, and k_staged_general's between two checkpoints)
//   streaming side lane = row, one wave per block, the block's 64 rows in LDS at stride F | 1, the outputs of a row in registers:
//                  stream_stage_tile, stream_load_row / stream_store_row, stream_leaf (conditions through wave-uniform addresses), and
//                  stream_chain_group with kStreamGroup and StreamOwner (a group of trees walked, gathered, then applied in tree order)
//   host side      which family takes a model (leaves_streamable, chain_streamable), the LDS budget and its per-device opt-in
//                  (kStreamLdsBudget, stream_tile_bytes, StreamLdsOptIn), stream_cu_count, and the template-width ladders
//                  (with_stream_dmax, with_general_dmax)
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"

namespace gbrl {
namespace kern {
namespace {

// ------------------------------------------------------------------------------------------------------------ model views
struct LeavesModel {
    const int32_t *tree_indices, *depths, *feature_indices, *cat_ids, *cond_pack, *grd_nodes, *grd_node_off;
    const float *feature_values;
    const uint8_t *is_numerics, *inequality_directions;
    int n_leaves, max_depth, oblivious;
    const int32_t *feature_bins;   // code walks only: the bin of every numeric condition, indexed like feature_values (null otherwise)
};

// rate(t, o) = rate[t * rate_stride + o]: PredictModel::rate (stride n_opts) for an ensemble with a Linear schedule (absolute tree index),
// opt_lr (stride 0: one rate per optimizer) otherwise
struct ChainRates {
    const int32_t *opt_start, *opt_stop;
    const float *rate;
    int n_opts, rate_stride;
};

// the routing view and what the chain kernels (continue, staged) need beside it; one struct, so that a kernel takes one model argument
struct ChainModel {
    const float *values, *bias;
    ChainRates rates;
    int D;
    LeavesModel walk;
};

inline LeavesModel leaves_model(const PredictModel &pm) {
    LeavesModel cm{};
    cm.tree_indices = pm.tree_indices; cm.depths = pm.depths; cm.feature_indices = pm.feature_indices; cm.cat_ids = pm.cat_ids;
    cm.cond_pack = pm.cond_pack; cm.grd_nodes = pm.grd_nodes; cm.grd_node_off = pm.grd_node_off;
    cm.feature_values = pm.feature_values;
    cm.is_numerics = pm.is_numerics; cm.inequality_directions = pm.inequality_directions;
    cm.n_leaves = pm.n_leaves; cm.max_depth = pm.max_depth; cm.oblivious = pm.oblivious;
    return cm;
}
inline ChainRates chain_rates(const PredictModel &pm) {
    return ChainRates{pm.opt_start, pm.opt_stop, pm.rate != nullptr ? pm.rate : pm.opt_lr, pm.n_opts, pm.rate != nullptr ? pm.n_opts : 0};
}
inline ChainModel chain_model(const PredictModel &pm) { return ChainModel{pm.values, pm.bias, chain_rates(pm), pm.D, leaves_model(pm)}; }

// ------------------------------------------------------------------------------------------------------------ general side
// global leaf of (row, tree t), -1 when a greedy search runs off the ensemble
struct GeneralRow {
    const float *x;
    const int32_t *xc;
    __device__ __forceinline__ bool numeric(const LeavesModel &cm, int f, int c) const { return x[f] > cm.feature_values[c]; }
    __device__ __forceinline__ bool categorical(const LeavesModel &cm, int f, int c) const { return xc != nullptr && xc[f] == cm.cat_ids[c]; }
};
// a row of a prepared data set: its 32-byte code records, one per group of 16 features, `group_stride` u16 apart ([G][N][16]); numeric-only
struct GeneralCodeRow {
    const uint16_t *rec;
    size_t group_stride;
    __device__ __forceinline__ bool numeric(const LeavesModel &cm, int f, int c) const {
        return static_cast<int>(rec[static_cast<size_t>(f >> 4) * group_stride + (f & 15)]) > cm.feature_bins[c];
    }
    __device__ __forceinline__ bool categorical(const LeavesModel &, int, int) const { return false; }
};
template <typename Row>
__device__ __forceinline__ bool general_test(const LeavesModel &cm, const Row &r, int c) {
    const int f = cm.feature_indices[c];
    return cm.is_numerics[c] ? r.numeric(cm, f, c) : r.categorical(cm, f, c);
}
template <typename Row>
__device__ __forceinline__ int general_leaf(const LeavesModel &cm, const Row &r, int t) {
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

// tree t's step of the chain on the outputs p of one row: every optimizer that owns output j, in order
template <int DMAX>
__device__ __forceinline__ void general_apply(const ChainModel &cm, int t, int leaf, float (&p)[DMAX]) {
    const int D = cm.D;
    const float *v = cm.values + static_cast<size_t>(leaf) * D;
    for (int o = 0; o < cm.rates.n_opts; ++o) {
        const float lr = cm.rates.rate[static_cast<size_t>(t) * cm.rates.rate_stride + o];
        const int a = cm.rates.opt_start[o], b = cm.rates.opt_stop[o];
#pragma unroll
        for (int j = 0; j < DMAX; ++j)
            if (j >= a && j < b && j < D) p[j] = __fmaf_rn(-lr, v[j], p[j]);
    }
}

// The reference walks a greedy ensemble leaf by leaf in storage order with a tree counter beside it: a leaf that passes is applied at the
// counter's rate, the counter moves on and the search restarts at tree_indices[t + 1]; a search that passes the last leaf ends the walk.  So
// per tree it finds general_leaf(t) -- a later tree's leaf when none of tree t's passes (a depth-0 leaf never does, Q7), still applied at
// tree t's rate -- and -1 ends the walk for good.  Returns false then; a caller that suspends the walk at a checkpoint must not resume it.
template <int DMAX, typename Row>
__device__ __forceinline__ bool general_chain_tree(const ChainModel &cm, const Row &r, int t, float (&p)[DMAX]) {
    const int leaf = general_leaf(cm.walk, r, t);
    if (leaf < 0) return false;
    general_apply<DMAX>(cm, t, leaf, p);
    return true;
}

// ------------------------------------------------------------------------------------------------------------ streaming side
constexpr int kStreamRows = 64;   // rows per block = one wave

// D floats of one row into registers: 16-byte accesses when the row is a whole number of them and its address allows it
template <int DMAX>
__device__ __forceinline__ void stream_load_row(const float *src, int D, bool vec4, float (&v)[DMAX]) {
    if (vec4) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q) {
            const float4 w = 4 * q < D ? s4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < DMAX; ++j) v[j] = j < D ? src[j] : 0.0f;
    }
}
// ... and back
template <int DMAX>
__device__ __forceinline__ void stream_store_row(float *dst, int D, bool vec4, const float (&p)[DMAX]) {
    if (vec4) {
        float4 *d4 = reinterpret_cast<float4 *>(dst);
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q)
            if (4 * q < D) d4[q] = make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < DMAX; ++j)
            if (j < D) dst[j] = p[j];
    }
}

// coalesced staging of a block's `rows` rows from r0 on (contiguous in the row-major matrix) into tile[kStreamRows][F | 1], 16 x 16 bytes in flight
// per lane; the caller synchronises the block afterwards
__device__ __forceinline__ void stream_stage_tile(float *tile, const float *__restrict__ obs, int F, int r0, int rows, int lane) {
    const int xs = F | 1;
    const float *src = obs + static_cast<size_t>(r0) * F;
    if (F > 0 && (F & 3) == 0 && (reinterpret_cast<uintptr_t>(obs) & 15) == 0) {
        const float4 *src4 = reinterpret_cast<const float4 *>(src);
        const int F4 = F >> 2, tot4 = rows * F4;
        constexpr int UL = 16;
        for (int i0 = lane; i0 < tot4; i0 += kStreamRows * UL) {
            float4 v[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * kStreamRows;
                v[u] = i < tot4 ? src4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * kStreamRows;
                if (i < tot4) {
                    const int r = i / F4, f = (i - r * F4) << 2;
                    float *dst = tile + r * xs + f;
                    dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
                }
            }
        }
    } else {
        const int tot = rows * F;
        for (int i = lane; i < tot; i += kStreamRows) {
            const int r = i / F, f = i - r * F;
            tile[r * xs + f] = src[i];
        }
    }
}

// A block's rows of a prepared data set into a code tile: tile[kStreamRows][stream_code_stride(G)] 4-byte words, a row = its G records of 16 u16
// codes back to back.  The stride is odd, so a wave that reads one feature of its 64 rows (a 2-byte read: banks are per word, modulo 32 within
// each half of the wave) never meets a bank twice.  The records are group-major in memory, [G][N][16]: lane `lane` names the data set row of
// tile row `lane` (my_row; any valid row for a lane without one), and the G * 128 half-records travel as 16-byte loads, two lanes per record,
// 16 in flight per lane.  The caller synchronises the block afterwards.
// stream_stage_code_groups is the same staging for a LIST of groups: tile group i holds the records of data set group group_of(i) (gather_cols.hip
// stages only the groups that hold a selected column).
__device__ __forceinline__ int stream_code_stride(int G) { return (G * 8) | 1; }
template <typename GroupOf>
__device__ __forceinline__ void stream_stage_code_groups(uint32_t *tile, const uint16_t *__restrict__ codes, size_t N, int G, GroupOf group_of, int my_row, int rows,
                                                         int lane) {
    const int ws = stream_code_stride(G);
    const uint4 *src4 = reinterpret_cast<const uint4 *>(codes);
    const int tot = G * 2 * kStreamRows;   // half-records of the block: [group][tile row][half]
    constexpr int UL = 16;
    for (int i0 = lane; i0 < tot; i0 += kStreamRows * UL) {
        uint4 v[UL];
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int i = i0 + u * kStreamRows;
            const int j = (i & (2 * kStreamRows - 1)) >> 1;
            const int src_row = __shfl(my_row, j);   // (every lane takes part: i0 < tot is wave-uniform, tot is a multiple of 64)
            v[u] = (i < tot && j < rows) ? src4[((static_cast<size_t>(group_of(i >> 7)) * N + static_cast<size_t>(src_row)) << 1) + (i & 1)] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int i = i0 + u * kStreamRows;
            if (i < tot) {
                const int j = (i & (2 * kStreamRows - 1)) >> 1;
                uint32_t *dst = tile + j * ws + (i >> 7) * 8 + (i & 1) * 4;
                dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
            }
        }
    }
}
__device__ __forceinline__ void stream_stage_code_tile(uint32_t *tile, const uint16_t *__restrict__ codes, size_t N, int G, int my_row, int rows, int lane) {
    stream_stage_code_groups(tile, codes, N, G, [](int g) { return g; }, my_row, rows, lane);
}

// the lane's row in the LDS tile: floats against a condition's threshold bits, or the u16 codes of a code tile against its bin
__device__ __forceinline__ bool stream_numeric(const float *x, int f, int tv) { return x[f] > __int_as_float(tv); }
struct StreamCodeRow { const uint16_t *c; };
__device__ __forceinline__ bool stream_numeric(const StreamCodeRow &x, int f, int bin) { return static_cast<int>(x.c[f]) > bin; }

// the walk of tree t (wave-uniform t); x is the lane's row in the LDS tile
template <bool GREEDY, typename Row>
__device__ __forceinline__ int stream_leaf(const LeavesModel &cm, const Row &x, const int32_t *xc, int t) {
    // feature word >= 0: numeric feature against a threshold (a code row: against a bin); < 0: ~categorical feature against a dictionary id
    auto pass = [&](int fi, int tv) -> bool { return fi >= 0 ? stream_numeric(x, fi, tv) : (xc != nullptr && xc[~fi] == tv); };
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

template <int DMAX>
constexpr int kStreamGroup = DMAX <= 4 ? 8 : DMAX <= 8 ? 4 : DMAX <= 16 ? 2 : 1;   // trees whose leaf values are in flight together

template <int DMAX>
struct StreamOwner { uint8_t opt[DMAX]; };   // optimizer that owns output j (meaningful where bit j of PredictModel::coef_cover is set)
template <int DMAX>
StreamOwner<DMAX> stream_owner(const PredictModel &pm) {
    StreamOwner<DMAX> own;
    for (int j = 0; j < DMAX; ++j) own.opt[j] = j < pm.D ? pm.owner[j] : 0;
    return own;
}

// the trees [t0, min(t0 + kStreamGroup, t_end)) (wave-uniform) on the outputs p of the lane's row: all walked, then the values of all their
// leaves gathered, then applied tree by tree.  An output outside `cover` is skipped, not multiplied by a zero rate.
template <int DMAX, bool GREEDY, typename Row>
__device__ __forceinline__ void stream_chain_group(const ChainModel &cm, const StreamOwner<DMAX> &own, uint64_t cover, const Row &x,
                                                   const int32_t *xc, int t0, int t_end, int vec_values, float (&p)[DMAX]) {
    constexpr int kG = kStreamGroup<DMAX>;
    const int D = cm.D;
    int leaf[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) leaf[g] = t0 + g < t_end ? stream_leaf<GREEDY>(cm.walk, x, xc, t0 + g) : 0;
    float v[kG][DMAX];
#pragma unroll
    for (int g = 0; g < kG; ++g)
        if (t0 + g < t_end) stream_load_row<DMAX>(cm.values + static_cast<size_t>(leaf[g]) * D, D, vec_values != 0, v[g]);
#pragma unroll
    for (int g = 0; g < kG; ++g) {
        const int t = t0 + g;
        if (t < t_end) {
            const float *rt = cm.rates.rate + static_cast<size_t>(t) * cm.rates.rate_stride;
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D && ((cover >> j) & 1ull)) p[j] = __fmaf_rn(-rt[own.opt[j]], v[g][j], p[j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
// the streaming family: the packed conditions / rebuilt node records (no depth-0 greedy tree then), at least one level ...
inline bool leaves_streamable(const PredictModel &pm, bool generic) {
    return !generic && pm.max_depth >= 1 &&
           (pm.oblivious ? pm.cond_pack != nullptr : (pm.grd_ok && pm.grd_nodes != nullptr && pm.grd_node_off != nullptr));
}
// ... and for a chain: every output owned by at most one optimizer (owner[] and coef_cover are valid), a row's outputs in registers
inline bool chain_streamable(const PredictModel &pm, bool generic) { return leaves_streamable(pm, generic) && pm.coef_ok && pm.D <= 64; }

// (kStreamLdsBudget, the dynamic LDS the streaming kernels opt in to, is leaf_accum.h's: its launch plan is tested without a device)
inline size_t stream_tile_bytes(int F) { return static_cast<size_t>(kStreamRows) * (F | 1) * sizeof(float); }
inline size_t stream_code_tile_bytes(int G) { return static_cast<size_t>(kStreamRows) * ((G * 8) | 1) * sizeof(uint32_t); }

// Dynamic LDS above the default 64 KiB needs an opt-in per kernel and device; one of these per kernel (a function-local static).
// ok(): false when this device refused the opt-in and `lds` needs it -- the caller takes its general kernel.
struct StreamLdsOptIn {
    PerDeviceOnce asked;
    std::atomic<uint64_t> refused{0};
    template <typename K>
    bool ok(K kernel, size_t lds) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0;
        if (asked.first() && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(kStreamLdsBudget)) != hipSuccess) {
            (void)hipGetLastError();
            refused.fetch_or(bit, std::memory_order_relaxed);
        }
        return !((refused.load(std::memory_order_relaxed) & bit) && lds > 64 * 1024);
    }
};

inline int stream_cu_count() {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    return c;
}

// f(std::integral_constant<int, DMAX>) at the narrowest template width that holds D outputs: the streaming kernels (D <= 64) ...
template <typename Fn>
auto with_stream_dmax(int D, Fn &&f) {
    if (D <= 4) return f(std::integral_constant<int, 4>{});
    if (D <= 8) return f(std::integral_constant<int, 8>{});
    if (D <= 16) return f(std::integral_constant<int, 16>{});
    if (D <= 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}
// ... and the general chain kernels (D <= 128)
template <typename Fn>
auto with_general_dmax(int D, Fn &&f) {
    if (D <= 8) return f(std::integral_constant<int, 8>{});
    if (D <= 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 128>{});
}

}  // namespace
}  // namespace kern
}  // namespace gbrl
