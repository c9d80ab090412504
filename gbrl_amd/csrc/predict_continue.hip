// predict_continue.hip -- gfx950 kernels behind GBRL::predict_continue: a prediction the caller already holds over the trees [0, start) is
// carried through the trees [start, stop).  Per (row, output) that is the continuation of ONE chain in tree order,
// p = fma(-rate(t, optimizer of the output), value(leaf(row, t)), p) (optimizer.cpp:110-118), started from base[row][output] instead of the
// bias: the bits of a walk over [0, stop).  The range is never split over blocks and no partial sums are combined, at any batch size
// or range length -- that is the call's contract, and why it is not a variant of kern::predict's dispatcher.
//
//   k_continue          lane = row, one wave per block.  The block's 64 rows sit in LDS at stride F | 1 (a wave that reads one feature of
//                       its 64 rows touches 64 banks), the outputs of a row in registers, loaded from `base` before the tile is staged so
//                       that both streams are in flight together.  The trees of the range are taken in groups of kG: a tree's condition
//                       words (oblivious: cond_pack) or its root (greedy: the rebuilt node records) and the rate of (tree, output) have
//                       wave-uniform addresses and come through the scalar cache; the leaf's values are gathered per lane from the
//                       ensemble (a few KiB per tree: L2) for the whole group before they are applied tree by tree.  The case that
//                       matters is 1 to a few dozen trees over 2^12 .. 2^20 rows, where the kernel moves n (4 F + 8 D) bytes and little else;
//                       independent one-wave blocks let the staging of one tile overlap the walk and the stores of its neighbours on the CU.
//                       Every output owned by at most one optimizer, D <= 64.  Outputs that no optimizer owns keep their base bits
//                       (they are skipped, not multiplied by a zero rate: fma(-0, v, -0.0f) is not always -0.0f).
//   k_continue_general  anything the file format can hold: one thread per row, the reference's walk (greedy: leaf by leaf, Q7), optimizers
//                       that share outputs, D <= 128, rows too wide for an LDS tile.  Also the cross-check behind GBRL_HIP_CONTINUE_GENERIC=1.
//
// rate(t, o): PredictModel::rate[t * n_opts + o] for an ensemble with a Linear schedule (absolute tree index), opt_lr[o] otherwise.
// `base` and `out` may be the same buffer: a thread reads and writes its own row only.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_stream_common.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

struct ContModel {
    const int32_t *tree_indices, *depths, *feature_indices, *cat_ids, *cond_pack, *grd_nodes, *grd_node_off, *opt_start, *opt_stop;
    const float *feature_values, *values, *rate;
    const uint8_t *is_numerics, *inequality_directions;
    int n_leaves, max_depth, D, oblivious, n_opts, rate_stride;   // rate_stride: n_opts (rate table) or 0 (one rate per optimizer)
};

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX>
__global__ __launch_bounds__(256) void k_continue_general(ContModel cm, const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes,
                                                          int Fc, int n, int start_tree, int stop_tree, const float *base, float *out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const int D = cm.D, md = cm.max_depth;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? base[static_cast<size_t>(row) * D + j] : 0.0f;
    const float *x = obs + static_cast<size_t>(row) * F;
    const int32_t *xc = cat_codes ? cat_codes + static_cast<size_t>(row) * Fc : nullptr;
    auto test = [&](int c) -> bool {
        const int f = cm.feature_indices[c];
        return cm.is_numerics[c] ? (x[f] > cm.feature_values[c]) : (xc != nullptr && xc[f] == cm.cat_ids[c]);
    };
    auto apply = [&](int t, const float *v) {
        for (int o = 0; o < cm.n_opts; ++o) {
            const float lr = cm.rate[static_cast<size_t>(t) * cm.rate_stride + o];
            const int a = cm.opt_start[o], b = cm.opt_stop[o];
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j >= a && j < b && j < D) p[j] = __fmaf_rn(-lr, v[j], p[j]);
        }
    };
    if (cm.oblivious) {
        for (int t = start_tree; t < stop_tree; ++t) {
            const int depth = cm.depths[t], cond = t * md;
            int leaf = 0;
            for (int d = 0; d < depth; ++d) leaf |= (test(cond + d) ? 1 : 0) << (depth - 1 - d);
            apply(t, cm.values + static_cast<size_t>(cm.tree_indices[t] + leaf) * D);
        }
    } else {
        int t = start_tree;
        int leaf = cm.tree_indices[t];
        while (leaf < cm.n_leaves && t < stop_tree) {
            const int depth = cm.depths[leaf], cond = leaf * md;
            bool passed = false;
            for (int d = depth - 1; d >= 0; --d) {
                passed = (test(cond + d) == (cm.inequality_directions[cond + d] != 0));
                if (!passed) break;
            }
            if (passed) {
                apply(t, cm.values + static_cast<size_t>(leaf) * D);
                ++t;
                if (t < stop_tree) leaf = cm.tree_indices[t];
            } else {
                ++leaf;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < D) out[static_cast<size_t>(row) * D + j] = p[j];
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
constexpr int kContRows = kStreamRows;   // rows per block = one wave

template <int DMAX>
struct ContOwner { uint8_t opt[DMAX]; };   // optimizer that owns output j (meaningful where bit j of `cover` is set)

template <int DMAX, bool GREEDY>
__global__ __launch_bounds__(kContRows) void k_continue(ContModel cm, ContOwner<DMAX> own, uint64_t cover, const float *__restrict__ obs, int F,
                                                        const int32_t *__restrict__ cat_codes, int Fc, int n, int start_tree, int stop_tree,
                                                        const float *base, float *out, int vec_values, int vec_io) {
    extern __shared__ float ctile[];   // [kContRows][F | 1]
    constexpr int kG = DMAX <= 4 ? 8 : DMAX <= 8 ? 4 : DMAX <= 16 ? 2 : 1;   // trees whose leaf values are in flight together
    const int lane = threadIdx.x;
    const int xs = F | 1;
    const int D = cm.D, md = cm.max_depth;
    const int r0 = blockIdx.x * kContRows;
    const int rows = min(kContRows, n - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    float p[DMAX];
    if (live) {
        stream_load_row<DMAX>(base + row * D, D, vec_io != 0, p);
    } else {
#pragma unroll
        for (int j = 0; j < DMAX; ++j) p[j] = 0.0f;
    }
    stream_stage_tile(ctile, obs, F, r0, rows, lane);
    __syncthreads();
    if (live) {
        const float *x = ctile + lane * xs;
        const int32_t *xc = cat_codes ? cat_codes + row * Fc : nullptr;
        // feature word >= 0: numeric feature against a threshold; < 0: ~categorical feature against a dictionary id
        auto pass = [&](int fi, int tv) -> bool { return fi >= 0 ? (x[fi] > __int_as_float(tv)) : (xc != nullptr && xc[~fi] == tv); };
        for (int t0 = start_tree; t0 < stop_tree; t0 += kG) {
            int leaf[kG];
#pragma unroll
            for (int g = 0; g < kG; ++g) {
                const int t = t0 + g;
                leaf[g] = 0;
                if (t < stop_tree) {   // (wave-uniform)
                    if (!GREEDY) {
                        const int depth = cm.depths[t];
                        const int32_t *cp = cm.cond_pack + static_cast<size_t>(t) * 2 * md;
                        int l = 0;
                        for (int d = 0; d < depth; ++d) l |= pass(cp[2 * d], cp[2 * d + 1]) ? (1 << (depth - 1 - d)) : 0;
                        leaf[g] = cm.tree_indices[t] + l;
                    } else {
                        // descent of the rebuilt binary tree: a child >= 0 is a node of the tree, < 0 is ~(leaf within the tree); a leaf lies
                        // at most max_depth steps below the root
                        const int4 *nodes = reinterpret_cast<const int4 *>(cm.grd_nodes) + cm.grd_node_off[t];
                        int node = 0;
                        for (int d = 0; d < md && node >= 0; ++d) {
                            const int4 nd = nodes[node];
                            node = pass(nd.x, nd.y) ? nd.w : nd.z;
                        }
                        leaf[g] = cm.tree_indices[t] + (node < 0 ? ~node : 0);
                    }
                }
            }
            float v[kG][DMAX];
#pragma unroll
            for (int g = 0; g < kG; ++g)
                if (t0 + g < stop_tree) stream_load_row<DMAX>(cm.values + static_cast<size_t>(leaf[g]) * D, D, vec_values != 0, v[g]);
#pragma unroll
            for (int g = 0; g < kG; ++g) {
                const int t = t0 + g;
                if (t < stop_tree) {
                    const float *rt = cm.rate + static_cast<size_t>(t) * cm.rate_stride;
#pragma unroll
                    for (int j = 0; j < DMAX; ++j)
                        if (j < D && ((cover >> j) & 1ull)) p[j] = __fmaf_rn(-rt[own.opt[j]], v[g][j], p[j]);
                }
            }
        }
        float *o = out + row * D;
        if (vec_io) {
            float4 *o4 = reinterpret_cast<float4 *>(o);
#pragma unroll
            for (int q = 0; q < DMAX / 4; ++q)
                if (4 * q < D) o4[q] = make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D) o[j] = p[j];
        }
    }
}

template <int DMAX, bool GREEDY>
bool launch_continue(const ContModel &cm, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                     int stop_tree, const float *base, float *out, hipStream_t s) {
    const size_t lds = static_cast<size_t>(kContRows) * (F | 1) * sizeof(float);
    if (lds > 156 * 1024) return false;   // rows too wide for an LDS tile
    static PerDeviceOnce attr;
    if (attr.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_continue<DMAX, GREEDY>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    }
    ContOwner<DMAX> own;
    for (int j = 0; j < DMAX; ++j) own.opt[j] = j < pm.D ? pm.owner[j] : 0;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_io = d4 && ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL((k_continue<DMAX, GREEDY>), dim3((n + kContRows - 1) / kContRows), dim3(kContRows), lds, s, cm, own, pm.coef_cover, obs, F,
                       cat_codes, Fc, n, start_tree, stop_tree, base, out, vec_values, vec_io);
    return true;
}

template <bool GREEDY>
bool launch_continue_d(const ContModel &cm, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                       int stop_tree, const float *base, float *out, hipStream_t s) {
    if (pm.D <= 4) return launch_continue<4, GREEDY>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s);
    if (pm.D <= 8) return launch_continue<8, GREEDY>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s);
    if (pm.D <= 16) return launch_continue<16, GREEDY>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s);
    if (pm.D <= 32) return launch_continue<32, GREEDY>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s);
    return launch_continue<64, GREEDY>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s);
}

}  // namespace

void predict_continue(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                      const float *base, float *out, bool generic, hipStream_t s) {
    if (stop_tree <= start_tree || pm.n_opts <= 0) {   // no tree to apply, or no optimizer that owns an output: the base as it is
        if (out != base) (void)hipMemcpyAsync(out, base, sizeof(float) * static_cast<size_t>(n) * pm.D, hipMemcpyDeviceToDevice, s);
        return;
    }
    ContModel cm{};
    cm.tree_indices = pm.tree_indices; cm.depths = pm.depths; cm.feature_indices = pm.feature_indices; cm.cat_ids = pm.cat_ids;
    cm.cond_pack = pm.cond_pack; cm.grd_nodes = pm.grd_nodes; cm.grd_node_off = pm.grd_node_off;
    cm.opt_start = pm.opt_start; cm.opt_stop = pm.opt_stop;
    cm.feature_values = pm.feature_values; cm.values = pm.values;
    cm.rate = pm.rate != nullptr ? pm.rate : pm.opt_lr;
    cm.rate_stride = pm.rate != nullptr ? pm.n_opts : 0;
    cm.is_numerics = pm.is_numerics; cm.inequality_directions = pm.inequality_directions;
    cm.n_leaves = pm.n_leaves; cm.max_depth = pm.max_depth; cm.D = pm.D; cm.oblivious = pm.oblivious; cm.n_opts = pm.n_opts;
    // the streaming family: every output owned by at most one optimizer (owner[] is valid), the packed conditions / rebuilt node records
    const bool fast = !generic && pm.coef_ok && pm.D <= 64 && pm.max_depth >= 1 &&
                      (pm.oblivious ? pm.cond_pack != nullptr : (pm.grd_ok && pm.grd_nodes != nullptr && pm.grd_node_off != nullptr));
    if (fast) {
        if (pm.oblivious ? launch_continue_d<false>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s)
                         : launch_continue_d<true>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s))
            return;
    }
    dim3 grid((n + 255) / 256), block(256);
    if (pm.D <= 8)
        hipLaunchKernelGGL(k_continue_general<8>, grid, block, 0, s, cm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out);
    else if (pm.D <= 32)
        hipLaunchKernelGGL(k_continue_general<32>, grid, block, 0, s, cm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out);
    else
        hipLaunchKernelGGL(k_continue_general<128>, grid, block, 0, s, cm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out);
}

}  // namespace kern
}  // namespace gbrl
