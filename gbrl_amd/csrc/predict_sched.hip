// predict_sched.hip -- gfx950 kernels behind GBRL::predict for ensembles with a Linear learning-rate schedule (scheduler.h:124-134).
//
// A Const optimizer scales every tree by one rate, so the kernels of predict.hip carry one rate per output in registers.  A Linear
// optimizer scales tree t -- its ABSOLUTE index, also when a call starts at a later tree (predictor.cpp:220, 261) -- by lr(t); the
// engine keeps rate[t][optimizer] on the device (Engine::sync_model_to_device, filled by gbrl::scheduler_lr: the only definition of
// the schedule) and the kernels here read it.  Per (row, output) the sum is still ONE chain in tree order,
// p = fma(-rate[t][o], value, p) (optimizer.cpp:110-118), so the three kernels return the same bits when each walks the whole range:
//
//   k_sched_general   anything the file format can hold: one thread per row, the reference's walk (greedy: leaf by leaf, Q7),
//                     optimizers that share outputs, D <= 128.
//   k_sched_stream    large batches (>= 32 768 rows), both grow policies, categorical columns: lane = row, the row tile and a group of
//                     trees (values transposed, greedy: node records) in LDS -- the layout of k_predict_obl / k_predict_grd -- all
//                     outputs of a row in registers.  rate[t][o(j)] has a wave-uniform address: it arrives through the scalar cache
//                     (one scalar load per output and tree, no vector or LDS instruction).  Two 128-row blocks share a CU when the
//                     rows are narrow enough, so that one block's staging overlaps the other's walk.
//   k_sched_relay     <= 8192 rows against long ensembles: the leaf search of predict_chain.hip (it does not depend on rates) and its
//                     relay of the chains between the waves of a block, with the tree's rate fetched next to the tree's value.
//
// ONE EXCEPTION to "the same bits", inherited from kern::predict: small batches (<= 16 384 rows; beyond 1024 rows against 128 .. 2048
// trees, or fewer than 2 * par_th rows against more) have their trees spread over block columns, for a Const ensemble and for a scheduled one
// alike.  k_sched_stream then writes one partial chain per slice (started at 0, rates by ABSOLUTE tree index) and predict_combine adds
// bias + the slices in tree order: within 1e-5 of the one chain, not its bits -- and, for a schedule that happens to be constant, the bits
// a Const twin gets there.  fit() never slices.
//
// A model whose optimizers are all Const never comes here (kern::predict tests PredictModel::rate).
#include "kernels.h"
#include "hooks.h"
#include "kernels_common.h"

#include <algorithm>
#include <cstdlib>

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX>
__global__ __launch_bounds__(256) void k_sched_general(PredictModel pm, const float *__restrict__ rate, const float *__restrict__ obs, int F,
                                                       const int32_t *__restrict__ cat_codes, int Fc, int n, int start_tree, int stop_tree,
                                                       float *__restrict__ out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const int D = pm.D, md = pm.max_depth;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? 0.0f + pm.bias[j] : 0.0f;
    const float *x = obs + static_cast<size_t>(row) * F;
    const int32_t *xc = cat_codes ? cat_codes + static_cast<size_t>(row) * Fc : nullptr;
    auto test = [&](int c) -> bool {
        const int f = pm.feature_indices[c];
        return pm.is_numerics[c] ? (x[f] > pm.feature_values[c]) : (xc != nullptr && xc[f] == pm.cat_ids[c]);
    };
    auto apply = [&](int t, const float *v) {
        for (int o = 0; o < pm.n_opts; ++o) {
            const float lr = rate[static_cast<size_t>(t) * pm.n_opts + o];
            const int a = pm.opt_start[o], b = pm.opt_stop[o];
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j >= a && j < b) p[j] = fmaf(-lr, v[j], p[j]);
        }
    };
    if (stop_tree > start_tree && pm.n_opts > 0) {
        if (pm.oblivious) {
            for (int t = start_tree; t < stop_tree; ++t) {
                const int depth = pm.depths[t], cond = t * md;
                int leaf = 0;
                for (int d = 0; d < depth; ++d) leaf |= (test(cond + d) ? 1 : 0) << (depth - 1 - d);
                apply(t, pm.values + static_cast<size_t>(pm.tree_indices[t] + leaf) * D);
            }
        } else {
            int t = start_tree;
            int leaf = pm.tree_indices[t];
            while (leaf < pm.n_leaves && t < stop_tree) {
                const int depth = pm.depths[leaf], cond = leaf * md;
                bool passed = false;
                for (int d = depth - 1; d >= 0; --d) {
                    passed = (test(cond + d) == (pm.inequality_directions[cond + d] != 0));
                    if (!passed) break;
                }
                if (passed) {
                    apply(t, pm.values + static_cast<size_t>(leaf) * D);
                    ++t;
                    if (t < stop_tree) leaf = pm.tree_indices[t];
                } else {
                    ++leaf;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < D) out[static_cast<size_t>(row) * D + j] = p[j];
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX>
struct SchedOwner { int32_t opt[DMAX]; };   // optimizer that owns output j (padded outputs: optimizer 0, their values are zero)

// coalesced staging of rows [r0, r0 + rows) into an LDS tile with the odd row stride xs (64 consecutive rows of one feature: 64 banks)
__device__ __forceinline__ void sched_stage_rows(const float *__restrict__ obs, int r0, int rows, int F, int xs, float *__restrict__ xt) {
    const int R = blockDim.x;
    const float *src = obs + static_cast<size_t>(r0) * F;
    if (F > 0 && (F & 3) == 0 && (reinterpret_cast<uintptr_t>(obs) & 15) == 0) {
        const float4 *src4 = reinterpret_cast<const float4 *>(src);
        const int F4 = F >> 2, tot4 = rows * F4;
        constexpr int UL = 8;   // 16-byte loads in flight per thread
        for (int i0 = threadIdx.x; i0 < tot4; i0 += R * UL) {
            float4 v[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * R;
                v[u] = i < tot4 ? src4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * R;
                if (i < tot4) {
                    const int r = i / F4, f = (i - r * F4) << 2;
                    float *dst = xt + r * xs + f;
                    dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
                }
            }
        }
    } else {
        const int tot = rows * F;
        for (int i = threadIdx.x; i < tot; i += R) {
            const int r = i / F, f = i - r * F;
            xt[r * xs + f] = src[i];
        }
    }
}

template <int DMAX, bool GREEDY>
__global__ __launch_bounds__(256) void k_sched_stream(const float *__restrict__ values, const int32_t *__restrict__ tree_indices,
                                                      const int32_t *__restrict__ depths, const int32_t *__restrict__ cond_pack, int md,
                                                      const int32_t *__restrict__ nodes, const int32_t *__restrict__ node_off,
                                                      const float *__restrict__ bias, const float *__restrict__ rate, int n_opts,
                                                      SchedOwner<DMAX> own, int D, int n_leaves_total, int n_trees_total, int max_nodes, int LS,
                                                      const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes, int Fc, int n,
                                                      int start_tree, int stop_tree, float *__restrict__ out, int TT, int tree_chunk) {
    extern __shared__ float ptile[];
    // tree_chunk > 0: this block covers the trees [start + y*chunk, ...) only and writes a PARTIAL sum (no bias) into slice y of `out`
    // (small batches with large ensembles, the slices kern::predict chooses for Const ensembles; predict_combine adds them in tree order)
    if (tree_chunk > 0) {
        start_tree += blockIdx.y * tree_chunk;
        if (blockIdx.y + 1 < gridDim.y) stop_tree = min(stop_tree, start_tree + tree_chunk);   // the last slice takes the remainder
        out += static_cast<size_t>(blockIdx.y) * n * D;
    }
    const int R = blockDim.x;
    const int xs = F | 1;
    float *xt = ptile;                                              // [R][xs]
    float *vt = ptile + static_cast<size_t>(R) * xs;                // [TT][DMAX][LS]: the leaf's outputs at immediate offsets from one address
    int4 *nt = reinterpret_cast<int4 *>(vt + static_cast<size_t>(TT) * DMAX * LS);              // [TT][max_nodes]   (greedy)
    int *tmeta = reinterpret_cast<int *>(nt + (GREEDY ? static_cast<size_t>(TT) * max_nodes : 0));   // [TT][4]: first leaf, leaves, first node, nodes
    const int r0 = blockIdx.x * R;
    const int rows = min(R, n - r0);
    sched_stage_rows(obs, r0, rows, F, xs, xt);
    const bool live = static_cast<int>(threadIdx.x) < rows;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = (j < D && tree_chunk == 0) ? 0.0f + bias[j] : 0.0f;
    const float *x = xt + threadIdx.x * xs;
    const int32_t *xc = (cat_codes && live) ? cat_codes + static_cast<size_t>(r0 + threadIdx.x) * Fc : nullptr;
    const int vtree = DMAX * LS;
    for (int t0 = start_tree; t0 < stop_tree; t0 += TT) {
        const int tn = min(TT, stop_tree - t0);
        __syncthreads();   // row tile staged / previous group fully consumed
        if (static_cast<int>(threadIdx.x) < tn) {
            const int t = t0 + threadIdx.x;
            const int l0 = tree_indices[t], l1 = t + 1 < n_trees_total ? tree_indices[t + 1] : n_leaves_total;
            tmeta[4 * threadIdx.x + 0] = l0;
            tmeta[4 * threadIdx.x + 1] = min(l1 - l0, LS);
            tmeta[4 * threadIdx.x + 2] = GREEDY ? node_off[t] : 0;
            tmeta[4 * threadIdx.x + 3] = GREEDY ? min(node_off[t + 1] - node_off[t], max_nodes) : 0;
        }
        __syncthreads();
        {
            constexpr int US = 8;
            for (int i0 = threadIdx.x; i0 < tn * vtree; i0 += R * US) {
                float v[US];
                int dst[US];
#pragma unroll
                for (int u = 0; u < US; ++u) {
                    const int i = i0 + u * R;
                    dst[u] = -1;
                    v[u] = 0.0f;
                    if (i < tn * vtree) {
                        // i = (tt, leaf, j) with j fastest: consecutive threads read consecutive values of a leaf row
                        const int tt = i / vtree, e = i - tt * vtree;
                        const int leaf = e / DMAX, j = e - leaf * DMAX;
                        dst[u] = (tt * DMAX + j) * LS + leaf;
                        if (j < D && leaf < tmeta[4 * tt + 1]) v[u] = values[(static_cast<size_t>(tmeta[4 * tt]) + leaf) * D + j];
                    }
                }
#pragma unroll
                for (int u = 0; u < US; ++u)
                    if (dst[u] >= 0) vt[dst[u]] = v[u];
            }
            if (GREEDY) {
                const int4 *gn = reinterpret_cast<const int4 *>(nodes);
                for (int i = threadIdx.x; i < tn * max_nodes; i += R) {
                    const int tt = i / max_nodes, k = i - tt * max_nodes;
                    if (k < tmeta[4 * tt + 3]) nt[i] = gn[tmeta[4 * tt + 2] + k];
                }
            }
        }
        __syncthreads();
        if (live) {
            // tree t of the group: DMAX LDS reads at immediate offsets, DMAX scalar loads of the tree's rates (uniform address: the
            // tree and the owner of output j are the same for every lane), DMAX fused multiply-adds
            auto apply = [&](int tt, int leaf) {
                const float *v = vt + tt * vtree + leaf;
                const float *rt = rate + static_cast<size_t>(t0 + tt) * n_opts;
                float vv[DMAX], rr[DMAX];
#pragma unroll
                for (int j = 0; j < DMAX; ++j) { vv[j] = v[j * LS]; rr[j] = rt[own.opt[j]]; }
#pragma unroll
                for (int j = 0; j < DMAX; ++j) p[j] = fmaf(-rr[j], vv[j], p[j]);
            };
            if (GREEDY) {
                auto step = [&](const int4 *base, int &node) {
                    if (node >= 0) {
                        const int4 nd = base[node];
                        const bool right = nd.x >= 0 ? (x[nd.x] > __int_as_float(nd.y)) : (xc != nullptr && xc[~nd.x] == nd.y);
                        node = right ? nd.w : nd.z;
                    }
                };
                int tt = 0;
                for (; tt + 3 < tn; tt += 4) {   // four descents in flight (independent chains); values applied in tree order
                    int nd0 = 0, nd1 = 0, nd2 = 0, nd3 = 0;
                    const int4 *b0 = nt + tt * max_nodes, *b1 = b0 + max_nodes, *b2 = b1 + max_nodes, *b3 = b2 + max_nodes;
                    while ((nd0 & nd1 & nd2 & nd3) >= 0) {   // until all four are leaves (negative)
                        step(b0, nd0); step(b1, nd1); step(b2, nd2); step(b3, nd3);
                    }
                    apply(tt, ~nd0); apply(tt + 1, ~nd1); apply(tt + 2, ~nd2); apply(tt + 3, ~nd3);
                }
                for (; tt < tn; ++tt) {
                    int node = 0;
                    const int4 *b = nt + tt * max_nodes;
                    while (node >= 0) step(b, node);
                    apply(tt, ~node);
                }
            } else {
                // the (feature, threshold) pairs of a tree come through the scalar cache too (uniform addresses)
                auto leaf_of = [&](int t) -> int {
                    const int depth = depths[t];
                    const int32_t *cp = cond_pack + static_cast<size_t>(t) * 2 * md;
                    int leaf = 0;
                    if (md <= 8) {
                        int fi[8], tv[8];
                        float xv[8];
#pragma unroll
                        for (int d = 0; d < 8; ++d) {
                            const int dd = min(d, md - 1);   // inside the tree's own record
                            fi[d] = cp[2 * dd];
                            tv[d] = cp[2 * dd + 1];
                        }
#pragma unroll
                        for (int d = 0; d < 8; ++d) xv[d] = (d < depth && fi[d] >= 0) ? x[fi[d]] : 0.0f;
#pragma unroll
                        for (int d = 0; d < 8; ++d) {
                            if (d < depth) {
                                const bool pass = fi[d] >= 0 ? (xv[d] > __int_as_float(tv[d])) : (xc != nullptr && xc[~fi[d]] == tv[d]);
                                leaf |= (pass ? 1 : 0) << (depth - 1 - d);
                            }
                        }
                    } else {
                        for (int d = 0; d < depth; ++d) {
                            const int fi = cp[2 * d], tv = cp[2 * d + 1];
                            const bool pass = fi >= 0 ? (x[fi] > __int_as_float(tv)) : (xc != nullptr && xc[~fi] == tv);
                            leaf |= (pass ? 1 : 0) << (depth - 1 - d);
                        }
                    }
                    return leaf;
                };
                int tt = 0;
                for (; tt + 3 < tn; tt += 4) {
                    const int l0 = leaf_of(t0 + tt), l1 = leaf_of(t0 + tt + 1), l2 = leaf_of(t0 + tt + 2), l3 = leaf_of(t0 + tt + 3);
                    apply(tt, l0); apply(tt + 1, l1); apply(tt + 2, l2); apply(tt + 3, l3);
                }
                for (; tt < tn; ++tt) apply(tt, leaf_of(t0 + tt));
            }
        }
    }
    if (live) {
        float *o = out + static_cast<size_t>(r0 + threadIdx.x) * D;
#pragma unroll
        for (int j = 0; j < DMAX; ++j)
            if (j < D) o[j] = p[j];
    }
}

template <int DMAX, bool GREEDY>
bool launch_sched_stream(const PredictModel &pm, const int *owner, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                         int stop_tree, float *out, hipStream_t s) {
    const int LS = GREEDY ? pm.grd_max_leaves : (1 << pm.max_depth);
    const int MN = GREEDY ? std::max(1, pm.grd_max_nodes) : 0;
    const size_t per_tree = static_cast<size_t>(LS) * DMAX * sizeof(float) + static_cast<size_t>(MN) * 16 + 16;
    const int xs = F | 1;
    const int trees = pm.tree_chunk > 0 ? pm.tree_chunk : stop_tree - start_tree;
    // Two blocks of 128 rows per CU (160 KiB of LDS) when at least four trees of a group fit beside the rows: the staging of one
    // overlaps the walk of the other.  Otherwise one block with as many rows as fit.
    int R = 128;
    size_t budget = 78 * 1024;
    if (static_cast<size_t>(R) * xs * sizeof(float) + per_tree * std::min(trees, 4) > budget) {
        budget = 156 * 1024;
        R = 256;
        while (R >= 64 && static_cast<size_t>(R) * xs * sizeof(float) + per_tree > budget) R -= 64;
        if (R < 64) return false;
    }
    int TT = static_cast<int>((budget - static_cast<size_t>(R) * xs * sizeof(float)) / per_tree);
    TT = std::max(1, std::min(TT, std::min(64, trees)));
    const size_t lds = static_cast<size_t>(R) * xs * sizeof(float) + static_cast<size_t>(TT) * per_tree;
    static PerDeviceOnce attr;
    if (attr.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_sched_stream<DMAX, GREEDY>), hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024);
    }
    SchedOwner<DMAX> own;
    for (int j = 0; j < DMAX; ++j) own.opt[j] = j < pm.D ? owner[j] : 0;
    const int splits = pm.tree_chunk > 0 ? pm.tree_splits : 1;
    hipLaunchKernelGGL((k_sched_stream<DMAX, GREEDY>), dim3((n + R - 1) / R, splits), dim3(R), lds, s, pm.values, pm.tree_indices, pm.depths, pm.cond_pack,
                       pm.max_depth, pm.grd_nodes, pm.grd_node_off, pm.bias, pm.rate, pm.n_opts, own, pm.D, pm.n_leaves, pm.n_trees, MN, LS, obs, F,
                       cat_codes, Fc, n, start_tree, stop_tree, pm.tree_chunk > 0 ? pm.partial : out, TT, pm.tree_chunk);
    return true;
}

template <bool GREEDY>
bool launch_sched_stream_d(const PredictModel &pm, const int *owner, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                           int stop_tree, float *out, hipStream_t s) {
    if (pm.D <= 4) return launch_sched_stream<4, GREEDY>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s);
    if (pm.D <= 8) return launch_sched_stream<8, GREEDY>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s);
    if (pm.D <= 16) return launch_sched_stream<16, GREEDY>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s);
    if (pm.D <= 32) return launch_sched_stream<32, GREEDY>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s);
    return launch_sched_stream<64, GREEDY>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s);
}

// ------------------------------------------------------------------------------------------------------------ chain stage
// The relay of predict_chain.hip (k_chain_relay: W waves own the same 64 chains and take turns, a wave gathers the values of its next
// batch while the others apply theirs) with one more operand per tree: the rate of (tree, owner of the lane's output), requested
// together with the tree's value.  Those requests are cheap beside the value gathers -- the 64 lanes of a request read at most
// n_opts different words of one cache line.
struct RelayOwner {
    uint8_t opt[64];    // optimizer that owns the output
    uint64_t cover;     // outputs owned by an optimizer (the others keep the bias, like the general kernel)
};

template <int W, int U>
__global__ __launch_bounds__(64 * W) void k_sched_relay(const int32_t *__restrict__ slots, int Tn, int Ts, const float *__restrict__ values,
                                                        const float *__restrict__ bias, const float *__restrict__ rate, int n_opts, int start_tree,
                                                        RelayOwner own, int D, int n_lanes, float *__restrict__ out) {
    static_assert((3 * W - 2) * U <= kSlotPad && U == kChainU, "slot rows are padded for the batches requested behind the range");
    __shared__ float token[64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 64 + lane;            // lane i = (row, output)
    const bool live = i < n_lanes;
    const int ii = live ? i : n_lanes - 1;
    const int row = ii / D, d0 = ii - row * D;
    const float b0 = 0.0f + bias[d0];
    const float *rp = rate + static_cast<size_t>(start_tree) * n_opts + own.opt[d0];
    const int32_t *sp = slots + static_cast<size_t>(row) * Ts;
    const char *vb8 = reinterpret_cast<const char *>(values);
    const uint32_t d4 = static_cast<uint32_t>(d0) * 4u;
    int s[U];
    float v[U], c[U];
    auto load_slots = [&](int batch) {
        const int4 *q = reinterpret_cast<const int4 *>(sp + static_cast<size_t>(batch) * U);
#pragma unroll
        for (int u = 0; u < U / 4; ++u) {
            const int4 x = q[u];
            s[4 * u] = x.x; s[4 * u + 1] = x.y; s[4 * u + 2] = x.z; s[4 * u + 3] = x.w;
        }
    };
    auto load_values = [&](int batch) {   // the values whose slot words are in s[], and the rates of the batch's trees
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = *reinterpret_cast<const float *>(vb8 + (static_cast<uint32_t>(s[u]) + d4));
            const int j = min(batch * U + u, Tn - 1);   // batches requested behind the range are never applied
            c[u] = rp[static_cast<size_t>(j) * n_opts];
        }
    };
    if (w == 0) token[lane] = b0;
    const int nbt = (Tn + U - 1) / U;                 // batches, the last one possibly partial
    const int rounds = (nbt + W - 1) / W;
    if (live) {
        load_slots(w);
        load_values(w);
        load_slots(w + W);
    }
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            __syncthreads();
            if (w == j) {                              // my turn: batch r * W + j
                const int kb = r * W + j;
                if (kb < nbt && live) {
                    float p = token[lane];
                    if ((kb + 1) * U <= Tn) {
#pragma unroll
                        for (int u = 0; u < U; ++u) p = fmaf(-c[u], v[u], p);
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (kb * U + u < Tn) p = fmaf(-c[u], v[u], p);
                    }
                    token[lane] = p;
                }
            } else if (w == (j + W - 1) % W && (r > 0 || j > 0)) {
                // my turn was the previous one: request my next batch (its slot words are here) and the slot words of the one after
                const int kb = r * W + j - 1 + W;       // my next batch
                if (live) {
                    load_values(kb);
                    load_slots(kb + W);
                }
            }
        }
    }
    __syncthreads();
    if (w == 0 && live) out[static_cast<size_t>(row) * D + d0] = ((own.cover >> d0) & 1ull) ? token[lane] : b0;
}

}  // namespace

void predict_sched(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                   float *out, hipStream_t s) {
    // the fast paths: every output owned by exactly one optimizer, the packed conditions / node records of the fast Const kernels
    int owner[64];
    bool fast = pm.coef_ok && pm.D <= 64 && F > 0 && stop_tree > start_tree && pm.max_depth >= 1;
    if (fast) {
        const uint64_t all_out = pm.D >= 64 ? ~0ull : ((1ull << pm.D) - 1ull);
        fast = pm.coef_cover == all_out;
        for (int j = 0; j < pm.D && fast; ++j) owner[j] = pm.owner[j];
    }
    if (fast) fast = pm.oblivious ? (pm.obl_ok && pm.cond_pack != nullptr && pm.max_depth <= 12) : (pm.grd_ok && pm.grd_nodes != nullptr && pm.grd_max_leaves <= 256);
    // Small batches whose trees kern::predict spread over block columns (the same slices as for a Const ensemble, so a schedule that
    // happens to be constant gives the bits of its Const twin): partial sums by the streaming kernel, added in tree order.
    if (fast && pm.tree_chunk > 0) {
        if (pm.oblivious ? launch_sched_stream_d<false>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s)
                         : launch_sched_stream_d<true>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s)) {
            predict_combine(pm, n, out, s);
            return;
        }
    }
    if (fast && pm.slots != nullptr) {
        int Ts = 0;
        if (static_cast<long long>(n) * pm.D < (1ll << 31) && predict_chain_slots(pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, &Ts, s)) {
            RelayOwner own;
            for (int j = 0; j < 64; ++j) own.opt[j] = static_cast<uint8_t>(j < pm.D ? owner[j] : 0);
            own.cover = pm.coef_cover;
            const int n_lanes = n * pm.D;
            hipLaunchKernelGGL((k_sched_relay<4, 64>), dim3(static_cast<unsigned>((n_lanes + 63) / 64)), dim3(256), 0, s, pm.slots, stop_tree - start_tree, Ts,
                               pm.values, pm.bias, pm.rate, pm.n_opts, start_tree, own, pm.D, n_lanes, out);
            return;
        }
    }
    // GBRL_HIP_PREDICT_SCHED_MIN_ROWS: tests move the boundary between the streaming and the general kernel
    if (fast && n >= hooks::num(hooks::PREDICT_SCHED_MIN_ROWS, 32768)) {
        if (pm.oblivious ? launch_sched_stream_d<false>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s)
                         : launch_sched_stream_d<true>(pm, owner, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s))
            return;
    }
    dim3 grid((n + 255) / 256), block(256);
    if (pm.D <= 8)
        hipLaunchKernelGGL(k_sched_general<8>, grid, block, 0, s, pm, pm.rate, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out);
    else if (pm.D <= 32)
        hipLaunchKernelGGL(k_sched_general<32>, grid, block, 0, s, pm, pm.rate, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out);
    else
        hipLaunchKernelGGL(k_sched_general<128>, grid, block, 0, s, pm, pm.rate, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out);
}

}  // namespace kern
}  // namespace gbrl
