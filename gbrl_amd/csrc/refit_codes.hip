// refit_codes.hip -- gfx950 kernels behind GBRL::refit_leaves_prepared: the leaf values of the trees [start, stop) fitted again on a prepared data set,
// the structure kept, with an objective's gradient mean (refit.hip's rule) or its Newton step (newton_core.h's).  The running prediction P [n][D]
// and a copy of the whole value table (new_values: the refit writes its range there, pm.values is only read) live on the device for the whole
// range; the host enqueues everything and never waits.
//
// The design point: the rows are walked in k_continue_codes' geometry (one wave per 64-row tile, the 32-byte code records staged by
// stream_stage_code_tile at the odd word stride; P, the targets and the weight in registers, in flight with the tile), and the tile STAYS in LDS, so
// one row pass walks TWO trees: tree t - 1, whose new values have just been finalized, is applied to P (predict_continue's chain, stream_chain_group),
// P is stored, g (and h) of the advanced P are computed from objective_core.h / newton_core.h, and tree t is walked on the same tile to find the leaf
// the row's integers join (leaf_accum.h's int64 LDS accumulators behind the tile, flushed once per block).  No leaf index per row is kept and no
// pass only applies.  One kernel template, NV values per output and leaf:
//
//   NV = 2  Newton        one row pass per tree: apply t - 1, store P, q(g), q(h), 1 into W = 2 D + 1 words; the quantum newton_sum_bits(n, weight_max)
//                         does not depend on the data.  The tree's flag word collects kNewtonBadPred / kNewtonBadTarget.
//   NV = 0  advance       the first of the gradient rule's two passes: apply t - 1, store P, max |g| of tree t by refit.hip's integer maximum on the
//                         float bits (a prediction that is not finite counts as +inf) -- the quantum leaf_sum_bits(n, max |g|) needs it first.
//   NV = 1  accumulate    the second: g again from P, tree t walked, q(g), 1 into W = D + 1 words.
//   k_refit_codes_finalize   one small launch per tree: the new values from the sums (newton_leaf_quotient / refit_mean_value, mixed with the old
//                         value by refit_mix) into new_values, the rows per leaf into counts.
//   tail                  the last tree is applied and the objective's row loss reduced by k_continue_codes' own fused-loss tail: predict_continue_codes
//                         on [stop - 1, stop) with new_values as the model's values.
//
// k_refit_codes_general is the one-thread-per-row form of the three passes: the records read in place, P advanced in global memory output by output,
// one global atomic per wave, leaf and word (k_newton_sums_general's scheme).  D > 64, optimizers that share outputs, rows too wide for the tile,
// accumulators that do not fit in LDS, a refused LDS opt-in, a greedy model without node records, GBRL_HIP_CONTINUE_GENERIC=1.  Every sum is an
// integer and every float operation is written out: both forms write the same bytes.
#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"
#include "predict_rowwalk.h"
#include "newton_core.h"
#include "refit_common.h"

#include <cmath>

namespace gbrl {
namespace kern {

namespace {

constexpr int kRefitCodesSumBlocksPerCu = 4;    // one-wave blocks per CU of a pass that flushes leaves x W global atomics per block
constexpr int kRefitCodesWalkBlocksPerCu = 16;  // ... of the advance pass, which flushes nothing: as many waves as hide the loads

struct RefitCodesPass : TreeSpan {   // t: the tree whose leaves are summed (NV > 0) or whose max |g| is taken (NV == 0)
    int apply_t;                     // the tree whose new values advance P in front (-1: none)
    unsigned long long *acc;         // [n_leaves][NV D + 1]
    uint32_t *slot;                  // the tree's word: NV == 2 the flag bits; NV == 0 receives the bits of max |g|; NV == 1 reads them
    double scale;                    // NV == 2: 2^bits
};

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int OBJ, bool WEIGHTED, int NV>
__global__ __launch_bounds__(256) void k_refit_codes_general(ChainModel cm, RefitCodesPass ps, CodeRows cr, int n, float *P, const float *__restrict__ targets,
                                                             const float *__restrict__ weights) {
#pragma clang fp contract(off)
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = row < static_cast<size_t>(n);   // (dead lanes stay for the ballots)
    const size_t rr = live ? row : 0;
    const GeneralCodeRow r{cr.codes + (static_cast<size_t>(cr.row0) + rr) * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const int lane = threadIdx.x & (kWave - 1);
    const int D = cm.D, W = NV * D + 1;
    float *p = P + rr * D;
    if (ps.apply_t >= 0 && live) {   // general_apply's chain on the row in memory: every optimizer that owns the output, in order
        const int leaf = general_leaf(cm.walk, r, ps.apply_t);
        if (leaf >= 0) {
            const float *v = cm.values + static_cast<size_t>(leaf) * D;
            for (int o = 0; o < cm.rates.n_opts; ++o) {
                const float lr = cm.rates.rate[static_cast<size_t>(ps.apply_t) * cm.rates.rate_stride + o];
                const int b = min(cm.rates.opt_stop[o], D);
#pragma unroll 1
                for (int j = max(cm.rates.opt_start[o], 0); j < b; ++j) p[j] = __fmaf_rn(-lr, v[j], p[j]);
            }
        }
    }
    int l = -1;
    if (NV > 0 && live) l = local_leaf(general_leaf(cm.walk, r, ps.t), ps.leaf0, ps.n_leaves);
    const float *y = targets + rr * (OBJ == kObjSoftmax ? 1 : D);
    float w = 1.0f;
    if constexpr (WEIGHTED) w = weights[rr];
    int label = 0;
    float mx = 0.0f, S = 1.0f;
    if constexpr (OBJ == kObjSoftmax) {   // obj_softmax_grad_row's first two loops
        label = *reinterpret_cast<const int32_t *>(y);
        mx = p[0];
#pragma unroll 1
        for (int c = 1; c < D; ++c) mx = p[c] > mx ? p[c] : mx;
        S = 0.0f;
#pragma unroll 1
        for (int c = 0; c < D; ++c) S = S + obj_exp_f32(p[c] == mx ? 0.0f : p[c] - mx);
    }
    const double scale = NV == 2 ? ps.scale : NV == 1 ? refit_scale(n, ps.slot) : 0.0;
    unsigned flag = 0;
    uint32_t gm = 0;
#pragma unroll 1
    for (int d = 0; d < D; ++d) {
        const float pd = p[d];
        float g, h = 0.0f;
        if constexpr (OBJ == kObjSoftmax) {
            const float q = obj_div(obj_exp_f32(pd == mx ? 0.0f : pd - mx), S);
            h = obj_softmax_hess_of(q);
            g = obj_softmax_grad_of(q, d == label);
        } else if constexpr (OBJ == kObjLogistic) {
            const float yd = y[d];
            if (NV == 2 && live && newton_bad_target(yd)) flag |= kNewtonBadTarget;
            obj_logistic_grad_hess(pd, yd, g, h);
        } else {
            g = __fsub_rn(pd, y[d]);
        }
        const bool bad_p = newton_bad_pred(pd);
        if (live && bad_p) flag |= kNewtonBadPred;
        if constexpr (WEIGHTED) {
            g = obj_weighted(w, g);
            h = obj_weighted(w, h);
        }
        if constexpr (NV == 0) {
            if (live) gm = max(gm, bad_p ? 0x7f800000u : refit_abs_bits(g));
        } else {
            const long long qg = l >= 0 ? newton_quantise(g, scale) : 0ll, qh = NV == 2 && l >= 0 ? newton_quantise(h, scale) : 0ll;
            for_each_wave_leaf(l, lane, [&](int k, bool mine, unsigned long long, bool leader) {
                const long long sg = wave_sum(mine ? qg : 0ll);
                long long sh = 0;
                if constexpr (NV == 2) sh = wave_sum(mine ? qh : 0ll);
                if (leader) {
                    unsigned long long *a = ps.acc + static_cast<size_t>(k) * W;
                    if (sg != 0) atomicAdd(&a[d], static_cast<unsigned long long>(sg));
                    if (sh != 0) atomicAdd(&a[D + d], static_cast<unsigned long long>(sh));
                }
            });
        }
    }
    if constexpr (NV == 0) {
        refit_block_max(gm, ps.slot);
    } else {
        for_each_wave_leaf(l, lane, [&](int k, bool, unsigned long long same, bool leader) {
            if (leader) atomicAdd(&ps.acc[static_cast<size_t>(k) * W + NV * D], static_cast<unsigned long long>(__popcll(same)));
        });
        if (NV == 2 && flag) atomicOr(ps.slot, flag);
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED, int NV>
__global__ __launch_bounds__(kStreamRows) void k_refit_codes(ChainModel cm, StreamOwner<DMAX> own, uint64_t cover, RefitCodesPass ps, CodeRows cr, int n,
                                                             int n_tiles, float *P, const float *__restrict__ targets, const float *__restrict__ weights,
                                                             int vec_values, int vec_p, int vec_y) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) uint32_t rctile[];   // [kStreamRows][stream_code_stride(G)] words, then (NV > 0) [n_leaves][NV D + 1] int64
    const int lane = threadIdx.x;
    const int D = cm.D;
    const int ws = stream_code_stride(cr.groups);
    const LeafAccLds<(NV > 0 ? NV : 1)> lacc{reinterpret_cast<unsigned long long *>(rctile + static_cast<size_t>(kStreamRows) * ws), NV > 0 ? ps.n_leaves : 0, NV * D + 1};
    if constexpr (NV > 0) lacc.zero(lane);
    const double scale = NV == 2 ? ps.scale : NV == 1 ? refit_scale(n, ps.slot) : 0.0;
    unsigned flag = 0;
    uint32_t gm = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (uniform over the block)
        const int r0 = tile * kStreamRows;
        const int rows = min(kStreamRows, n - r0);
        const bool live = lane < rows;
        const size_t row = static_cast<size_t>(r0) + (live ? lane : 0);   // (a lane without a row names the tile's first: a valid record, never stored or summed)
        float g[DMAX], h[DMAX];   // the row's prediction and targets, then its gradient and hessian; in flight together with the tile
        stream_load_row<DMAX>(P + row * D, D, vec_p != 0, g);
        int label = 0;
        if constexpr (OBJ == kObjSoftmax) label = reinterpret_cast<const int32_t *>(targets)[row];
        else stream_load_row<DMAX>(targets + row * D, D, vec_y != 0, h);
        float w = 1.0f;
        if constexpr (WEIGHTED) w = weights[row];
        __syncthreads();   // the previous tile has been read (and, the first time, the accumulators are zero)
        stream_stage_code_tile(rctile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, cr.row0 + static_cast<int>(row), rows, lane);
        __syncthreads();
        const StreamCodeRow x{reinterpret_cast<const uint16_t *>(rctile + lane * ws)};
        if (ps.apply_t >= 0 && live) {   // the first walk of the tile: predict_continue's chain through the tree before, its new values
            stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, static_cast<const int32_t *>(nullptr), ps.apply_t, ps.apply_t + 1, vec_values, g);
            stream_store_row<DMAX>(P + row * D, D, vec_p != 0, g);
        }
        int l = -1;   // the second: the leaf of tree t
        if (NV > 0 && live) l = local_leaf(stream_leaf<GREEDY>(cm.walk, x, static_cast<const int32_t *>(nullptr), ps.t), ps.leaf0, ps.n_leaves);
        bool bad_p = false, bad_y = false;
#pragma unroll
        for (int j = 0; j < DMAX; ++j)
            if (j < D) {
                bad_p = bad_p || newton_bad_pred(g[j]);
                if constexpr (OBJ == kObjLogistic) bad_y = bad_y || newton_bad_target(h[j]);
            }
        if (live) flag |= (bad_p ? kNewtonBadPred : 0) | (bad_y ? kNewtonBadTarget : 0);
        if constexpr (OBJ == kObjSoftmax) {
            obj_softmax_grad_hess_regs<DMAX>(g, h, D, label);
        } else if constexpr (OBJ == kObjLogistic) {
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D) obj_logistic_grad_hess(g[j], h[j], g[j], h[j]);
        } else {
#pragma unroll
            for (int j = 0; j < DMAX; ++j) g[j] = __fsub_rn(g[j], h[j]);
        }
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int j = 0; j < DMAX; ++j) {
                g[j] = obj_weighted(w, g[j]);
                if constexpr (NV == 2) h[j] = obj_weighted(w, h[j]);
            }
        }
        if constexpr (NV == 0) {
            uint32_t m = bad_p ? 0x7f800000u : 0u;
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D) m = max(m, refit_abs_bits(g[j]));
            if (live) gm = max(gm, m);
        } else {
            lacc.template add<DMAX>(l, lane, D, [&](int v, int j) { return newton_quantise(v == 0 ? g[j] : h[j], scale); });
        }
    }
    if constexpr (NV == 0) {
        refit_block_max(gm, ps.slot);
    } else {
        lacc.flush(ps.acc, lane);
        if (NV == 2 && flag) atomicOr(ps.slot, flag);
    }
}

// ------------------------------------------------------------------------------------------------------------ finalize
struct RefitCodesRule { int newton; double scale, leaf_l2, decay, keep; };

__global__ __launch_bounds__(256) void k_refit_codes_finalize(RefitCodesPass ps, RefitCodesRule rule, const int32_t *__restrict__ depths, int oblivious,
                                                              const float *__restrict__ values, int n, int D, float *__restrict__ new_values,
                                                              long long *__restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ps.n_leaves * D) return;
    const int l = i / D, j = i - l * D;
    const int W = (rule.newton ? 2 : 1) * D + 1;
    const size_t at = static_cast<size_t>(ps.leaf0 + l) * D + j;
    const float old = values[at];
    const unsigned long long *a = ps.acc + static_cast<size_t>(l) * W;
    const long long Sg = static_cast<long long>(a[j]), cnt = static_cast<long long>(a[W - 1]);
    const int depth = oblivious ? depths[ps.t] : depths[ps.leaf0 + l];
    float v = old;
    if (rule.newton) {
        double q = 0.0;
        if (newton_leaf_quotient(Sg, static_cast<long long>(a[D + j]), cnt, depth, rule.scale, rule.leaf_l2, q))
            v = refit_mix(rule.decay, rule.keep, old, static_cast<double>(static_cast<float>(q)));   // (newton_leaf_value's float, then the mix)
    } else {
        v = refit_mean_value(Sg, cnt, depth, old, n, ps.slot, rule.decay, rule.keep);
    }
    new_values[at] = v;
    if (j == 0) counts[l] = cnt;
}

template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED, int NV>
bool launch_refit_codes(const ChainModel &cm, const PredictModel &pm, const RefitCodesPass &ps, const CodeRows &cr, int n, float *P, const float *targets,
                        const float *weights, hipStream_t s) {
    const int n_tiles = (n + kStreamRows - 1) / kStreamRows;
    const LeafAccPlan plan = leaf_acc_plan(stream_code_tile_bytes(cr.groups), NV > 0 ? static_cast<size_t>(ps.n_leaves) * (NV * pm.D + 1) * sizeof(unsigned long long) : 0,
                                           n_tiles, NV > 0 ? kRefitCodesSumBlocksPerCu : kRefitCodesWalkBlocksPerCu, stream_cu_count());
    if (!plan.fits) return false;   // rows too wide, or a tree with too many accumulators, for the LDS of a CU
    static StreamLdsOptIn optin;
    if (!optin.ok(k_refit_codes<DMAX, GREEDY, OBJ, WEIGHTED, NV>, plan.lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(cm.values) & 15) == 0;
    const int vec_p = d4 && (reinterpret_cast<uintptr_t>(P) & 15) == 0;
    const int vec_y = d4 && OBJ != kObjSoftmax && (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    hipLaunchKernelGGL((k_refit_codes<DMAX, GREEDY, OBJ, WEIGHTED, NV>), dim3(plan.blocks), dim3(kStreamRows), plan.lds, s, cm, stream_owner<DMAX>(pm), pm.coef_cover, ps,
                       cr, n, n_tiles, P, targets, weights, vec_values, vec_p, vec_y);
    return true;
}

// one row pass in whichever form takes it; true: the streaming kernel
template <int OBJ, bool WEIGHTED, int NV>
bool refit_codes_pass(const PredictModel &pm, const ChainModel &cm, const RefitCodesPass &ps, const CodeRows &cr, int n, float *P, const float *targets,
                      const float *weights, bool generic, hipStream_t s) {
    if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_refit_codes<DMAX, false, OBJ, WEIGHTED, NV>(cm, pm, ps, cr, n, P, targets, weights, s)
                                : launch_refit_codes<DMAX, true, OBJ, WEIGHTED, NV>(cm, pm, ps, cr, n, P, targets, weights, s);
        }))
        return true;
    hipLaunchKernelGGL((k_refit_codes_general<OBJ, WEIGHTED, NV>), dim3((n + 255) / 256), dim3(256), 0, s, cm, ps, cr, n, P, targets, weights);
    return false;
}

template <int OBJ, bool WEIGHTED>
int refit_codes_range(const PredictModel &pm, const ChainModel &cm, const CodeRows &cr, const int32_t *tree_first_leaf, int n, int start_tree, int stop_tree,
                      const RefitCodesRule &rule, const float *targets, const float *weights, float *P, unsigned long long *acc, long long *counts, uint32_t *slots,
                      bool generic, hipStream_t s) {
    const int D = pm.D, W = (rule.newton ? 2 : 1) * D + 1;
    auto first_leaf = [&](int t) { return t < pm.n_trees ? tree_first_leaf[t] : pm.n_leaves; };
    const int base = first_leaf(start_tree);
    int streamed = 0;
    for (int t = start_tree; t < stop_tree; ++t) {
        RefitCodesPass ps{};
        ps.t = t; ps.leaf0 = first_leaf(t); ps.n_leaves = first_leaf(t + 1) - ps.leaf0;
        ps.apply_t = t > start_tree ? t - 1 : -1;
        ps.acc = acc + static_cast<size_t>(ps.leaf0 - base) * W;
        ps.slot = slots + (t - start_tree);
        ps.scale = rule.scale;
        bool took;
        if constexpr (OBJ != kObjRmse) {
            if (rule.newton) {
                took = refit_codes_pass<OBJ, WEIGHTED, 2>(pm, cm, ps, cr, n, P, targets, weights, generic, s);
            } else {
                refit_codes_pass<OBJ, WEIGHTED, 0>(pm, cm, ps, cr, n, P, targets, weights, generic, s);
                ps.apply_t = -1;
                took = refit_codes_pass<OBJ, WEIGHTED, 1>(pm, cm, ps, cr, n, P, targets, weights, generic, s);
            }
        } else {
            refit_codes_pass<OBJ, WEIGHTED, 0>(pm, cm, ps, cr, n, P, targets, weights, generic, s);
            ps.apply_t = -1;
            took = refit_codes_pass<OBJ, WEIGHTED, 1>(pm, cm, ps, cr, n, P, targets, weights, generic, s);
        }
        streamed += took ? 1 : 0;
        hipLaunchKernelGGL(k_refit_codes_finalize, dim3((ps.n_leaves * D + 255) / 256), dim3(256), 0, s, ps, rule, pm.depths, pm.oblivious, pm.values, n, D,
                           const_cast<float *>(cm.values), counts + (ps.leaf0 - base));
    }
    return streamed;
}

}  // namespace

int refit_leaves_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, const int32_t *tree_first_leaf, int n, int start_tree, int stop_tree,
                       int objective, bool newton, int bits, double leaf_l2, double decay, const void *targets, const float *weights, float *P,
                       unsigned long long *acc, float *new_values, long long *counts, uint32_t *slots, double *loss_part, bool generic, hipStream_t s) {
    // P over the trees before the range: the tiled bias carried through [0, start_tree) by predict_continue_codes' own kernels
    tile_rows(pm.bias, pm.D, n, P, s);
    if (start_tree > 0) predict_continue_codes(pm, ct, cr, n, 0, start_tree, P, P, nullptr, nullptr, nullptr, nullptr, generic, s);
    PredictModel pn = pm;   // the model as it will be: the same structure, the values of the refitted table
    pn.values = new_values;
    ChainModel cm = chain_model(pn);   // the view of the code walk: the threshold words replaced by bins
    cm.walk.cond_pack = ct.cond_pack;
    cm.walk.grd_nodes = ct.grd_nodes;
    cm.walk.feature_bins = ct.bins;
    const RefitCodesRule rule{newton ? 1 : 0, std::ldexp(1.0, bits), leaf_l2, decay, 1.0 - decay};
    const float *y = static_cast<const float *>(targets);
    auto run = [&](auto obj, auto weighted) {
        return refit_codes_range<decltype(obj)::value, decltype(weighted)::value>(pm, cm, cr, tree_first_leaf, n, start_tree, stop_tree, rule, y, weights, P, acc,
                                                                                  counts, slots, generic, s);
    };
    auto with_weights = [&](auto obj) { return weights != nullptr ? run(obj, std::true_type{}) : run(obj, std::false_type{}); };
    const int streamed = objective == kObjSoftmax    ? with_weights(std::integral_constant<int, kObjSoftmax>{})
                         : objective == kObjLogistic ? with_weights(std::integral_constant<int, kObjLogistic>{})
                                                     : with_weights(std::integral_constant<int, kObjRmse>{});
    // the last tree applied and the row losses reduced in one pass: k_continue_codes' fused-loss tail on the refitted values
    predict_continue_codes(pn, ct, cr, n, stop_tree - 1, stop_tree, P, P, nullptr, nullptr, y, loss_part, generic, s, objective, weights);
    return streamed;
}

}  // namespace kern
}  // namespace gbrl
