// newton.hip -- gfx950 kernels behind GBRL::newton_leaves_prepared and fit_prepared(leaf_update="newton"): the per-leaf sums of the objective's
// gradient and hessian over one tree, the rows read from a prepared data set's bin codes.  newton_core.h has the rule; this file only sums.
//
//   A row is routed through tree t by the code walk of predict_rowwalk.h (a leaf gets exactly the rows predict_leaves reports), its prediction
//   p[] -- the trees [0, t) -- and its targets give g and h per output (objective_core.h / newton_core.h: the bits of the host functions), and
//   q(g), q(h) = llrint((double)x * 2^bits) and a 1 are added to the leaf's int64 accumulators acc[leaf][2 D + 1] = (Sg[D], Sh[D], cnt).
//   The accumulators are leaf_accum.h's, in both of its schemes:
//
//   k_newton_sums<DMAX, GREEDY, OBJ>   streaming, in k_continue_codes' geometry, W = 2 D + 1: the 64 code records staged by stream_stage_code_tile
//                (the tile is a multiple of 256 bytes), p[] (and the logistic targets) in registers and in flight together with the tile.
//   k_newton_sums_general<OBJ>         general: the records read in place, p[] and the targets read from global memory output by output in
//                rolled loops (softmax: the row's maximum and sum first, then every exp again -- the same bits; nothing is held in a register
//                row, so D up to 128 needs no scratch).
//                D > 64, rows too wide for the tile, accumulators that do not fit in LDS, a refused LDS opt-in, a greedy model without node
//                records, and the cross-check behind GBRL_HIP_CONTINUE_GENERIC=1.
//
//   k_newton_check_targets             *flag |= kNewtonBadTarget when any entry of a logistic target matrix lies outside [0, 1].
//
//   pred / targets are indexed by the position j of the call, or (abs_index) by the data set row the position names: fit_prepared's held
//   prediction and targets are [n][D] of the whole data set while a sampled iteration sums over a row list.
//   WEIGHTED (a template flag of both sums kernels) with weights float32, indexed like pred: the row's weight is loaded with p[] and the targets,
//   and g, h become fl32(w * g), fl32(w * h) in front of the quantisation (newton_core.h: the caller's bits make room for the largest weight).
//   cnt counts rows as before.  Without the flag the pointer is never read.
//   OBJ == kObjGiven (newton_core.h; the ranking objectives): pred and targets are two float32 buffers [.][D] that hold g and h themselves; both
//   kernels load them as they load p and y and skip the objective's arithmetic and its checks.  Every other instantiation is what it was.
//   The flag word behind the accumulators collects what the caller refuses: kNewtonBadTarget (a logistic target outside [0, 1]; a NaN counts),
//   kNewtonBadPred (a prediction that is not finite).  The caller zeroes accumulators and flag and reads both back in one copy.
#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"
#include "predict_rowwalk.h"
#include "newton_core.h"

#include <algorithm>
#include <cmath>

namespace gbrl {
namespace kern {

namespace {

constexpr int kNewtonRows = kStreamRows;   // rows per block of the streaming kernel = one wave
constexpr int kNewtonBlocksPerCu = 4;      // one-wave blocks per CU: every block flushes leaves x (2 D + 1) global atomics once

struct NewtonTree : TreeSpan {
    unsigned long long *acc;     // [n_leaves][2 D + 1], then the flag word
};

// a logistic target outside [0, 1] anywhere in the matrix (fit_prepared refuses it before anything changes)
__global__ __launch_bounds__(256) void k_newton_check_targets(const float *__restrict__ targets, size_t n_el, unsigned long long *__restrict__ flag) {
    bool bad = false;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el; i += static_cast<size_t>(gridDim.x) * blockDim.x)
        bad = bad || newton_bad_target(targets[i]);
    if (bad) atomicOr(flag, static_cast<unsigned long long>(kNewtonBadTarget));
}

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int OBJ, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_newton_sums_general(LeavesModel cm, NewtonTree nt, CodeRows cr, int m, int D, const float *__restrict__ pred,
                                                             const float *__restrict__ targets, int abs_index, double scale,
                                                             const float *__restrict__ weights) {
#pragma clang fp contract(off)
    const size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = j < static_cast<size_t>(m);   // (dead lanes stay for the ballots)
    const size_t jj = live ? j : 0;
    const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + jj] : cr.row0 + static_cast<int>(jj));
    const GeneralCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const int lane = threadIdx.x & (kWave - 1);
    const int W = 2 * D + 1;
    int l = -1;
    if (live) l = local_leaf(general_leaf(cm, r, nt.t), nt.leaf0, nt.n_leaves);
    const size_t pr = abs_index ? src : jj;
    const float *p = pred + pr * D;
    const float *y = targets + pr * (OBJ == kObjSoftmax ? 1 : D);
    float w = 1.0f;
    if constexpr (WEIGHTED) w = weights[pr];
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
    unsigned flag = 0;
#pragma unroll 1
    for (int d = 0; d < D; ++d) {
        const float pd = p[d];
        float g, h;
        if constexpr (OBJ == kObjSoftmax) {
            const float q = obj_div(obj_exp_f32(pd == mx ? 0.0f : pd - mx), S);
            h = obj_softmax_hess_of(q);
            g = obj_softmax_grad_of(q, d == label);
        } else if constexpr (OBJ == kObjGiven) {   // pred holds g, targets h
            g = pd;
            h = y[d];
        } else {
            const float yd = y[d];
            if (live && newton_bad_target(yd)) flag |= kNewtonBadTarget;
            obj_logistic_grad_hess(pd, yd, g, h);
        }
        if constexpr (OBJ != kObjGiven)
            if (live && newton_bad_pred(pd)) flag |= kNewtonBadPred;
        if constexpr (WEIGHTED) {
            g = obj_weighted(w, g);
            h = obj_weighted(w, h);
        }
        const long long qg = l >= 0 ? newton_quantise(g, scale) : 0ll, qh = l >= 0 ? newton_quantise(h, scale) : 0ll;
        for_each_wave_leaf(l, lane, [&](int k, bool mine, unsigned long long, bool leader) {
            const long long sg = wave_sum(mine ? qg : 0ll), sh = wave_sum(mine ? qh : 0ll);
            if (leader) {
                unsigned long long *a = nt.acc + static_cast<size_t>(k) * W;
                if (sg != 0) atomicAdd(&a[d], static_cast<unsigned long long>(sg));
                if (sh != 0) atomicAdd(&a[D + d], static_cast<unsigned long long>(sh));
            }
        });
    }
    for_each_wave_leaf(l, lane, [&](int k, bool, unsigned long long same, bool leader) {
        if (leader) atomicAdd(&nt.acc[static_cast<size_t>(k) * W + 2 * D], static_cast<unsigned long long>(__popcll(same)));
    });
    if (flag) atomicOr(&nt.acc[static_cast<size_t>(nt.n_leaves) * W], static_cast<unsigned long long>(flag));
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED>
__global__ __launch_bounds__(kNewtonRows) void k_newton_sums(LeavesModel cm, NewtonTree nt, CodeRows cr, int m, int n_tiles, int D,
                                                             const float *__restrict__ pred, const float *__restrict__ targets, int abs_index, double scale,
                                                             int vec_p, int vec_y, const float *__restrict__ weights) {
    extern __shared__ __align__(16) uint32_t ntile[];   // [kNewtonRows][stream_code_stride(G)] words, then [n_leaves][2 D + 1] int64
    const int lane = threadIdx.x;
    const int ws = stream_code_stride(cr.groups);
    const LeafAccLds<2> lacc{reinterpret_cast<unsigned long long *>(ntile + static_cast<size_t>(kNewtonRows) * ws), nt.n_leaves, 2 * D + 1};
    lacc.zero(lane);
    unsigned flag = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (uniform over the block)
        const int r0 = tile * kNewtonRows;
        const int rows = min(kNewtonRows, m - r0);
        const bool live = lane < rows;
        const int pos = r0 + (live ? lane : 0);   // (a lane without a row names the tile's first: a valid record, never summed)
        const int at = cr.row0 + pos;
        const int my_row = cr.rows ? cr.rows[at] : at;
        const size_t pr = static_cast<size_t>(abs_index ? my_row : pos);
        float g[DMAX], h[DMAX];   // the row's prediction and targets, then its gradient and hessian; in flight together with the tile
        stream_load_row<DMAX>(pred + pr * D, D, vec_p != 0, g);
        int label = 0;
        if constexpr (OBJ == kObjSoftmax) label = reinterpret_cast<const int32_t *>(targets)[pr];
        else stream_load_row<DMAX>(targets + pr * D, D, vec_y != 0, h);
        float w = 1.0f;
        if constexpr (WEIGHTED) w = weights[pr];
        __syncthreads();   // the previous tile has been read (and, the first time, the accumulators are zero)
        stream_stage_code_tile(ntile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
        __syncthreads();
        int l = -1;
        if (live) {
            const StreamCodeRow x{reinterpret_cast<const uint16_t *>(ntile + lane * ws)};
            l = local_leaf(stream_leaf<GREEDY>(cm, x, static_cast<const int32_t *>(nullptr), nt.t), nt.leaf0, nt.n_leaves);
        }
        bool bad_p = false, bad_y = false;
        if constexpr (OBJ != kObjGiven) {
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D) {
                    bad_p = bad_p || newton_bad_pred(g[j]);
                    if constexpr (OBJ != kObjSoftmax) bad_y = bad_y || newton_bad_target(h[j]);
                }
        }
        if (live) flag |= (bad_p ? kNewtonBadPred : 0) | (bad_y ? kNewtonBadTarget : 0);
        if constexpr (OBJ == kObjSoftmax) {
            obj_softmax_grad_hess_regs<DMAX>(g, h, D, label);
        } else if constexpr (OBJ == kObjGiven) {
            // g[] and h[] are what the two loads brought
        } else {
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D) obj_logistic_grad_hess(g[j], h[j], g[j], h[j]);
        }
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int j = 0; j < DMAX; ++j) {
                g[j] = obj_weighted(w, g[j]);
                h[j] = obj_weighted(w, h[j]);
            }
        }
        lacc.template add<DMAX>(l, lane, D, [&](int v, int j) { return newton_quantise(v == 0 ? g[j] : h[j], scale); });
    }
    lacc.flush(nt.acc, lane);
    if (flag) atomicOr(&nt.acc[nt.n_leaves * lacc.W], static_cast<unsigned long long>(flag));
}

template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED>
bool launch_newton_sums(const LeavesModel &cm, const NewtonTree &nt, const CodeRows &cr, int m, int D, const float *pred, const float *targets, int abs_index,
                        double scale, const float *weights, hipStream_t s) {
    const int n_tiles = (m + kNewtonRows - 1) / kNewtonRows;
    const LeafAccPlan plan = leaf_acc_plan(stream_code_tile_bytes(cr.groups), static_cast<size_t>(nt.n_leaves) * (2 * D + 1) * sizeof(unsigned long long),
                                           n_tiles, kNewtonBlocksPerCu, stream_cu_count());
    if (!plan.fits) return false;   // rows too wide, or a tree with too many accumulators, for the LDS of a CU
    static StreamLdsOptIn optin;
    if (!optin.ok(k_newton_sums<DMAX, GREEDY, OBJ, WEIGHTED>, plan.lds)) return false;
    const bool d4 = (D & 3) == 0;
    const int vec_p = d4 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0;
    const int vec_y = d4 && OBJ != kObjSoftmax && (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    hipLaunchKernelGGL((k_newton_sums<DMAX, GREEDY, OBJ, WEIGHTED>), dim3(plan.blocks), dim3(kNewtonRows), plan.lds, s, cm, nt, cr, m, n_tiles, D, pred, targets, abs_index,
                       scale, vec_p, vec_y, weights);
    return true;
}

template <int OBJ, bool WEIGHTED>
bool newton_sums_obj(const PredictModel &pm, const LeavesModel &cm, const NewtonTree &nt, const CodeRows &cr, int m, const float *pred, const float *targets,
                     int abs_index, double scale, bool generic, const float *weights, hipStream_t s) {
    const int D = pm.D;
    if (leaves_streamable(pm, generic) && D <= 64 && with_stream_dmax(D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_newton_sums<DMAX, false, OBJ, WEIGHTED>(cm, nt, cr, m, D, pred, targets, abs_index, scale, weights, s)
                                : launch_newton_sums<DMAX, true, OBJ, WEIGHTED>(cm, nt, cr, m, D, pred, targets, abs_index, scale, weights, s);
        }))
        return true;
    hipLaunchKernelGGL((k_newton_sums_general<OBJ, WEIGHTED>), dim3((m + 255) / 256), dim3(256), 0, s, cm, nt, cr, m, D, pred, targets, abs_index, scale, weights);
    return false;
}

}  // namespace

void newton_check_targets(const float *targets, size_t n_el, unsigned long long *flag, hipStream_t s) {
    if (n_el == 0) return;
    hipLaunchKernelGGL(k_newton_check_targets, dim3(static_cast<unsigned>(std::min<size_t>((n_el + 255) / 256, 4096))), dim3(256), 0, s, targets, n_el, flag);
}

bool newton_leaf_sums(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int tree, int leaf0, int n_leaves, const float *pred,
                      const void *targets, bool abs_index, int objective, int bits, unsigned long long *acc, bool generic, hipStream_t s, const float *weights) {
    if (m <= 0 || n_leaves <= 0) return false;
    LeavesModel cm = leaves_model(pm);   // the routing view of the float walk with the threshold words replaced by bins
    cm.cond_pack = ct.cond_pack;
    cm.grd_nodes = ct.grd_nodes;
    cm.feature_bins = ct.bins;
    const NewtonTree nt{{tree, leaf0, n_leaves}, acc};
    const double scale = std::ldexp(1.0, bits);
    const float *y = static_cast<const float *>(targets);
    const int ai = abs_index ? 1 : 0;
    if (objective == kObjGiven) return newton_sums_obj<kObjGiven, false>(pm, cm, nt, cr, m, pred, y, ai, scale, generic, nullptr, s);
    if (weights != nullptr)
        return objective == kObjSoftmax ? newton_sums_obj<kObjSoftmax, true>(pm, cm, nt, cr, m, pred, y, ai, scale, generic, weights, s)
                                        : newton_sums_obj<kObjLogistic, true>(pm, cm, nt, cr, m, pred, y, ai, scale, generic, weights, s);
    return objective == kObjSoftmax ? newton_sums_obj<kObjSoftmax, false>(pm, cm, nt, cr, m, pred, y, ai, scale, generic, nullptr, s)
                                    : newton_sums_obj<kObjLogistic, false>(pm, cm, nt, cr, m, pred, y, ai, scale, generic, nullptr, s);
}

}  // namespace kern
}  // namespace gbrl
