// newton.hip -- gfx950 kernels behind GBRL::newton_leaves_prepared and fit_prepared(leaf_update="newton"): the per-leaf sums of the objective's
// gradient and hessian over one tree, the rows read from a prepared data set's bin codes.  newton_core.h has the rule; this file only sums.
//
//   A row is routed through tree t by the code walk of predict_rowwalk.h (a leaf gets exactly the rows predict_leaves reports), its prediction
//   p[] -- the trees [0, t) -- and its targets give g and h per output (objective_core.h / newton_core.h: the bits of the host functions), and
//   q(g), q(h) = llrint((double)x * 2^bits) and a 1 are added to the leaf's int64 accumulators acc[leaf][2 D + 1] = (Sg[D], Sh[D], cnt).
//   Integer adds only: exact and order-free, so every run and both kernel families produce the same bytes.
//
//   k_newton_sums<DMAX, GREEDY, OBJ>   k_continue_codes' geometry with refit.hip's accumulators: one wave per block, lane = row, the 64 code records
//                staged by stream_stage_code_tile, p[] (and the logistic targets) in registers and in flight together with the tile, the tree's
//                (2 D + 1) x leaves accumulators in LDS behind the tile (the tile is a multiple of 256 bytes), tiles in a grid-stride loop, one
//                64-bit global atomic per non-zero accumulator at the block's end: global atomics are blocks x leaves x (2 D + 1), not rows.
//                Up to kNewtonWaveLeaves leaves 16 or more lanes meet on every address; there the wave reduces a leaf's contributions with a
//                butterfly and lane 0 adds the result with a plain LDS add.  Deeper trees use one 64-bit LDS atomic per (lane, output).
//   k_newton_sums_general<OBJ>         one thread per row, the records read in place, p[] and the targets read from global memory output by output in
//                rolled loops (softmax: the row's maximum and sum first, then every exp again -- the same bits; nothing is held in a register
//                row, so D up to 128 needs no scratch), accumulators in global memory, one add per distinct leaf and wave (ballot + butterfly).
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
#include "predict_rowwalk.h"
#include "newton_core.h"

#include <algorithm>
#include <cmath>

namespace gbrl {
namespace kern {

namespace {

constexpr int kNewtonRows = kStreamRows;   // rows per block of the streaming kernel = one wave
constexpr int kNewtonWaveLeaves = 4;       // up to this many leaves: reduce within the wave (refit.hip's kRefitWaveLeaves)
constexpr int kNewtonBlocksPerCu = 4;      // one-wave blocks per CU: every block flushes leaves x (2 D + 1) global atomics once

struct NewtonTree {
    int t, leaf0, n_leaves;      // the tree, its first global leaf, its leaves
    unsigned long long *acc;     // [n_leaves][2 D + 1], then the flag word
};

// sum over the wave (every lane ends with it); integers: exact, order-free
__device__ __forceinline__ long long newton_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

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
    if (live) {
        l = general_leaf(cm, r, nt.t) - nt.leaf0;
        if (l < 0 || l >= nt.n_leaves) l = -1;   // the search left the tree: the row joins no sum
    }
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
    const unsigned long long in_tree = __ballot(l >= 0);
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
        // one add per distinct leaf of the wave: every lane of the leaf contributes to a butterfly, the lowest of them adds the result
        unsigned long long todo = in_tree;
        while (todo) {   // (wave-uniform)
            const int first = __ffsll(static_cast<long long>(todo)) - 1;
            const int k = __shfl(l, first, kWave);
            const bool mine = l == k;
            const unsigned long long same = __ballot(mine);
            const long long sg = newton_wave_sum(mine ? qg : 0ll), sh = newton_wave_sum(mine ? qh : 0ll);
            if (lane == first) {
                unsigned long long *a = nt.acc + static_cast<size_t>(k) * W;
                if (sg != 0) atomicAdd(&a[d], static_cast<unsigned long long>(sg));
                if (sh != 0) atomicAdd(&a[D + d], static_cast<unsigned long long>(sh));
            }
            todo &= ~same;
        }
    }
    unsigned long long todo = in_tree;
    while (todo) {
        const int first = __ffsll(static_cast<long long>(todo)) - 1;
        const int k = __shfl(l, first, kWave);
        const unsigned long long same = __ballot(l == k);
        if (lane == first) atomicAdd(&nt.acc[static_cast<size_t>(k) * W + 2 * D], static_cast<unsigned long long>(__popcll(same)));
        todo &= ~same;
    }
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
    const int W = 2 * D + 1;
    const int na = nt.n_leaves * W;
    unsigned long long *lacc = reinterpret_cast<unsigned long long *>(ntile + static_cast<size_t>(kNewtonRows) * ws);
    for (int i = lane; i < na; i += kNewtonRows) lacc[i] = 0ull;
    const bool few = nt.n_leaves <= kNewtonWaveLeaves;   // (uniform)
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
            l = stream_leaf<GREEDY>(cm, x, static_cast<const int32_t *>(nullptr), nt.t) - nt.leaf0;
            if (l < 0 || l >= nt.n_leaves) l = -1;
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
        if (few) {
            for (int k = 0; k < nt.n_leaves; ++k) {
                const bool mine = l == k;
                const unsigned long long same = __ballot(mine);
                if (same == 0ull) continue;   // (wave-uniform)
                unsigned long long *a = lacc + k * W;
#pragma unroll
                for (int j = 0; j < DMAX; ++j)
                    if (j < D) {
                        const long long sg = newton_wave_sum(mine ? newton_quantise(g[j], scale) : 0ll);
                        const long long sh = newton_wave_sum(mine ? newton_quantise(h[j], scale) : 0ll);
                        if (lane == 0) {
                            a[j] += static_cast<unsigned long long>(sg);
                            a[D + j] += static_cast<unsigned long long>(sh);
                        }
                    }
                if (lane == 0) a[2 * D] += static_cast<unsigned long long>(__popcll(same));
            }
        } else if (l >= 0) {
            unsigned long long *a = lacc + l * W;
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j < D) {
                    atomicAdd(&a[j], static_cast<unsigned long long>(newton_quantise(g[j], scale)));
                    atomicAdd(&a[D + j], static_cast<unsigned long long>(newton_quantise(h[j], scale)));
                }
            atomicAdd(&a[2 * D], 1ull);
        }
    }
    __syncthreads();
    for (int i = lane; i < na; i += kNewtonRows) {
        const unsigned long long v = lacc[i];
        if (v) atomicAdd(&nt.acc[i], v);
    }
    if (flag) atomicOr(&nt.acc[na], static_cast<unsigned long long>(flag));
}

template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED>
bool launch_newton_sums(const LeavesModel &cm, const NewtonTree &nt, const CodeRows &cr, int m, int D, const float *pred, const float *targets, int abs_index,
                        double scale, const float *weights, hipStream_t s) {
    const size_t lds = stream_code_tile_bytes(cr.groups) + static_cast<size_t>(nt.n_leaves) * (2 * D + 1) * sizeof(unsigned long long);
    if (lds > kStreamLdsBudget) return false;   // rows too wide, or a tree with too many accumulators, for the LDS of a CU
    static StreamLdsOptIn optin;
    if (!optin.ok(k_newton_sums<DMAX, GREEDY, OBJ, WEIGHTED>, lds)) return false;
    const int n_tiles = (m + kNewtonRows - 1) / kNewtonRows;
    const int per_cu = static_cast<int>(std::min<size_t>(kNewtonBlocksPerCu, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(lds, 1))));
    const int blocks = std::min(n_tiles, stream_cu_count() * per_cu);
    const bool d4 = (D & 3) == 0;
    const int vec_p = d4 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0;
    const int vec_y = d4 && OBJ != kObjSoftmax && (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    hipLaunchKernelGGL((k_newton_sums<DMAX, GREEDY, OBJ, WEIGHTED>), dim3(blocks), dim3(kNewtonRows), lds, s, cm, nt, cr, m, n_tiles, D, pred, targets, abs_index,
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
    const NewtonTree nt{tree, leaf0, n_leaves, acc};
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
