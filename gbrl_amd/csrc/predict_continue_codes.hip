// predict_continue_codes.hip -- gfx950 kernels behind GBRL::predict_continue_prepared and GBRL::fit_prepared: predict_continue.hip's chain with the
// row read from a prepared data set's bin codes instead of the observations.  Every condition of a tree grown on a data set compares against one
// of that data set's thresholds, and code(r, f) = #{b : thr[f][b] < obs[r, f]}, so `x > v` is `code > bin` with bin = #{b : thr[f][b] < v}
// (Engine::condition_bins has the argument; a model with a condition outside the thresholds never gets here).  The walk, the grouping of trees,
// the rates and the owner rule are predict_rowwalk.h's, instantiated with a code row: the bits are predict_continue's.
//
//   k_continue_codes          lane = row, one wave per block.  The block's 64 rows are staged from the group-major records [G][N][16] u16 into an
//                             LDS tile of G * 8 words per row at an odd word stride (stream_stage_code_tile: 16-byte loads, two lanes per record);
//                             a row costs 32 G bytes against the float walk's 4 F -- half of it when F is a multiple of 16.  With `rows` lane j
//                             stages the records of rows[row0 + j]; without, of row0 + j.  base / out / targets / grad_out are indexed by j.
//   k_continue_codes_general  one thread per row, the records read in place: D in 65..128, optimizers that share outputs, a greedy depth-0
//                             tree, F too wide for the tile, a refused LDS opt-in, and the cross-check behind GBRL_HIP_CONTINUE_GENERIC=1.
//   fused tail                targets != nullptr: grad_out[j][d] = fl32(out[j][d] - targets[j][d]) for the NEW out -- one float32 subtraction,
//                             kern::sub_arrays' bits -- in the same pass (fit_prepared's MultiRMSE gradient).
//   objective                 both kernels take the objective as a template parameter (objective_core.h; predict_loss.h has the register forms): rmse is the
//                             code below as it always was; logistic reads the same [m][D] float targets and writes obj_logistic_grad; softmax reads
//                             ONE int32 label per row (targets / loss_targets are then int32 [m] behind the float pointer) and runs the per-lane loops
//                             max / exp / sum / divide over p[] -- a lane owns a row, no cross-lane traffic.  The loss tail sums the objective's row loss.
//   loss tail                 loss_targets != nullptr: the row's sum_d (double)fl32(out - y)^2 for the NEW out, reduced over the wave's 64 rows by
//                             predict_loss.h's butterfly and written to loss_part[j / 64] -- what k_loss_of_predictions writes for these
//                             predictions, without the second pass over them (fit_prepared's validation rows).  The streaming kernel's block is
//                             one wave (kStreamRows == kStagedRows): one partial per block; the general kernel's four waves write four.  The two
//                             tails are independent options.
//   weights (row_operand)     WEIGHTED (a template flag of both kernels) with weights float32 [m], indexed by j like the targets: the row's weight
//                             is loaded with its prediction, so it is in flight with the code tile; the gradient tail stores fl32(w * g) and the
//                             loss tail multiplies the row loss by (double)w in front of the butterfly (objective_core.h has the rule).  One
//                             vector for the call: it weighs whichever tails are on.  Without the flag the pointer is never read.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"
#include "predict_loss.h"

namespace gbrl {
namespace kern {

namespace {

__global__ __launch_bounds__(256) void k_sub_rows(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out, size_t n) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) out[i] = __fsub_rn(a[i], b[i]);
}

__global__ __launch_bounds__(256) void k_tile_rows(const float *__restrict__ row, int D, size_t n_el, float *__restrict__ out) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el; i += static_cast<size_t>(gridDim.x) * blockDim.x) out[i] = row[i % D];
}

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX, int OBJ, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_continue_codes_general(ChainModel cm, CodeRows cr, int m, int start_tree, int stop_tree, const float *base, float *out,
                                                                const float *__restrict__ targets, float *__restrict__ grad_out,
                                                                const float *__restrict__ loss_targets, double *__restrict__ loss_part, int loss_nb,
                                                                const float *__restrict__ row_operand) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < m;
    if (!live && loss_targets == nullptr) return;   // (with the loss tail whole waves stay for the butterfly)
    const int D = cm.D;
    float p[DMAX];
    float w = 1.0f;
    if constexpr (WEIGHTED) w = live ? row_operand[j] : 0.0f;
    if (live) {
#pragma unroll
        for (int d = 0; d < DMAX; ++d) p[d] = d < D ? base[static_cast<size_t>(j) * D + d] : 0.0f;
        const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j);
        const GeneralCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
        for (int t = start_tree; t < stop_tree; ++t)
            if (!general_chain_tree<DMAX>(cm, r, t, p)) break;   // a greedy search ran off the ensemble: the walk ends
        if constexpr (OBJ == kObjRmse) {
#pragma unroll
            for (int d = 0; d < DMAX; ++d)
                if (d < D) {
                    out[static_cast<size_t>(j) * D + d] = p[d];
                    if (targets != nullptr) {
                        const float g = __fsub_rn(p[d], targets[static_cast<size_t>(j) * D + d]);
                        grad_out[static_cast<size_t>(j) * D + d] = WEIGHTED ? obj_weighted(w, g) : g;
                    }
                }
        } else {
            stream_store_row<DMAX>(out + static_cast<size_t>(j) * D, D, false, p);
            if (targets != nullptr)
                objective_grad_store<OBJ, DMAX, WEIGHTED>(p, objective_target_row<OBJ>(targets, j, D), D, false, false, grad_out + static_cast<size_t>(j) * D, w, row_operand);
        }
    }
    if (loss_targets != nullptr) {
        double acc = 0.0;
        if constexpr (OBJ == kObjRmse) {
            if (live) acc = staged_row_loss<DMAX>(p, loss_targets + static_cast<size_t>(j) * D, D);
        } else {
            if (live) acc = objective_loss_regs<OBJ, DMAX>(p, out + static_cast<size_t>(j) * D, objective_target_row<OBJ>(loss_targets, j, D), D, false, row_operand);
        }
        if constexpr (WEIGHTED) acc = obj_weighted_loss(w, acc);
        acc = staged_wave_sum(acc);
        const int wave = j / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
        if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < loss_nb) loss_part[wave] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED>
__global__ __launch_bounds__(kStreamRows) void k_continue_codes(ChainModel cm, StreamOwner<DMAX> own, uint64_t cover, CodeRows cr, int m, int start_tree,
                                                                int stop_tree, const float *base, float *out, const float *__restrict__ targets,
                                                                float *__restrict__ grad_out, const float *__restrict__ loss_targets,
                                                                double *__restrict__ loss_part, int vec_values, int vec_io, int vec_grad, int vec_loss,
                                                                const float *__restrict__ row_operand) {
    extern __shared__ __align__(16) uint32_t cctile[];   // [kStreamRows][stream_code_stride(G)]
    const int lane = threadIdx.x;
    const int D = cm.D;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, m - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    float p[DMAX];
    float w = 1.0f;
    if constexpr (WEIGHTED) w = live ? row_operand[row] : 0.0f;   // (one coalesced float per lane, in flight with the row and the tile)
    if (live) {
        stream_load_row<DMAX>(base + row * D, D, vec_io != 0, p);
    } else {
#pragma unroll
        for (int d = 0; d < DMAX; ++d) p[d] = 0.0f;
    }
    const int at = cr.row0 + r0 + (live ? lane : 0);   // (a lane without a row names the block's first: a valid record, never stored)
    const int my_row = cr.rows ? cr.rows[at] : at;
    stream_stage_code_tile(cctile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
    __syncthreads();
    if (live) {
        const StreamCodeRow x{reinterpret_cast<const uint16_t *>(cctile + lane * stream_code_stride(cr.groups))};
        for (int t0 = start_tree; t0 < stop_tree; t0 += kStreamGroup<DMAX>)
            stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, static_cast<const int32_t *>(nullptr), t0, stop_tree, vec_values, p);
        stream_store_row<DMAX>(out + row * D, D, vec_io != 0, p);
        if constexpr (OBJ == kObjRmse) {
            if (targets != nullptr) {
                float y[DMAX];
                stream_load_row<DMAX>(targets + row * D, D, vec_grad != 0, y);
#pragma unroll
                for (int d = 0; d < DMAX; ++d) y[d] = WEIGHTED ? obj_weighted(w, __fsub_rn(p[d], y[d])) : __fsub_rn(p[d], y[d]);
                stream_store_row<DMAX>(grad_out + row * D, D, vec_grad != 0, y);
            }
        } else {
            if (targets != nullptr)
                objective_grad_store<OBJ, DMAX, WEIGHTED>(p, objective_target_row<OBJ>(targets, row, D), D, vec_grad != 0, vec_grad != 0, grad_out + row * D, w, row_operand);
        }
    }
    if (loss_targets != nullptr) {   // (block-uniform; the block is one wave: one partial)
        double acc = 0.0;
        if constexpr (OBJ == kObjRmse) {
            if (live) {
                float y[DMAX];
                stream_load_row<DMAX>(loss_targets + row * D, D, vec_loss != 0, y);
                acc = staged_row_loss<DMAX>(p, y, D);
            }
        } else {
            if (live) acc = objective_loss_regs<OBJ, DMAX>(p, out + row * D, objective_target_row<OBJ>(loss_targets, row, D), D, vec_loss != 0, row_operand);
        }
        if constexpr (WEIGHTED) acc = obj_weighted_loss(w, acc);
        acc = staged_wave_sum(acc);
        if (lane == 0) loss_part[blockIdx.x] = acc;
    }
}

template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED>
bool launch_continue_codes(const ChainModel &cm, const PredictModel &pm, const CodeRows &cr, int m, int start_tree, int stop_tree, const float *base,
                           float *out, const float *targets, float *grad_out, const float *loss_targets, double *loss_part, const float *row_operand,
                           hipStream_t s) {
    static_assert(kStreamRows == kStagedRows, "a block of the streaming kernel writes exactly one loss partial");
    const size_t lds = stream_code_tile_bytes(cr.groups);
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_continue_codes<DMAX, GREEDY, OBJ, WEIGHTED>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_io = d4 && ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    // (softmax targets are one label per row: only grad_out's address counts, and the loss tail loads no vector)
    const int vec_grad = d4 && (((OBJ == kObjSoftmax ? 0 : reinterpret_cast<uintptr_t>(targets)) | reinterpret_cast<uintptr_t>(grad_out)) & 15) == 0;
    const int vec_loss = d4 && (reinterpret_cast<uintptr_t>(loss_targets) & 15) == 0;
    hipLaunchKernelGGL((k_continue_codes<DMAX, GREEDY, OBJ, WEIGHTED>), dim3((m + kStreamRows - 1) / kStreamRows), dim3(kStreamRows), lds, s, cm,
                       stream_owner<DMAX>(pm), pm.coef_cover, cr, m, start_tree, stop_tree, base, out, targets, grad_out, loss_targets, loss_part, vec_values,
                       vec_io, vec_grad, vec_loss, row_operand);
    return true;
}

}  // namespace

void tile_rows(const float *row, int D, int n, float *out, hipStream_t s) {
    const size_t n_el = static_cast<size_t>(n) * D;
    if (n_el == 0) return;
    hipLaunchKernelGGL(k_tile_rows, dim3(static_cast<unsigned>(std::min<size_t>((n_el + 255) / 256, 4096))), dim3(256), 0, s, row, D, n_el, out);
}

void predict_continue_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int start_tree, int stop_tree, const float *base,
                            float *out, const float *targets, float *grad_out, const float *loss_targets, double *loss_part, bool generic,
                            hipStream_t s, int objective, const float *weights, const float *alpha) {
    if (m <= 0) return;
    if (stop_tree <= start_tree || pm.n_opts <= 0) {   // no tree to apply, or no optimizer that owns an output: the base as it is
        const size_t n_el = static_cast<size_t>(m) * pm.D;
        if (out != base) (void)hipMemcpyAsync(out, base, sizeof(float) * n_el, hipMemcpyDeviceToDevice, s);
        if (objective != kObjRmse || weights != nullptr) {   // the stand-alone kernel of the objective: the tails' device functions on the matrix
            if (targets != nullptr) objective_rows(objective, out, targets, m, pm.D, grad_out, nullptr, s, weights, alpha);
            if (loss_targets != nullptr) objective_rows(objective, out, loss_targets, m, pm.D, nullptr, loss_part, s, weights, alpha);
            return;
        }
        if (targets != nullptr) {
            const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n_el + 255) / 256, 4096));
            hipLaunchKernelGGL(k_sub_rows, dim3(blocks), dim3(256), 0, s, out, targets, grad_out, n_el);
        }
        if (loss_targets != nullptr) loss_partials_of_predictions(out, loss_targets, m, pm.D, loss_part, s);
        return;
    }
    // the model view of the float walk with the threshold words replaced by bins (the packed conditions, the greedy node records, the general table)
    ChainModel cm = chain_model(pm);
    cm.walk.cond_pack = ct.cond_pack;
    cm.walk.grd_nodes = ct.grd_nodes;
    cm.walk.feature_bins = ct.bins;
    auto run = [&](auto obj, auto weighted) {
        constexpr int OBJ = decltype(obj)::value;
        constexpr bool WEIGHTED = decltype(weighted)::value;
        const float *const row_operand = OBJ == kObjQuantile ? alpha : weights;   // WEIGHTED: the weights [m]; kObjQuantile (never WEIGHTED): its level table [D]
        if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
                constexpr int DMAX = decltype(dmax)::value;
                return pm.oblivious ? launch_continue_codes<DMAX, false, OBJ, WEIGHTED>(cm, pm, cr, m, start_tree, stop_tree, base, out, targets, grad_out,
                                                                                        loss_targets, loss_part, row_operand, s)
                                    : launch_continue_codes<DMAX, true, OBJ, WEIGHTED>(cm, pm, cr, m, start_tree, stop_tree, base, out, targets, grad_out,
                                                                                       loss_targets, loss_part, row_operand, s);
            }))
            return;
        with_general_dmax(pm.D, [&](auto dmax) {
            hipLaunchKernelGGL((k_continue_codes_general<decltype(dmax)::value, OBJ, WEIGHTED>), dim3((m + 255) / 256), dim3(256), 0, s, cm, cr, m, start_tree,
                               stop_tree, base, out, targets, grad_out, loss_targets, loss_part, staged_loss_partials(m), row_operand);
        });
    };
    with_objective(objective, [&](auto obj) {
        if constexpr (decltype(obj)::value == kObjQuantile) run(obj, std::false_type{});   // (no weighted form: the caller has refused weights)
        else if (weights != nullptr) run(obj, std::true_type{});
        else run(obj, std::false_type{});
    });
}

}  // namespace kern
}  // namespace gbrl
