// predict_staged_codes.hip -- gfx950 kernels behind GBRL::predict_staged_prepared / GBRL::staged_loss_prepared: every prefix [0, stops[s]) of the
// ensemble evaluated in ONE walk over a prepared data set's bin codes.  It joins predict_staged.hip's checkpointed chain with
// predict_continue_codes.hip's code tile, objective tails and weights.  Stage s has, bit for bit, what kern::predict_continue_codes(base = tiled
// bias, 0, stops[s]) leaves in `out`, and its loss partial is what that call's loss tail writes: the row loss (predict_loss.h), the weight in front
// of the butterfly, the butterfly over the same 64 positions, k_staged_finish's fixed-order sum.  stops[s] == 0 is the bias alone.
//
//   k_staged_codes          lane = row, one wave per block.  The block's 64 rows are staged ONCE from the group-major records [G][N][16] u16 into
//                           the LDS tile at the odd word stride (stream_stage_code_tile; with `rows` lane j stages the records of rows[row0 + j]),
//                           the D <= 64 outputs of a row live in registers, trees are walked in groups of kG that end at the next checkpoint and
//                           never straddle it (stream_chain_group on the code row).  At a checkpoint
//                             predict mode  stores the lane's outputs to stage s (16-byte stores where D and the address allow);
//                             loss mode     forms the objective's row loss of the current p[] (times (double)w when weighted), reduces the wave's 64
//                                           values by the shared butterfly, lane 0 writes part[s][block];
//                             metric mode   also ballots the wrong rows (softmax) or cells (logistic) and lane 0 writes the popcount to
//                                           cnt[s][c][block], c = 0 (softmax) or the output (logistic): metric_core.h's integers.
//                           Targets and the weight are loaded once per row and held in registers next to the chain: D floats, or one label for
//                           softmax.  softmax_row_loss and the arg-max read p[] and never write it: the chain is not disturbed.
//                           Traffic: the codes are read once, 32 G bytes per row; partials are 8 bytes per stage and 64 rows (written, then read by
//                           the finishing launch); predict mode stores 4 D bytes per row and stage.
//   k_staged_codes_general  one thread per row, the records read in place, k_continue_codes_general's walk suspended at each checkpoint: D in
//                           65..128, optimizers that share outputs, a greedy depth-0 tree, rows too wide for the tile, a refused LDS opt-in, and the
//                           cross-check behind GBRL_HIP_STAGED_GENERIC=1.  Targets are re-read per checkpoint.  At its widest width (128) the
//                           logistic and quantile row losses are the rolled loops of predict_loss.h over the row as the lane has stored it: the
//                           lane stores p[] to row_scratch[j] at each checkpoint and sums from there.  A wave still covers 64 consecutive positions
//                           and reduces them with the same butterfly, so both kernels write the same partials and the same counts.
//   finishing launches      kern::staged_loss_finish_rows (k_staged_finish, one block per stage) for the float64 partials; k_staged_count_finish,
//                           an integer sum, one block per (stage, counter).  No atomics: two calls return identical bytes.
//
// Register budget (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; a one-wave block may use 512 VGPRs).  The widest streaming
// forms hold chain, targets and temporaries at once; at DMAX = 64 (oblivious / greedy; VGPRs + AGPRs, scratch bytes per lane):
//   predict 142 / 143, 0     rmse loss 211 / 212, 0 (weighted 212 / 213)     softmax loss 181 / 182, 0 (weighted 183 / 184; metric 183 / 183)
//   logistic loss 256 + 50 / 256 + 52, 0 (weighted + 52 / + 54; metric + 58 / + 58)     quantile loss 256 + 18 / 256 + 20, 0
// None of the 131 instantiations of this unit uses scratch (the general kernel at DMAX = 128 included: 161 .. 256 + 2), so the streaming kernel
// keeps every (OBJ, D <= 64) and nothing is routed to the general kernel for register reasons.  The logistic and quantile forms at DMAX = 64 run
// at one wave per SIMD; the narrower widths (the common case) at two to eight.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"
#include "predict_loss.h"
#include "metric_core.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kModePredict = 0, kModeLoss = 1, kModeMetric = 2;

// what a checkpoint emits
struct StagedCodesIo {
    const int32_t *stops;      // [n_stops] strictly ascending tree counts
    int n_stops;
    int walk;                  // 0: no optimizer owns an output -- every stage is the bias, no tree is visited
    float *out;                // predict mode: [n_stops][m][D]
    const float *targets;      // loss modes: [m][D] float32, or int32 [m] behind the pointer (softmax)
    const float *row_operand;  // WEIGHTED: the weights [m]; kObjQuantile (never WEIGHTED): its level table [D]
    double *part;              // [n_stops][nb], nb = ceil(m / 64)
    unsigned long long *cnt;   // metric mode: [n_stops][C][nb], C = 1 (softmax) or D (logistic)
    float *row_scratch;        // general kernel at DMAX = 128, logistic / quantile: [m][D]
    int nb, C;
};

// the instantiations of the general kernel that sum their row loss from the row as the lane has stored it (objective_loss_regs' rolled loops at
// its widest width): the ONE condition behind the kernel's store and behind staged_codes_row_scratch, the size the caller allocates
template <int DMAX, int OBJ>
constexpr bool kStoredRowLoss = DMAX > 64 && (OBJ == kObjLogistic || OBJ == kObjQuantile);

// metric_argmax on a register row: the lowest index among the maxima, a NaN never above the running maximum
template <int DMAX>
__device__ __forceinline__ int staged_argmax(const float (&p)[DMAX], int D) {
    int best = 0;
    float m = p[0];
#pragma unroll
    for (int c = 1; c < DMAX; ++c)
        if (c < D && p[c] > m) { m = p[c]; best = c; }
    return best;
}

// one lane's popcount of the wave's flags (whole waves only)
__device__ __forceinline__ unsigned long long staged_wrong(bool flag) { return static_cast<unsigned long long>(__popcll(__ballot(flag))); }

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX, int OBJ, bool WEIGHTED, int MODE>
__global__ __launch_bounds__(256) void k_staged_codes_general(ChainModel cm, StagedCodesIo io, CodeRows cr, int m) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < m;
    if (MODE == kModePredict && !live) return;   // (with a loss tail whole waves stay for the butterfly and the ballots)
    const int D = cm.D;
    float p[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) p[d] = d < D ? cm.bias[d] : 0.0f;
    float w = 1.0f;
    if constexpr (WEIGHTED) w = live ? io.row_operand[j] : 0.0f;
    const size_t src = live ? static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j) : 0;
    const GeneralCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const size_t at = live ? static_cast<size_t>(j) : 0;   // (a thread without a row names row 0: read, never counted)
    const int wave = j / kStagedRows;   // 256 = 4 x 64: a wave holds the positions of one partial
    const bool writer = (threadIdx.x & (kStagedRows - 1)) == 0 && wave < io.nb;
    int t = 0;
    bool ended = false;   // a greedy search ran off the ensemble: every later stage is the walk as it stands
    for (int s = 0; s < io.n_stops; ++s) {   // (uniform over the block)
        const int stop = io.walk ? io.stops[s] : 0;
        if (live)
            for (; t < stop && !ended; ++t)
                if (!general_chain_tree<DMAX>(cm, r, t, p)) ended = true;
        if constexpr (MODE == kModePredict) {
            stream_store_row<DMAX>(io.out + (static_cast<size_t>(s) * m + j) * D, D, false, p);
        } else {
            const float *y_row = objective_target_row<OBJ>(io.targets, at, D);
            double acc = 0.0;
            if constexpr (OBJ == kObjRmse) {
                if (live) acc = staged_row_loss<DMAX>(p, y_row, D);
            } else {
                float *p_row = nullptr;
                if constexpr (kStoredRowLoss<DMAX, OBJ>) {
                    p_row = io.row_scratch + at * D;
                    if (live) stream_store_row<DMAX>(p_row, D, false, p);
                }
                if (live) acc = objective_loss_regs<OBJ, DMAX>(p, p_row, y_row, D, false, io.row_operand);
            }
            if constexpr (WEIGHTED) acc = obj_weighted_loss(w, acc);
            acc = staged_wave_sum(acc);
            if (writer) io.part[static_cast<size_t>(s) * io.nb + wave] = acc;
            if constexpr (MODE == kModeMetric && OBJ == kObjSoftmax) {
                const unsigned long long c = staged_wrong(live && staged_argmax<DMAX>(p, D) != *reinterpret_cast<const int32_t *>(y_row));
                if (writer) io.cnt[static_cast<size_t>(s) * io.nb + wave] = c;
            } else if constexpr (MODE == kModeMetric) {
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                    if (d < D) {   // (uniform)
                        const unsigned long long c = staged_wrong(live && metric_logistic_wrong(p[d], y_row[d]));
                        if (writer) io.cnt[(static_cast<size_t>(s) * io.C + d) * io.nb + wave] = c;
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED, int MODE>
__global__ __launch_bounds__(kStreamRows) void k_staged_codes(ChainModel cm, StagedCodesIo io, StreamOwner<DMAX> own, uint64_t cover, CodeRows cr, int m,
                                                              int vec_values, int vec_io) {
    extern __shared__ __align__(16) uint32_t sctile[];   // [kStreamRows][stream_code_stride(G)]
    const int lane = threadIdx.x;
    const int D = cm.D;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, m - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    float p[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) p[d] = d < D ? cm.bias[d] : 0.0f;   // (wave-uniform addresses: the scalar cache)
    // the loss modes: the row's targets (D floats, or one label) and its weight, loaded once, in flight together with the tile
    constexpr bool kRowTargets = MODE != kModePredict && OBJ != kObjSoftmax;
    float y[kRowTargets ? DMAX : 1];
    int label = 0;
    float w = 1.0f;
    if constexpr (kRowTargets) {
        if (live) {
            stream_load_row<DMAX>(io.targets + row * D, D, vec_io != 0, y);
        } else {
#pragma unroll
            for (int d = 0; d < DMAX; ++d) y[d] = 0.0f;
        }
    } else {
        y[0] = 0.0f;
        if constexpr (MODE != kModePredict) label = live ? reinterpret_cast<const int32_t *>(io.targets)[row] : 0;
    }
    if constexpr (WEIGHTED) w = live ? io.row_operand[row] : 0.0f;
    const int at = cr.row0 + r0 + (live ? lane : 0);   // (a lane without a row names the block's first: a valid record, never counted)
    const int my_row = cr.rows ? cr.rows[at] : at;
    stream_stage_code_tile(sctile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
    __syncthreads();
    const StreamCodeRow x{reinterpret_cast<const uint16_t *>(sctile + (live ? lane : 0) * stream_code_stride(cr.groups))};
    int start_tree = 0;
    for (int s = 0; s < io.n_stops; ++s) {   // (wave-uniform)
        const int stop_tree = io.walk ? io.stops[s] : 0;
        if (live)
            for (int t0 = start_tree; t0 < stop_tree; t0 += kStreamGroup<DMAX>)   // a group ends at the checkpoint
                stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, static_cast<const int32_t *>(nullptr), t0, stop_tree, vec_values, p);
        start_tree = max(start_tree, stop_tree);
        if constexpr (MODE == kModePredict) {
            if (live) stream_store_row<DMAX>(io.out + (static_cast<size_t>(s) * m + row) * D, D, vec_io != 0, p);
        } else {
            double acc = 0.0;
            if (live) {
                if constexpr (OBJ == kObjRmse) acc = staged_row_loss<DMAX>(p, y, D);
                else if constexpr (OBJ == kObjSoftmax) acc = softmax_row_loss<DMAX>(p, label, D);
                else acc = objective_loss_regs<OBJ, DMAX>(p, nullptr, y, D, false, io.row_operand);   // (the targets from the registers, entry by entry)
            }
            if constexpr (WEIGHTED) acc = obj_weighted_loss(w, acc);
            acc = staged_wave_sum(acc);
            if (lane == 0) io.part[static_cast<size_t>(s) * io.nb + blockIdx.x] = acc;
            if constexpr (MODE == kModeMetric && OBJ == kObjSoftmax) {
                const unsigned long long c = staged_wrong(live && staged_argmax<DMAX>(p, D) != label);
                if (lane == 0) io.cnt[static_cast<size_t>(s) * io.nb + blockIdx.x] = c;
            } else if constexpr (MODE == kModeMetric) {
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                    if (d < D) {   // (wave-uniform)
                        const unsigned long long c = staged_wrong(live && metric_logistic_wrong(p[d], y[d]));
                        if (lane == 0) io.cnt[(static_cast<size_t>(s) * io.C + d) * io.nb + blockIdx.x] = c;
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ finishing kernel of the counts
constexpr int kCountFinishThreads = 256;
__global__ __launch_bounds__(kCountFinishThreads) void k_staged_count_finish(const unsigned long long *__restrict__ cnt, int nb, unsigned long long *__restrict__ counts) {
    __shared__ unsigned long long sh[kCountFinishThreads];
    const unsigned long long *cs = cnt + static_cast<size_t>(blockIdx.x) * nb;
    unsigned long long acc = 0ull;
    for (int i = threadIdx.x; i < nb; i += kCountFinishThreads) acc += cs[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kCountFinishThreads / 2; w >= 1; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = sh[0];
}

template <int DMAX, bool GREEDY, int OBJ, bool WEIGHTED, int MODE>
bool launch_staged_codes(const ChainModel &cm, const StagedCodesIo &io, const PredictModel &pm, const CodeRows &cr, int m, hipStream_t s) {
    static_assert(kStreamRows == kStagedRows, "a block of the streaming kernel writes exactly one loss partial");
    const size_t lds = stream_code_tile_bytes(cr.groups);
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_staged_codes<DMAX, GREEDY, OBJ, WEIGHTED, MODE>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    // (softmax targets are one label per row: no vector is loaded)
    const void *io_ptr = MODE == kModePredict ? static_cast<const void *>(io.out) : static_cast<const void *>(io.targets);
    const int vec_io = d4 && (MODE == kModePredict || OBJ != kObjSoftmax) && (reinterpret_cast<uintptr_t>(io_ptr) & 15) == 0;
    hipLaunchKernelGGL((k_staged_codes<DMAX, GREEDY, OBJ, WEIGHTED, MODE>), dim3((m + kStreamRows - 1) / kStreamRows), dim3(kStreamRows), lds, s, cm, io,
                       stream_owner<DMAX>(pm), pm.coef_cover, cr, m, vec_values, vec_io);
    return true;
}

template <int OBJ, bool WEIGHTED, int MODE>
void staged_codes_dispatch(const ChainModel &cm, const StagedCodesIo &io, const PredictModel &pm, const CodeRows &cr, int m, bool generic, hipStream_t s) {
    if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_staged_codes<DMAX, false, OBJ, WEIGHTED, MODE>(cm, io, pm, cr, m, s)
                                : launch_staged_codes<DMAX, true, OBJ, WEIGHTED, MODE>(cm, io, pm, cr, m, s);
        }))
        return;
    with_general_dmax(pm.D, [&](auto dmax) {
        hipLaunchKernelGGL((k_staged_codes_general<decltype(dmax)::value, OBJ, WEIGHTED, MODE>), dim3((m + 255) / 256), dim3(256), 0, s, cm, io, cr, m);
    });
}

}  // namespace

size_t staged_codes_row_scratch(int m, int D, int objective) {
    const bool stored = with_general_dmax(D, [&](auto dmax) {
        return with_objective(objective, [&](auto obj) { return kStoredRowLoss<decltype(dmax)::value, decltype(obj)::value>; });
    });
    return stored ? static_cast<size_t>(m) * D : 0;
}

void predict_staged_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, const StagedStops &st, const StagedCodesOut &o, int objective,
                          bool generic, hipStream_t s) {
    if (m <= 0) return;
    // the model view of the float walk with the threshold words replaced by bins (kern::predict_continue_codes)
    ChainModel cm = chain_model(pm);
    cm.walk.cond_pack = ct.cond_pack;
    cm.walk.grd_nodes = ct.grd_nodes;
    cm.walk.feature_bins = ct.bins;
    StagedCodesIo io{};
    io.stops = st.stops; io.n_stops = st.n_stops;
    io.walk = (pm.n_opts > 0 && pm.n_trees > 0 && st.last_stop > 0) ? 1 : 0;   // as kern::predict_continue_codes: no optimizer, no tree to apply
    io.out = o.out; io.targets = o.targets; io.part = o.part; io.cnt = o.cnt_part; io.row_scratch = o.row_scratch;
    io.nb = staged_loss_partials(m);
    io.C = metric_count_columns(objective == kObjSoftmax, pm.D);
    if (o.out != nullptr) {
        staged_codes_dispatch<kObjRmse, false, kModePredict>(cm, io, pm, cr, m, generic, s);
        return;
    }
    with_objective(objective, [&](auto obj) {
        constexpr int OBJ = decltype(obj)::value;
        io.row_operand = OBJ == kObjQuantile ? o.alpha : o.weights;
        if constexpr (OBJ == kObjLogistic || OBJ == kObjSoftmax) {
            if (o.counts != nullptr) {   // (never weighted: the caller has refused weights with a metric)
                staged_codes_dispatch<OBJ, false, kModeMetric>(cm, io, pm, cr, m, generic, s);
                return;
            }
        }
        if constexpr (OBJ != kObjQuantile) {   // (quantile has no weighted form: the caller has refused weights)
            if (o.weights != nullptr) {
                staged_codes_dispatch<OBJ, true, kModeLoss>(cm, io, pm, cr, m, generic, s);
                return;
            }
        }
        staged_codes_dispatch<OBJ, false, kModeLoss>(cm, io, pm, cr, m, generic, s);
    });
    staged_loss_finish_rows(o.part, io.nb, st.n_stops, o.sums, s);
    if (o.counts != nullptr) hipLaunchKernelGGL(k_staged_count_finish, dim3(st.n_stops * io.C), dim3(kCountFinishThreads), 0, s, o.cnt_part, io.nb, o.counts);
}

}  // namespace kern
}  // namespace gbrl
