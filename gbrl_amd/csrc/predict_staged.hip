// predict_staged.hip -- gfx950 kernels behind GBRL::predict_staged / GBRL::staged_loss: every prefix [0, stops[s]) of the ensemble evaluated in
// ONE walk.  Per (row, output) a prediction is one chain in tree order, p = fma(-rate(t, optimizer of the output), value(leaf(row, t)), p)
// started from the bias (predict_continue.hip); a staged evaluation is that chain with checkpoints.  Stage s has, bit for bit, what
// kern::predict_continue(base = tiled bias, 0, stops[s]) returns: rates at the absolute tree index, an output that no optimizer owns keeps the
// bias bits, and the walk is never split over tree ranges.  stops[s] == 0 is the bias alone (0 never means "all trees" here).
//
//   k_staged          k_continue's layout: lane = row, one wave per block, the block's 64 rows in LDS at stride F | 1, the outputs of a row in
//                     registers, trees in groups of kG whose leaf values are in flight together.  A group ends at the next checkpoint and never
//                     straddles it.  At a checkpoint, predict mode stores the lane's D outputs to stage s (16-byte stores where D and the
//                     addresses allow); loss mode forms the row's sum_j (double)g_j^2, g_j = fl32(p_j - y_j), reduces the wave's 64 values by
//                     a fixed butterfly and lane 0 writes part[s][block].  The targets of a row are loaded once and held in registers next to
//                     the chain (D <= 64: at most 64 more VGPRs of the 512 a one-wave block may use); re-reading them per checkpoint would
//                     cost 4 D bytes per row and stage, more than the observation tile from a few dozen stages on.  The rows are read once:
//                     predict mode moves n (4 F + 4 D stages) bytes, loss mode n (4 F + 4 D) + 16 stages n / 64 (the partials written, then read).
//                     The group body, the tile staging and the row load and store are k_continue's own (predict_rowwalk.h).
//                     Every output owned by at most one optimizer, D <= 64, a row tile that fits in LDS.
//   k_staged_general  anything the file format can hold: one thread per row, k_continue_general's walk (predict_rowwalk.h; greedy: leaf by leaf,
//                     Q7) suspended at each checkpoint, so that stage s is the walk over [0, stops[s]) and not a restart, optimizers that share
//                     outputs, D <= 128, rows too wide for an LDS tile.  The targets are re-read per checkpoint.  A wave still covers 64
//                     consecutive rows and reduces them with the same butterfly, so both kernels write the same part[][] and staged_loss has
//                     the same bytes through either.  Also the cross-check behind GBRL_HIP_STAGED_GENERIC=1.
//   k_staged_finish   one block per stage: part[s][0 .. nb) summed in a fixed order (a strided serial sum per thread, then a fixed LDS tree).
//                     No floating-point atomics anywhere: two identical calls return identical bytes.
// This file keeps the checkpoints, k_staged_finish and k_loss_of_predictions (the row sum and the butterfly are predict_loss.h's); the model view, both walks, the family
// choice and the LDS opt-in are predict_rowwalk.h's, shared with predict_continue.hip, predict_leaves.hip and refit.hip.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"
#include "predict_loss.h"

namespace gbrl {
namespace kern {

namespace {

// what a checkpoint emits: predict mode (out != nullptr) or loss mode (targets, part)
struct StagedIo {
    const int32_t *stops;   // [n_stops] strictly ascending tree counts
    int n_stops;
    int walk;               // 0: no optimizer owns an output -- every stage is the bias, no tree is visited
    float *out;             // [n_stops][n][D]
    const float *targets;   // [n][D]
    double *part;           // [n_stops][nb], nb = ceil(n / 64)
    int nb;
};

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX, bool LOSS>
__global__ __launch_bounds__(256) void k_staged_general(ChainModel cm, StagedIo io, const float *__restrict__ obs, int F,
                                                        const int32_t *__restrict__ cat_codes, int Fc, int n) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = row < static_cast<size_t>(n);
    const int D = cm.D;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? cm.bias[j] : 0.0f;
    const GeneralRow r{obs + (live ? row : 0) * F, cat_codes ? cat_codes + (live ? row : 0) * Fc : nullptr};
    int t = 0;
    bool ended = false;   // a greedy search ran off the ensemble: every later stage is the walk as it stands
    for (int s = 0; s < io.n_stops; ++s) {   // (uniform over the block)
        const int stop = io.walk ? io.stops[s] : 0;
        if (live)
            for (; t < stop && !ended; ++t)
                if (!general_chain_tree<DMAX>(cm, r, t, p)) ended = true;
        if constexpr (!LOSS) {
            if (live) {
                float *o = io.out + (static_cast<size_t>(s) * n + row) * D;
#pragma unroll
                for (int j = 0; j < DMAX; ++j)
                    if (j < D) o[j] = p[j];
            }
        } else {
            double acc = 0.0;
            if (live) acc = staged_row_loss<DMAX>(p, io.targets + row * D, D);   // (the targets are re-read per checkpoint)
            acc = staged_wave_sum(acc);
            const size_t wave = row / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
            if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < static_cast<size_t>(io.nb)) io.part[static_cast<size_t>(s) * io.nb + wave] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, bool LOSS>
__global__ __launch_bounds__(kStagedRows) void k_staged(ChainModel cm, StagedIo io, StreamOwner<DMAX> own, uint64_t cover, const float *__restrict__ obs,
                                                        int F, const int32_t *__restrict__ cat_codes, int Fc, int n, int vec_values, int vec_io) {
    extern __shared__ float stile[];   // [kStagedRows][F | 1]
    const int lane = threadIdx.x;
    const int xs = F | 1;
    const int D = cm.D;
    const int r0 = blockIdx.x * kStagedRows;
    const int rows = min(kStagedRows, n - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? cm.bias[j] : 0.0f;   // (wave-uniform addresses: the scalar cache)
    float y[DMAX];   // loss mode: the row's targets, in flight together with the tile
    if constexpr (LOSS) {
        if (live) {
            stream_load_row<DMAX>(io.targets + row * D, D, vec_io != 0, y);
        } else {
#pragma unroll
            for (int j = 0; j < DMAX; ++j) y[j] = 0.0f;
        }
    }
    stream_stage_tile(stile, obs, F, r0, rows, lane);
    __syncthreads();
    const float *x = stile + (live ? lane : 0) * xs;
    const int32_t *xc = cat_codes ? cat_codes + (live ? row : 0) * Fc : nullptr;
    int start_tree = 0;
    for (int s = 0; s < io.n_stops; ++s) {   // (wave-uniform)
        const int stop_tree = io.walk ? io.stops[s] : 0;
        if (live)
            for (int t0 = start_tree; t0 < stop_tree; t0 += kStreamGroup<DMAX>)   // a group ends at the checkpoint
                stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, xc, t0, stop_tree, vec_values, p);
        start_tree = max(start_tree, stop_tree);
        if constexpr (!LOSS) {
            if (live) stream_store_row<DMAX>(io.out + (static_cast<size_t>(s) * n + row) * D, D, vec_io != 0, p);
        } else {
            double acc = 0.0;
            if (live) acc = staged_row_loss<DMAX>(p, y, D);
            acc = staged_wave_sum(acc);
            if (lane == 0) io.part[static_cast<size_t>(s) * io.nb + blockIdx.x] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ finishing kernel
constexpr int kFinishThreads = 256;
__global__ __launch_bounds__(kFinishThreads) void k_staged_finish(const double *__restrict__ part, int nb, double *__restrict__ sums) {
    __shared__ double sh[kFinishThreads];
    const double *ps = part + static_cast<size_t>(blockIdx.x) * nb;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += kFinishThreads) acc += ps[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kFinishThreads / 2; w >= 1; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

// the loss checkpoint of k_staged_general on predictions that already exist (kern::staged_loss_of_predictions): the same row sum, the same
// butterfly over the same 64 rows, the same part[] entry
__global__ __launch_bounds__(256) void k_loss_of_predictions(const float *__restrict__ preds, const float *__restrict__ targets, int n, int D,
                                                             double *__restrict__ part, int nb) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    double acc = 0.0;
    if (row < static_cast<size_t>(n)) {
        const float *p = preds + row * D, *y = targets + row * D;
        for (int j = 0; j < D; ++j) {
            const double g = static_cast<double>(__fsub_rn(p[j], y[j]));
            acc = fma(g, g, acc);
        }
    }
    acc = staged_wave_sum(acc);
    const size_t wave = row / kStagedRows;
    if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < static_cast<size_t>(nb)) part[wave] = acc;
}

template <int DMAX, bool GREEDY, bool LOSS>
bool launch_staged(const ChainModel &cm, const StagedIo &io, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n,
                   hipStream_t s) {
    const size_t lds = stream_tile_bytes(F);
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_staged<DMAX, GREEDY, LOSS>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_io = d4 && (reinterpret_cast<uintptr_t>(LOSS ? static_cast<const void *>(io.targets) : static_cast<const void *>(io.out)) & 15) == 0;
    hipLaunchKernelGGL((k_staged<DMAX, GREEDY, LOSS>), dim3((n + kStagedRows - 1) / kStagedRows), dim3(kStagedRows), lds, s, cm, io,
                       stream_owner<DMAX>(pm), pm.coef_cover, obs, F, cat_codes, Fc, n, vec_values, vec_io);
    return true;
}

template <bool LOSS>
void staged_dispatch(const ChainModel &cm, const StagedIo &io, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n,
                     bool generic, hipStream_t s) {
    if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_staged<DMAX, false, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s)
                                : launch_staged<DMAX, true, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s);
        }))
        return;
    with_general_dmax(pm.D, [&](auto dmax) {
        hipLaunchKernelGGL((k_staged_general<decltype(dmax)::value, LOSS>), dim3((n + 255) / 256), dim3(256), 0, s, cm, io, obs, F, cat_codes, Fc, n);
    });
}

}  // namespace

int staged_loss_partials(int n) { return (n + kStagedRows - 1) / kStagedRows; }

void loss_partials_of_predictions(const float *preds, const float *targets, int n, int D, double *part, hipStream_t s) {
    hipLaunchKernelGGL(k_loss_of_predictions, dim3((n + 255) / 256), dim3(256), 0, s, preds, targets, n, D, part, staged_loss_partials(n));
}

void staged_loss_finish(const double *part, int nb, double *sum, hipStream_t s) {
    hipLaunchKernelGGL(k_staged_finish, dim3(1), dim3(kFinishThreads), 0, s, part, nb, sum);
}

void staged_loss_finish_rows(const double *part, int nb, int n_rows, double *sums, hipStream_t s) {
    hipLaunchKernelGGL(k_staged_finish, dim3(n_rows), dim3(kFinishThreads), 0, s, part, nb, sums);
}

void staged_loss_of_predictions(const float *preds, const float *targets, int n, int D, double *part, double *sum, hipStream_t s) {
    loss_partials_of_predictions(preds, targets, n, D, part, s);
    staged_loss_finish(part, staged_loss_partials(n), sum, s);
}

void predict_staged(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, const StagedStops &st, float *out,
                    const float *targets, double *part, double *sums, bool generic, hipStream_t s) {
    const ChainModel cm = chain_model(pm);
    StagedIo io{};
    io.stops = st.stops; io.n_stops = st.n_stops;
    io.walk = (pm.n_opts > 0 && pm.n_trees > 0 && st.last_stop > 0) ? 1 : 0;   // as kern::predict_continue: no optimizer, no tree to apply
    io.out = out; io.targets = targets; io.part = part; io.nb = staged_loss_partials(n);
    if (targets == nullptr) {
        staged_dispatch<false>(cm, io, pm, obs, F, cat_codes, Fc, n, generic, s);
    } else {
        staged_dispatch<true>(cm, io, pm, obs, F, cat_codes, Fc, n, generic, s);
        hipLaunchKernelGGL(k_staged_finish, dim3(st.n_stops), dim3(kFinishThreads), 0, s, part, io.nb, sums);
    }
}

}  // namespace kern
}  // namespace gbrl
