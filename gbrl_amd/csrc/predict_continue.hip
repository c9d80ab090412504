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
//                       that share outputs, D <= 128, rows too wide for an LDS tile or a device that refuses the LDS opt-in.  Also the
//                       cross-check behind GBRL_HIP_CONTINUE_GENERIC=1.
//
// This file keeps what is particular to the call: the base load and the rule for a range that applies nothing.  The model view, both walks,
// the group body (stream_chain_group), the tile staging, the row load and store, the family choice and the LDS opt-in are
// predict_rowwalk.h's, shared with predict_staged.hip, predict_leaves.hip and refit.hip.
// rate(t, o): PredictModel::rate[t * n_opts + o] for an ensemble with a Linear schedule (absolute tree index), opt_lr[o] otherwise (chain_rates).
// `base` and `out` may be the same buffer: a thread reads and writes its own row only.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX>
__global__ __launch_bounds__(256) void k_continue_general(ChainModel cm, const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes,
                                                          int Fc, int n, int start_tree, int stop_tree, const float *base, float *out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const int D = cm.D;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? base[static_cast<size_t>(row) * D + j] : 0.0f;
    const GeneralRow r{obs + static_cast<size_t>(row) * F, cat_codes ? cat_codes + static_cast<size_t>(row) * Fc : nullptr};
    for (int t = start_tree; t < stop_tree; ++t)
        if (!general_chain_tree<DMAX>(cm, r, t, p)) break;   // a greedy search ran off the ensemble: the walk ends
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < D) out[static_cast<size_t>(row) * D + j] = p[j];
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY>
__global__ __launch_bounds__(kStreamRows) void k_continue(ChainModel cm, StreamOwner<DMAX> own, uint64_t cover, const float *__restrict__ obs, int F,
                                                          const int32_t *__restrict__ cat_codes, int Fc, int n, int start_tree, int stop_tree,
                                                          const float *base, float *out, int vec_values, int vec_io) {
    extern __shared__ float ctile[];   // [kStreamRows][F | 1]
    const int lane = threadIdx.x;
    const int xs = F | 1;
    const int D = cm.D;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, n - r0);
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
        for (int t0 = start_tree; t0 < stop_tree; t0 += kStreamGroup<DMAX>)
            stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, xc, t0, stop_tree, vec_values, p);
        stream_store_row<DMAX>(out + row * D, D, vec_io != 0, p);
    }
}

template <int DMAX, bool GREEDY>
bool launch_continue(const ChainModel &cm, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                     int stop_tree, const float *base, float *out, hipStream_t s) {
    const size_t lds = stream_tile_bytes(F);
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_continue<DMAX, GREEDY>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_io = d4 && ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL((k_continue<DMAX, GREEDY>), dim3((n + kStreamRows - 1) / kStreamRows), dim3(kStreamRows), lds, s, cm, stream_owner<DMAX>(pm),
                       pm.coef_cover, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, vec_values, vec_io);
    return true;
}

}  // namespace

void predict_continue(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                      const float *base, float *out, bool generic, hipStream_t s) {
    if (stop_tree <= start_tree || pm.n_opts <= 0) {   // no tree to apply, or no optimizer that owns an output: the base as it is
        if (out != base) (void)hipMemcpyAsync(out, base, sizeof(float) * static_cast<size_t>(n) * pm.D, hipMemcpyDeviceToDevice, s);
        return;
    }
    const ChainModel cm = chain_model(pm);
    if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_continue<DMAX, false>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s)
                                : launch_continue<DMAX, true>(cm, pm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, base, out, s);
        }))
        return;
    with_general_dmax(pm.D, [&](auto dmax) {
        hipLaunchKernelGGL((k_continue_general<decltype(dmax)::value>), dim3((n + 255) / 256), dim3(256), 0, s, cm, obs, F, cat_codes, Fc, n, start_tree,
                           stop_tree, base, out);
    });
}

}  // namespace kern
}  // namespace gbrl
