// refit.hip -- gfx950 kernels behind GBRL::refit_leaves: the leaf values of the trees [start, stop) fitted again on a batch, the structure kept.
// The running prediction P [n][D] lives on the device for the whole range; per tree the host enqueues three launches and never waits:
//
//   accumulate   routes every row through tree t (the walks of predict_rowwalk.h, so a leaf gets exactly the rows predict_leaves reports),
//                stores the row's global leaf to leaf_idx[n] and adds q = llrint((double)fl32(P - y) * 2^lbits) per output, and 1, to the leaf's
//                int64 accumulators.  2^lbits comes from gmax[t], the bits of max |g| the previous apply pass left on the device, through
//                leaf_sum_bits_dev -- the step's own rule.  The accumulators are leaf_accum.h's, in both of its schemes:
//     k_refit_accum<DMAX, GREEDY>   streaming, in k_continue / k_leaf_counts' layout (64 rows in LDS at stride F | 1), W = D + 1.
//     k_refit_accum_general         general, rows from global memory.  Rows too wide for LDS, greedy ensembles without node records, more than
//                64 outputs, trees whose accumulators do not fit behind the tile, GBRL_HIP_REFIT_GENERIC=1.
//   finalize     k_refit_finalize: new value per (leaf, output) from the sums, the count, the old value and decay, into new_values.
//   apply        k_refit_apply: P = fma(-rate, new value, P) through leaf_idx (the rows X are not read again), then max |fl32(P - y)| of the
//                next tree (behind the last tree: of the final prediction) by an integer atomicMax on the float bits (a maximum is
//                order-free; NaN is carried as +inf).
//
// The accumulators of the whole range are zeroed once by the caller, so no pass clears them.  pm.values is only read: the result goes to
// new_values, and the caller writes the model after it has seen every gmax finite.  The model view, both walks, the rate rule of the apply
// pass (ChainRates), the tile staging, the row load, the LDS opt-in and the template-width ladder are predict_rowwalk.h's, shared with
// predict_continue.hip, predict_staged.hip and predict_leaves.hip.
#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kRefitRows = kStreamRows;   // rows per block of the streaming kernel = one wave
constexpr int kRefitBlocksPerCu = 4;      // one-wave blocks per CU: every block flushes leaves x (D + 1) global atomics once

struct RefitTree : TreeSpan {
    const uint32_t *gmax;            // bits of max |g| before this tree
    uint32_t *gmax_next;             // where the apply pass leaves the next tree's (behind the last tree: max |g| of the final prediction)
    unsigned long long *acc;         // [n_leaves][D + 1]
    float *new_values;               // [n_leaves][D]
};

// bits of |g| as an unsigned integer: ordered like the magnitudes; NaN is carried as +inf
__device__ __forceinline__ uint32_t refit_abs_bits(float g) {
    const uint32_t u = __float_as_uint(g) & 0x7fffffffu;
    return u > 0x7f800000u ? 0x7f800000u : u;
}
__device__ __forceinline__ double refit_scale(int n, const uint32_t *gmax) {
    return ldexp(1.0, leaf_sum_bits_dev(static_cast<long long>(n), __uint_as_float(*gmax)));
}
__device__ __forceinline__ long long refit_quantise(float g, double scale) { return __double2ll_rn(__dmul_rn(static_cast<double>(g), scale)); }
// maximum over the block, then one atomic per block
__device__ __forceinline__ void refit_block_max(uint32_t m, uint32_t *dst) {
    __shared__ uint32_t sh[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), off, kWave)));
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < static_cast<int>(blockDim.x) / kWave; ++w) m = max(m, sh[w]);
        if (m) atomicMax(dst, m);
    }
}

// ------------------------------------------------------------------------------------------------------------ start of the run
__global__ __launch_bounds__(256) void k_refit_tile_bias(const float *__restrict__ bias, int D, size_t total, float *__restrict__ P) {
    for (size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<size_t>(gridDim.x) * blockDim.x)
        P[e] = bias[e % D];
}
__global__ __launch_bounds__(256) void k_refit_gmax(const float *__restrict__ P, const float *__restrict__ Y, size_t total, uint32_t *__restrict__ gmax) {
    uint32_t m = 0;
    for (size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<size_t>(gridDim.x) * blockDim.x)
        m = max(m, refit_abs_bits(__fsub_rn(P[e], Y[e])));
    refit_block_max(m, gmax);
}

// ------------------------------------------------------------------------------------------------------------ accumulate
__global__ __launch_bounds__(256) void k_refit_accum_general(LeavesModel cm, RefitTree rt, const float *__restrict__ obs, int F,
                                                             const int32_t *__restrict__ cat_codes, int Fc, int n, int D, const float *__restrict__ P,
                                                             const float *__restrict__ Y, int32_t *__restrict__ leaf_idx) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = row < static_cast<size_t>(n);   // (dead lanes stay for the ballots)
    const size_t rr = live ? row : 0;
    const GeneralRow r{obs + rr * F, cat_codes ? cat_codes + rr * Fc : nullptr};
    const int lane = threadIdx.x & (kWave - 1);
    const double scale = refit_scale(n, rt.gmax);
    int l = -1;
    if (live) {
        const int leaf = general_leaf(cm, r, rt.t);
        leaf_idx[row] = leaf;
        l = local_leaf(leaf, rt.leaf0, rt.n_leaves);
    }
    const float *p = P + rr * D, *y = Y + rr * D;
    for_each_wave_leaf(l, lane, [&](int k, bool mine, unsigned long long same, bool leader) {
        unsigned long long *a = rt.acc + static_cast<size_t>(k) * (D + 1);
        for (int j = 0; j < D; ++j) {
            const long long q = wave_sum(mine ? refit_quantise(__fsub_rn(p[j], y[j]), scale) : 0ll);
            if (leader && q != 0) atomicAdd(&a[j], static_cast<unsigned long long>(q));
        }
        if (leader) atomicAdd(&a[D], static_cast<unsigned long long>(__popcll(same)));
    });
}

template <int DMAX, bool GREEDY>
__global__ __launch_bounds__(kRefitRows) void k_refit_accum(LeavesModel cm, RefitTree rt, const float *__restrict__ obs, int F,
                                                            const int32_t *__restrict__ cat_codes, int Fc, int n, int n_tiles, int D,
                                                            const float *__restrict__ P, const float *__restrict__ Y, int32_t *__restrict__ leaf_idx,
                                                            int vec_io) {
    extern __shared__ float rtile[];   // [kRefitRows][F | 1] floats, then [n_leaves][D + 1] int64 (the tile is a multiple of 256 bytes)
    const int lane = threadIdx.x;
    const int xs = F | 1;
    const LeafAccLds<1> lacc{reinterpret_cast<unsigned long long *>(rtile + static_cast<size_t>(kRefitRows) * xs), rt.n_leaves, D + 1};
    lacc.zero(lane);
    const double scale = refit_scale(n, rt.gmax);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (uniform over the block)
        const int r0 = tile * kRefitRows;
        const int rows = min(kRefitRows, n - r0);
        const bool live = lane < rows;
        const size_t row = static_cast<size_t>(r0) + (live ? lane : 0);
        float g[DMAX], y[DMAX];   // the row's prediction, then its gradient; in flight together with the tile
        stream_load_row<DMAX>(P + row * D, D, vec_io != 0, g);
        stream_load_row<DMAX>(Y + row * D, D, vec_io != 0, y);
        __syncthreads();   // the previous tile has been read (and, the first time, the accumulators are zero)
        stream_stage_tile(rtile, obs, F, r0, rows, lane);
        __syncthreads();
        int l = -1;
        if (live) {
            const int leaf = stream_leaf<GREEDY>(cm, rtile + lane * xs, cat_codes ? cat_codes + row * Fc : nullptr, rt.t);
            leaf_idx[row] = leaf;
            l = local_leaf(leaf, rt.leaf0, rt.n_leaves);
        }
#pragma unroll
        for (int j = 0; j < DMAX; ++j) g[j] = __fsub_rn(g[j], y[j]);
        lacc.template add<DMAX>(l, lane, D, [&](int, int j) { return refit_quantise(g[j], scale); });
    }
    lacc.flush(rt.acc, lane);
}

// ------------------------------------------------------------------------------------------------------------ finalize
__global__ __launch_bounds__(256) void k_refit_finalize(RefitTree rt, const int32_t *__restrict__ depths, int oblivious, const float *__restrict__ values,
                                                        int n, int D, double decay, double keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rt.n_leaves * D) return;
    const int l = i / D, j = i - l * D;
    const float old = values[static_cast<size_t>(rt.leaf0 + l) * D + j];
    const long long S = static_cast<long long>(rt.acc[static_cast<size_t>(l) * (D + 1) + j]);
    const long long cnt = static_cast<long long>(rt.acc[static_cast<size_t>(l) * (D + 1) + D]);
    const int depth = oblivious ? depths[rt.t] : depths[rt.leaf0 + l];
    float v = old;   // a leaf without rows and a leaf of depth 0 keep their value
    if (cnt > 0 && depth > 0) {
        // append_tree's expression: (sum / scale) / count, every operation rounded once (the first is exact: a power of two)
        const double mean = __ddiv_rn(__ddiv_rn(static_cast<double>(S), refit_scale(n, rt.gmax)), static_cast<double>(cnt));
        v = decay == 0.0 ? static_cast<float>(mean) : static_cast<float>(__dadd_rn(__dmul_rn(decay, static_cast<double>(old)), __dmul_rn(keep, mean)));
    }
    rt.new_values[i] = v;
}

// ------------------------------------------------------------------------------------------------------------ apply
__global__ __launch_bounds__(256) void k_refit_apply(RefitTree rt, ChainRates rr, const int32_t *__restrict__ leaf_idx, const float *__restrict__ Y, int D,
                                                     size_t total, float *__restrict__ P) {
    uint32_t m = 0;
    const float *rate = rr.rate + static_cast<size_t>(rt.t) * rr.rate_stride;
    for (size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const size_t row = e / D;
        const int j = static_cast<int>(e - row * D);
        const int l = leaf_idx[row] - rt.leaf0;
        float p = P[e];
        if (l >= 0 && l < rt.n_leaves) {
            const float v = rt.new_values[static_cast<size_t>(l) * D + j];
            bool owned = false;
            for (int o = 0; o < rr.n_opts; ++o)   // predict_continue's chain: every optimizer that owns the output, in order
                if (j >= rr.opt_start[o] && j < rr.opt_stop[o]) { p = __fmaf_rn(-rate[o], v, p); owned = true; }
            if (owned) P[e] = p;
        }
        m = max(m, refit_abs_bits(__fsub_rn(p, Y[e])));
    }
    refit_block_max(m, rt.gmax_next);
}

template <int DMAX, bool GREEDY>
bool launch_refit_accum(const LeavesModel &cm, const RefitTree &rt, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int D, const float *P,
                        const float *Y, int32_t *leaf_idx, hipStream_t s) {
    const int n_tiles = (n + kRefitRows - 1) / kRefitRows;
    const LeafAccPlan plan = leaf_acc_plan(stream_tile_bytes(F), static_cast<size_t>(rt.n_leaves) * (D + 1) * sizeof(unsigned long long), n_tiles,
                                           kRefitBlocksPerCu, stream_cu_count());
    if (!plan.fits) return false;   // rows too wide, or a tree with too many accumulators, for the LDS of a CU
    static StreamLdsOptIn optin;
    if (!optin.ok(k_refit_accum<DMAX, GREEDY>, plan.lds)) return false;
    const int vec_io = (D & 3) == 0 && ((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0;
    hipLaunchKernelGGL((k_refit_accum<DMAX, GREEDY>), dim3(plan.blocks), dim3(kRefitRows), plan.lds, s, cm, rt, obs, F, cat_codes, Fc, n, n_tiles, D, P, Y, leaf_idx,
                       vec_io);
    return true;
}

}  // namespace

int refit_leaves(const PredictModel &pm, const int32_t *tree_first_leaf, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                 int stop_tree, double decay, const float *targets, float *P, int32_t *leaf_idx, unsigned long long *acc, float *new_values,
                 uint32_t *gmax, bool generic, hipStream_t s) {
    int streamed = 0;
    const int D = pm.D;
    const size_t total = static_cast<size_t>(n) * D;
    const int eblocks = grid_for(total, 256, 4096);
    const LeavesModel cm = leaves_model(pm);
    const bool stream = leaves_streamable(pm, generic) && D <= 64;
    auto first_leaf = [&](int t) { return t < pm.n_trees ? tree_first_leaf[t] : pm.n_leaves; };
    // P over the trees before the range: the tiled bias carried through [0, start_tree) by predict_continue's own kernels
    hipLaunchKernelGGL(k_refit_tile_bias, dim3(eblocks), dim3(256), 0, s, pm.bias, D, total, P);
    if (start_tree > 0) predict_continue(pm, obs, F, cat_codes, Fc, n, 0, start_tree, P, P, generic, s);
    hipLaunchKernelGGL(k_refit_gmax, dim3(eblocks), dim3(256), 0, s, P, targets, total, gmax);
    const ChainRates rr = chain_rates(pm);
    const int base = first_leaf(start_tree);
    for (int t = start_tree; t < stop_tree; ++t) {
        RefitTree rt{};
        rt.t = t; rt.leaf0 = first_leaf(t); rt.n_leaves = first_leaf(t + 1) - rt.leaf0;
        rt.gmax = gmax + (t - start_tree);
        rt.gmax_next = gmax + (t + 1 - start_tree);
        rt.acc = acc + static_cast<size_t>(rt.leaf0 - base) * (D + 1);
        rt.new_values = new_values + static_cast<size_t>(rt.leaf0 - base) * D;
        bool done = rt.n_leaves <= 0;   // (a tree without leaves, which no grower writes: nothing to sum, the apply pass only hands gmax on)
        if (!done && stream)
            done = with_stream_dmax(D, [&](auto dmax) {
                constexpr int DMAX = decltype(dmax)::value;
                return pm.oblivious ? launch_refit_accum<DMAX, false>(cm, rt, obs, F, cat_codes, Fc, n, D, P, targets, leaf_idx, s)
                                    : launch_refit_accum<DMAX, true>(cm, rt, obs, F, cat_codes, Fc, n, D, P, targets, leaf_idx, s);
            });
        if (done && rt.n_leaves > 0) ++streamed;
        if (!done)
            hipLaunchKernelGGL(k_refit_accum_general, dim3((n + 255) / 256), dim3(256), 0, s, cm, rt, obs, F, cat_codes, Fc, n, D, P, targets, leaf_idx);
        if (rt.n_leaves > 0)
            hipLaunchKernelGGL(k_refit_finalize, dim3((rt.n_leaves * D + 255) / 256), dim3(256), 0, s, rt, pm.depths, pm.oblivious, pm.values, n, D, decay,
                               1.0 - decay);
        hipLaunchKernelGGL(k_refit_apply, dim3(eblocks), dim3(256), 0, s, rt, rr, leaf_idx, targets, D, total, P);
    }
    return streamed;
}

}  // namespace kern
}  // namespace gbrl
