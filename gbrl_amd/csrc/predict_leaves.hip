// predict_leaves.hip -- gfx950 kernels behind GBRL::predict_leaves / GBRL::leaf_counts: WHERE a row lands, not what it sums to.  For a row and a
// tree t the answer is the GLOBAL leaf index, the row of `values` the walk of predict_continue.hip gathers (both walks are predict_rowwalk.h's,
// the ones k_continue, k_staged and k_refit_accum call, as are the model view, the family choice and the LDS opt-in):
//   oblivious (predictor.cpp:99-118)   tree_indices[t] + sum_d pass(cond[t * max_depth + d]) << (depths[t] - 1 - d); depth 0: tree_indices[t]
//   greedy    (predictor.cpp:208-228)  the first leaf in storage order from tree_indices[t] on whose conditions all hold (tested from depth - 1
//                                      down to 0 against inequality_directions).  A depth-0 leaf never passes there (Q7): the search then runs on
//                                      into the leaves of the following trees, and a search that runs off the ensemble gives -1 (the reference's
//                                      walk ends there and applies nothing).  Well-formed trees without stumps never do either.
// The walk reads no leaf value, so nothing here depends on output_dim.
//
//   k_leaves<GREEDY>         k_continue's layout without the base load, the value gather and the chain: lane = row, one wave per block, the
//                            block's 64 rows in LDS at stride F | 1 (predict_rowwalk.h), conditions / node records through wave-uniform
//                            addresses, trees in groups of kLeavesG = 16.  The output is row-major [n][T]: a lane-per-row store would have stride
//                            T, so a group's 64 x 16 indices are staged in LDS (stride 17: lane-per-row writes touch 64 banks) and written so
//                            that consecutive lanes cover a row's contiguous segment -- one 16-byte store per lane and quad when T % 4 == 0 and
//                            the pointer allows (a group starts at a multiple of 16 trees, so its segment is then 16-byte aligned and whole
//                            quads), scalar stores otherwise.  The kernel moves n (4 F + 4 T) bytes.
//   k_leaf_counts<GREEDY>    the same walk reduced on chip.  A block (one wave) takes row tiles in a grid-stride loop and keeps the uint32
//                            counters of the call's tree chunk in LDS behind the tile (ds_add_u32, no return); at its end it adds the non-zero
//                            ones to the global uint32 counters, consecutive lanes on consecutive counters.  Global atomics: blocks x leaves
//                            of the chunk, never n x T.  Integer adds are exact and order-free: two calls, the same bytes.  A chunk holds at
//                            most kLeafCountChunk counters; kern::leaf_counts cuts the range into runs of whole trees that fit, one launch per
//                            run (the rows are re-read per run: 4 n F bytes each).  A tree with more leaves than a chunk takes the general kernel.
//   k_leaves_general         anything the file format can hold: one thread per row, rows from global memory, the reference's walk (greedy: leaf
//   k_leaf_counts_general    by leaf).  Rows too wide for the LDS budget, greedy ensembles without valid node records, max_depth == 0, and the
//                            cross-check behind GBRL_HIP_LEAVES_GENERIC=1.  The count kernel aggregates a wave's equal leaves (ballot) and
//                            issues one global add per distinct leaf and wave.
#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kLeavesRows = kStreamRows;           // rows per block = one wave
constexpr int kLeavesG = 16;                       // trees per group of k_leaves: 16 index registers, a 64 x 17-int staging buffer (4352 bytes)
constexpr int kLeavesStageStride = kLeavesG + 1;   // odd: the lane-per-row writes of one tree touch 64 banks
constexpr size_t kLeavesStageBytes = static_cast<size_t>(kLeavesRows) * kLeavesStageStride * sizeof(int32_t);

// ------------------------------------------------------------------------------------------------------------ general kernels
__global__ __launch_bounds__(256) void k_leaves_general(LeavesModel cm, const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes,
                                                        int Fc, int n, int start_tree, int stop_tree, int32_t *__restrict__ out) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= static_cast<size_t>(n)) return;
    const GeneralRow r{obs + row * F, cat_codes ? cat_codes + row * Fc : nullptr};
    int32_t *o = out + row * static_cast<size_t>(stop_tree - start_tree);
    for (int t = start_tree; t < stop_tree; ++t) o[t - start_tree] = general_leaf(cm, r, t);
}

__global__ __launch_bounds__(256) void k_leaf_counts_general(LeavesModel cm, const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes,
                                                             int Fc, int n, int start_tree, int stop_tree, uint32_t *__restrict__ counts) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = row < static_cast<size_t>(n);   // (dead lanes stay for the ballots)
    const size_t rr = live ? row : 0;
    const GeneralRow r{obs + rr * F, cat_codes ? cat_codes + rr * Fc : nullptr};
    const int lane = threadIdx.x & (kWave - 1);
    for (int t = start_tree; t < stop_tree; ++t) {   // (uniform over the block)
        const int leaf = live ? general_leaf(cm, r, t) : -1;
        // the global leaf is the counter: the lowest lane that holds it adds the number of lanes that do
        for_each_wave_leaf(leaf, lane, [&](int l, bool, unsigned long long same, bool leader) {
            if (leader) atomicAdd(&counts[l], static_cast<uint32_t>(__popcll(same)));
        });
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernels
template <bool GREEDY>
__global__ __launch_bounds__(kLeavesRows) void k_leaves(LeavesModel cm, const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes, int Fc,
                                                        int n, int start_tree, int stop_tree, int32_t *__restrict__ out, int vec_out) {
    extern __shared__ float ltile[];   // [kLeavesRows][F | 1] floats, then [kLeavesRows][kLeavesStageStride] ints
    const int lane = threadIdx.x;
    const int xs = F | 1;
    int32_t *stage = reinterpret_cast<int32_t *>(ltile + static_cast<size_t>(kLeavesRows) * xs);
    const int r0 = blockIdx.x * kLeavesRows;
    const int rows = min(kLeavesRows, n - r0);
    const bool live = lane < rows;
    const size_t T = static_cast<size_t>(stop_tree - start_tree);
    stream_stage_tile(ltile, obs, F, r0, rows, lane);
    __syncthreads();
    const float *x = ltile + (live ? lane : 0) * xs;
    const int32_t *xc = cat_codes ? cat_codes + (static_cast<size_t>(r0) + (live ? lane : 0)) * Fc : nullptr;
    int32_t *orow0 = out + static_cast<size_t>(r0) * T;
    for (int t0 = start_tree; t0 < stop_tree; t0 += kLeavesG) {   // (wave-uniform)
        const int gn = min(kLeavesG, stop_tree - t0);
        int leaf[kLeavesG];
#pragma unroll
        for (int g = 0; g < kLeavesG; ++g) leaf[g] = (g < gn) ? stream_leaf<GREEDY>(cm, x, xc, t0 + g) : 0;
#pragma unroll
        for (int g = 0; g < kLeavesG; ++g) stage[lane * kLeavesStageStride + g] = leaf[g];
        __syncthreads();
        const size_t c0 = static_cast<size_t>(t0 - start_tree);   // first column of the group
        if (vec_out) {   // T % 4 == 0: gn is a whole number of quads and every segment is 16-byte aligned
            const int quads = gn >> 2;
            for (int i = lane; i < rows * quads; i += kLeavesRows) {
                const int r = i / quads, q = i - r * quads;
                const int32_t *sp = stage + r * kLeavesStageStride + 4 * q;
                *reinterpret_cast<int4 *>(orow0 + r * T + c0 + 4 * q) = make_int4(sp[0], sp[1], sp[2], sp[3]);
            }
        } else {
            for (int i = lane; i < rows * gn; i += kLeavesRows) {
                const int r = i / gn, g = i - r * gn;
                orow0[r * T + c0 + g] = stage[r * kLeavesStageStride + g];
            }
        }
        __syncthreads();   // the staging buffer is rewritten by the next group
    }
}

template <bool GREEDY>
__global__ __launch_bounds__(kLeavesRows) void k_leaf_counts(LeavesModel cm, const float *__restrict__ obs, int F, const int32_t *__restrict__ cat_codes,
                                                             int Fc, int n, int n_tiles, int start_tree, int stop_tree, int leaf_base, int n_counters,
                                                             uint32_t *__restrict__ counts) {
    extern __shared__ float ctile_[];   // [kLeavesRows][F | 1] floats, then n_counters uint32
    const int lane = threadIdx.x;
    const int xs = F | 1;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(ctile_ + static_cast<size_t>(kLeavesRows) * xs);
    leaf_acc_zero(cnt, n_counters, lane, kLeavesRows);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (uniform over the block)
        const int r0 = tile * kLeavesRows;
        const int rows = min(kLeavesRows, n - r0);
        __syncthreads();   // the previous tile has been read (and, the first time, the counters are zero)
        stream_stage_tile(ctile_, obs, F, r0, rows, lane);
        __syncthreads();
        if (lane < rows) {
            const float *x = ctile_ + lane * xs;
            const int32_t *xc = cat_codes ? cat_codes + (static_cast<size_t>(r0) + lane) * Fc : nullptr;
#pragma unroll 4
            for (int t = start_tree; t < stop_tree; ++t) {
                const int c = stream_leaf<GREEDY>(cm, x, xc, t) - leaf_base;
                if (c >= 0 && c < n_counters) atomicAdd(&cnt[c], 1u);
            }
        }
    }
    __syncthreads();
    leaf_acc_flush(cnt, counts + leaf_base, n_counters, lane, kLeavesRows);
}

template <bool GREEDY>
bool launch_leaves(const LeavesModel &cm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree, int32_t *out,
                   hipStream_t s) {
    const size_t lds = stream_tile_bytes(F) + kLeavesStageBytes;
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile beside the staging buffer
    static StreamLdsOptIn optin;
    if (!optin.ok(k_leaves<GREEDY>, lds)) return false;
    const int vec_out = ((stop_tree - start_tree) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    hipLaunchKernelGGL((k_leaves<GREEDY>), dim3((n + kLeavesRows - 1) / kLeavesRows), dim3(kLeavesRows), lds, s, cm, obs, F, cat_codes, Fc, n, start_tree,
                       stop_tree, out, vec_out);
    return true;
}

template <bool GREEDY>
bool launch_leaf_counts(const LeavesModel &cm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                        int leaf_base, int n_counters, uint32_t *counts, hipStream_t s) {
    const int n_tiles = (n + kLeavesRows - 1) / kLeavesRows;
    const LeafAccPlan plan = leaf_acc_plan(stream_tile_bytes(F), static_cast<size_t>(n_counters) * sizeof(uint32_t), n_tiles, 8, stream_cu_count());
    if (!plan.fits) return false;   // rows too wide for an LDS tile beside the counters
    static StreamLdsOptIn optin;
    if (!optin.ok(k_leaf_counts<GREEDY>, plan.lds)) return false;
    hipLaunchKernelGGL((k_leaf_counts<GREEDY>), dim3(plan.blocks), dim3(kLeavesRows), plan.lds, s, cm, obs, F, cat_codes, Fc, n, n_tiles, start_tree, stop_tree,
                       leaf_base, n_counters, counts);
    return true;
}

}  // namespace

int leaf_counts_chunk() { return kLeafCountChunk; }

void predict_leaves(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree, int32_t *out,
                    bool generic, hipStream_t s) {
    const LeavesModel cm = leaves_model(pm);
    if (leaves_streamable(pm, generic)) {
        if (pm.oblivious ? launch_leaves<false>(cm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s)
                         : launch_leaves<true>(cm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out, s))
            return;
    }
    hipLaunchKernelGGL(k_leaves_general, dim3((n + 255) / 256), dim3(256), 0, s, cm, obs, F, cat_codes, Fc, n, start_tree, stop_tree, out);
}

void leaf_counts(const PredictModel &pm, const int32_t *tree_first_leaf, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                 int stop_tree, uint32_t *counts, bool generic, hipStream_t s) {
    const LeavesModel cm = leaves_model(pm);
    const bool stream = leaves_streamable(pm, generic);
    auto first_leaf = [&](int t) { return t < pm.n_trees ? tree_first_leaf[t] : pm.n_leaves; };
    auto general = [&](int a, int b) {
        hipLaunchKernelGGL(k_leaf_counts_general, dim3((n + 255) / 256), dim3(256), 0, s, cm, obs, F, cat_codes, Fc, n, a, b, counts);
    };
    if (!stream) { general(start_tree, stop_tree); return; }
    // runs of whole trees whose leaves fit a chunk's counters; one launch per run
    int a = start_tree;
    while (a < stop_tree) {
        int b = a;
        while (b < stop_tree && first_leaf(b + 1) - first_leaf(a) <= kLeafCountChunk) ++b;
        if (b == a) { general(a, a + 1); ++a; continue; }   // a tree with more leaves than a chunk holds
        const int base = first_leaf(a), nc = first_leaf(b) - base;
        const bool ok = pm.oblivious ? launch_leaf_counts<false>(cm, obs, F, cat_codes, Fc, n, a, b, base, nc, counts, s)
                                     : launch_leaf_counts<true>(cm, obs, F, cat_codes, Fc, n, a, b, base, nc, counts, s);
        if (!ok) { general(a, stop_tree); return; }   // rows too wide for an LDS tile beside the counters: the rest of the range in one launch
        a = b;
    }
}

}  // namespace kern
}  // namespace gbrl
