// predict_leaves_codes.hip -- gfx950 kernels behind GBRL::predict_leaves_prepared / GBRL::leaf_counts_prepared: predict_leaves.hip's answers (the
// GLOBAL leaf a tree routes a row to; the rows per leaf) with the row read from a prepared data set's bin codes, x > v <=> code > bin
// (engine_codes.hip has the argument).  The walks, the code tile, the family choice and the LDS opt-in are predict_rowwalk.h's, the counter
// helpers leaf_accum.h's; sample j of the call's m is data set row cr.rows[cr.row0 + j] (or cr.row0 + j), and everything a kernel writes is indexed by j.
//
//   k_leaves_codes<GREEDY>          lane = row, one wave per block, the block's 64 rows as a code tile in LDS ((G * 8) | 1 words per row), trees in
//                                   groups of kLeavesCodesG = 16 index registers, k_leaves' stride-17 staging transpose behind the tile: one 16-byte
//                                   store per lane and quad when T % 4 == 0 and the pointer allows, scalar stores otherwise.  n (32 G + 4 T) bytes.
//   k_leaf_counts_codes<GREEDY>     one wave per block, row tiles in a grid-stride loop; the tile and the launch's uint32 counters share the LDS.
//                                   A group of kLeavesCodesG trees is WALKED first -- sixteen counter indices in registers, no atomic between one
//                                   tree's tile reads and the next tree's, so the chains are independent and the scheduler may overlap them --
//                                   and only then are the group's ds_add_u32 issued, back to back (no return value: nothing waits on them).  A tree
//                                   of at most kLeafAccWaveLeaves leaves would put 16 or more lanes on one counter and serialise there (refit.hip's
//                                   threshold): such a tree is aggregated in the wave (for_each_wave_leaf) and adds once per distinct leaf.  At the
//                                   block's end the non-zero counters go to the global ones, consecutive lanes on consecutive counters.  Integer
//                                   adds: exact and order-free, so two calls and both families give the same bytes.
//   launch plan (leaves_codes_plan) the counter chunk is chosen per width: the largest power of two that leaves the block count per CU the code tile
//                                   alone would get (LeafAccPlan's rule: 160 KiB per CU, at most kLeavesCodesPerCu one-wave blocks), never below
//                                   kLeafCountChunk and never beyond kStreamLdsBudget; 0 when the tile does not fit beside kLeafCountChunk counters.
//                                   kern::leaf_counts_codes cuts the range into runs of whole trees whose leaves fit the chunk, one launch per run;
//                                   a tree with more leaves than the chunk takes the general kernel alone.
//   k_leaves_codes_general          one thread per row, the records read in place (GeneralCodeRow), the reference's walk: a tile too wide for the
//   k_leaf_counts_codes_general     budget, greedy ensembles without valid node records, max_depth == 0, a refused LDS opt-in, and the cross-check
//                                   behind GBRL_HIP_LEAVES_GENERIC=1.  The count form adds once per distinct leaf and wave (ballot).
#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kLeavesCodesG = 16;                              // trees per group: 16 index registers
constexpr int kLeavesCodesStageStride = kLeavesCodesG + 1;     // odd: the lane-per-row writes of one tree touch 64 banks
constexpr size_t kLeavesCodesStageBytes = static_cast<size_t>(kStreamRows) * kLeavesCodesStageStride * sizeof(int32_t);
constexpr int kLeavesCodesPerCu = 8;                           // one-wave blocks counted per CU (k_leaf_counts' cap)
constexpr size_t kLdsPerCu = 160 * 1024;                       // leaf_acc_plan's figure

struct LeavesCodesPlan { int chunk; size_t lds; };   // chunk == 0: no streaming count launch at this width

// host only, no device: the counter chunk and the dynamic LDS of a count launch on a data set of G 16-column groups
LeavesCodesPlan leaves_codes_plan(int G) {
    const size_t tile = static_cast<size_t>(kStreamRows) * ((static_cast<size_t>(G) * 8) | 1) * sizeof(uint32_t);
    if (G < 1 || !leaf_acc_plan(tile, sizeof(uint32_t) * kLeafCountChunk, 1, kLeavesCodesPerCu, 1).fits) return {0, 0};
    const size_t per_cu = std::min<size_t>(kLeavesCodesPerCu, std::max<size_t>(1, kLdsPerCu / tile));   // the tile alone
    const size_t share = kLdsPerCu / per_cu;
    const size_t room = share > tile ? (share - tile) / sizeof(uint32_t) : 0;
    size_t chunk = kLeafCountChunk;
    while (chunk * 2 <= room && leaf_acc_plan(tile, sizeof(uint32_t) * chunk * 2, 1, kLeavesCodesPerCu, 1).fits) chunk *= 2;
    return {static_cast<int>(chunk), tile + sizeof(uint32_t) * chunk};
}

// the data set row of sample j
__device__ __forceinline__ int code_row_of(const CodeRows &cr, int j) { return cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j; }

// ------------------------------------------------------------------------------------------------------------ general kernels
__global__ __launch_bounds__(256) void k_leaves_codes_general(LeavesModel cm, CodeRows cr, int m, int start_tree, int stop_tree, int32_t *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const GeneralCodeRow r{cr.codes + static_cast<size_t>(code_row_of(cr, j)) * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    int32_t *o = out + static_cast<size_t>(j) * (stop_tree - start_tree);
    for (int t = start_tree; t < stop_tree; ++t) o[t - start_tree] = general_leaf(cm, r, t);
}

__global__ __launch_bounds__(256) void k_leaf_counts_codes_general(LeavesModel cm, CodeRows cr, int m, int start_tree, int stop_tree, uint32_t *__restrict__ counts) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < m;   // (dead lanes stay for the ballots)
    const GeneralCodeRow r{cr.codes + static_cast<size_t>(code_row_of(cr, live ? j : 0)) * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const int lane = threadIdx.x & (kWave - 1);
    for (int t = start_tree; t < stop_tree; ++t) {   // (uniform over the block)
        const int leaf = live ? general_leaf(cm, r, t) : -1;
        for_each_wave_leaf(leaf, lane, [&](int l, bool, unsigned long long same, bool leader) {
            if (leader) atomicAdd(&counts[l], static_cast<uint32_t>(__popcll(same)));
        });
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernels
template <bool GREEDY>
__global__ __launch_bounds__(kStreamRows) void k_leaves_codes(LeavesModel cm, CodeRows cr, int m, int start_tree, int stop_tree, int32_t *__restrict__ out,
                                                              int vec_out) {
    extern __shared__ __align__(16) uint32_t lc_tile[];   // [kStreamRows][stream_code_stride(G)] words, then [kStreamRows][kLeavesCodesStageStride] ints
    const int lane = threadIdx.x;
    const int ws = stream_code_stride(cr.groups);
    int32_t *stage = reinterpret_cast<int32_t *>(lc_tile + static_cast<size_t>(kStreamRows) * ws);
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, m - r0);
    const bool live = lane < rows;
    const size_t T = static_cast<size_t>(stop_tree - start_tree);
    const int my_row = code_row_of(cr, r0 + (live ? lane : 0));   // (a lane without a row names the block's first: a valid record, never stored)
    stream_stage_code_tile(lc_tile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
    __syncthreads();
    const StreamCodeRow x{reinterpret_cast<const uint16_t *>(lc_tile + (live ? lane : 0) * ws)};
    int32_t *orow0 = out + static_cast<size_t>(r0) * T;
    for (int t0 = start_tree; t0 < stop_tree; t0 += kLeavesCodesG) {   // (wave-uniform)
        const int gn = min(kLeavesCodesG, stop_tree - t0);
        int leaf[kLeavesCodesG];
#pragma unroll
        for (int g = 0; g < kLeavesCodesG; ++g) leaf[g] = (g < gn) ? stream_leaf<GREEDY>(cm, x, static_cast<const int32_t *>(nullptr), t0 + g) : 0;
#pragma unroll
        for (int g = 0; g < kLeavesCodesG; ++g) stage[lane * kLeavesCodesStageStride + g] = leaf[g];
        __syncthreads();
        const size_t c0 = static_cast<size_t>(t0 - start_tree);   // first column of the group: a multiple of 16
        if (vec_out) {   // T % 4 == 0: gn is a whole number of quads and every segment is 16-byte aligned
            const int quads = gn >> 2;
            for (int i = lane; i < rows * quads; i += kStreamRows) {
                const int r = i / quads, q = i - r * quads;
                const int32_t *sp = stage + r * kLeavesCodesStageStride + 4 * q;
                *reinterpret_cast<int4 *>(orow0 + r * T + c0 + 4 * q) = make_int4(sp[0], sp[1], sp[2], sp[3]);
            }
        } else {
            for (int i = lane; i < rows * gn; i += kStreamRows) {
                const int r = i / gn, g = i - r * gn;
                orow0[r * T + c0 + g] = stage[r * kLeavesCodesStageStride + g];
            }
        }
        __syncthreads();   // the staging buffer is rewritten by the next group
    }
}

// counts[leaf_base + c] += rows of the call that reach counter c of the run [start_tree, stop_tree), whose n_counters leaves start at leaf_base
template <bool GREEDY>
__global__ __launch_bounds__(kStreamRows) void k_leaf_counts_codes(LeavesModel cm, CodeRows cr, int m, int n_tiles, int n_trees, int start_tree, int stop_tree,
                                                                   int leaf_base, int n_counters, uint32_t *__restrict__ counts) {
    extern __shared__ __align__(16) uint32_t lcc_tile[];   // [kStreamRows][stream_code_stride(G)] words, then n_counters uint32
    const int lane = threadIdx.x;
    const int ws = stream_code_stride(cr.groups);
    uint32_t *cnt = lcc_tile + static_cast<size_t>(kStreamRows) * ws;
    leaf_acc_zero(cnt, n_counters, lane, kStreamRows);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (uniform over the block)
        const int r0 = tile * kStreamRows;
        const int rows = min(kStreamRows, m - r0);
        const bool live = lane < rows;
        const int my_row = code_row_of(cr, r0 + (live ? lane : 0));
        __syncthreads();   // the previous tile has been read (and, the first time, the counters are zero)
        stream_stage_code_tile(lcc_tile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
        __syncthreads();
        // (a lane without a row walks the tile's first row, so that the whole wave reaches the ballots; its index is dropped below)
        const StreamCodeRow x{reinterpret_cast<const uint16_t *>(lcc_tile + (live ? lane : 0) * ws)};
        for (int t0 = start_tree; t0 < stop_tree; t0 += kLeavesCodesG) {   // (wave-uniform)
            const int gn = min(kLeavesCodesG, stop_tree - t0);
            // the walk of the whole group: counter indices in registers, -1 for "no counter"
            int c[kLeavesCodesG];
#pragma unroll
            for (int g = 0; g < kLeavesCodesG; ++g) {
                const int l = (g < gn) ? stream_leaf<GREEDY>(cm, x, static_cast<const int32_t *>(nullptr), t0 + g) - leaf_base : -1;
                c[g] = (live && l >= 0 && l < n_counters) ? l : -1;
            }
            // the group's adds, back to back
#pragma unroll
            for (int g = 0; g < kLeavesCodesG; ++g) {
                if (g >= gn) continue;   // (wave-uniform)
                const int t = t0 + g;
                const int tree_leaves = (t + 1 < n_trees ? cm.tree_indices[t + 1] : cm.n_leaves) - cm.tree_indices[t];
                if (tree_leaves <= kLeafAccWaveLeaves) {   // (wave-uniform) 16 or more lanes per counter: one add per distinct leaf
                    for_each_wave_leaf(c[g], lane, [&](int k, bool, unsigned long long same, bool leader) {
                        if (leader) atomicAdd(&cnt[k], static_cast<uint32_t>(__popcll(same)));
                    });
                } else if (c[g] >= 0) {
                    atomicAdd(&cnt[c[g]], 1u);
                }
            }
        }
    }
    __syncthreads();
    leaf_acc_flush(cnt, counts + leaf_base, n_counters, lane, kStreamRows);
}

template <bool GREEDY>
bool launch_leaves_codes(const LeavesModel &cm, const CodeRows &cr, int m, int start_tree, int stop_tree, int32_t *out, hipStream_t s) {
    const size_t lds = stream_code_tile_bytes(cr.groups) + kLeavesCodesStageBytes;
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile beside the staging buffer
    static StreamLdsOptIn optin;
    if (!optin.ok(k_leaves_codes<GREEDY>, lds)) return false;
    const int vec_out = ((stop_tree - start_tree) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    hipLaunchKernelGGL((k_leaves_codes<GREEDY>), dim3((m + kStreamRows - 1) / kStreamRows), dim3(kStreamRows), lds, s, cm, cr, m, start_tree, stop_tree, out,
                       vec_out);
    return true;
}

template <bool GREEDY>
bool launch_leaf_counts_codes(const LeavesModel &cm, const CodeRows &cr, int m, int n_trees, int start_tree, int stop_tree, int leaf_base, int n_counters,
                              uint32_t *counts, hipStream_t s) {
    const int n_tiles = (m + kStreamRows - 1) / kStreamRows;
    const LeafAccPlan plan = leaf_acc_plan(stream_code_tile_bytes(cr.groups), static_cast<size_t>(n_counters) * sizeof(uint32_t), n_tiles, kLeavesCodesPerCu,
                                           stream_cu_count());
    if (!plan.fits) return false;
    static StreamLdsOptIn optin;
    if (!optin.ok(k_leaf_counts_codes<GREEDY>, plan.lds)) return false;
    hipLaunchKernelGGL((k_leaf_counts_codes<GREEDY>), dim3(plan.blocks), dim3(kStreamRows), plan.lds, s, cm, cr, m, n_tiles, n_trees, start_tree, stop_tree,
                       leaf_base, n_counters, counts);
    return true;
}

// the model view of the float walk with the threshold words replaced by bins (predict_continue_codes' rule)
LeavesModel leaves_code_model(const PredictModel &pm, const CodeTables &ct) {
    LeavesModel cm = leaves_model(pm);
    cm.cond_pack = ct.cond_pack;
    cm.grd_nodes = ct.grd_nodes;
    cm.feature_bins = ct.bins;
    return cm;
}

}  // namespace

void leaves_codes_geometry(int n_groups, int *group_trees, int *count_chunk, uint64_t *lds_bytes) {
    const LeavesCodesPlan p = leaves_codes_plan(n_groups);
    if (group_trees) *group_trees = kLeavesCodesG;
    if (count_chunk) *count_chunk = p.chunk;
    if (lds_bytes) *lds_bytes = p.lds;
}

void predict_leaves_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int start_tree, int stop_tree, int32_t *out, bool generic,
                          hipStream_t s) {
    if (m <= 0 || stop_tree <= start_tree) return;
    const LeavesModel cm = leaves_code_model(pm, ct);
    if (leaves_streamable(pm, generic)) {
        if (pm.oblivious ? launch_leaves_codes<false>(cm, cr, m, start_tree, stop_tree, out, s) : launch_leaves_codes<true>(cm, cr, m, start_tree, stop_tree, out, s))
            return;
    }
    hipLaunchKernelGGL(k_leaves_codes_general, dim3((m + 255) / 256), dim3(256), 0, s, cm, cr, m, start_tree, stop_tree, out);
}

void leaf_counts_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, const int32_t *tree_first_leaf, int m, int start_tree, int stop_tree,
                       uint32_t *counts, bool generic, hipStream_t s) {
    if (m <= 0 || stop_tree <= start_tree) return;
    const LeavesModel cm = leaves_code_model(pm, ct);
    const int chunk = leaves_codes_plan(cr.groups).chunk;
    auto first_leaf = [&](int t) { return t < pm.n_trees ? tree_first_leaf[t] : pm.n_leaves; };
    auto general = [&](int a, int b) {
        hipLaunchKernelGGL(k_leaf_counts_codes_general, dim3((m + 255) / 256), dim3(256), 0, s, cm, cr, m, a, b, counts);
    };
    if (!leaves_streamable(pm, generic) || chunk == 0) { general(start_tree, stop_tree); return; }
    // runs of whole trees whose leaves fit the chunk's counters; one launch per run
    int a = start_tree;
    while (a < stop_tree) {
        int b = a;
        while (b < stop_tree && first_leaf(b + 1) - first_leaf(a) <= chunk) ++b;
        if (b == a) { general(a, a + 1); ++a; continue; }   // a tree with more leaves than the chunk holds
        const int base = first_leaf(a), nc = first_leaf(b) - base;
        const bool ok = pm.oblivious ? launch_leaf_counts_codes<false>(cm, cr, m, pm.n_trees, a, b, base, nc, counts, s)
                                     : launch_leaf_counts_codes<true>(cm, cr, m, pm.n_trees, a, b, base, nc, counts, s);
        if (!ok) { general(a, stop_tree); return; }   // a refused LDS opt-in: the rest of the range in one launch
        a = b;
    }
}

}  // namespace kern
}  // namespace gbrl
