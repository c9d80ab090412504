// pd_rows.hip -- gfx950 kernels behind GBRL::partial_dependence_prepared: the predictions of many "columns held constant" variants of a prepared
// data set's rows, none of them materialised.  A variant (col0, code0, col1, code1) reads column col0 (and col1, when >= 0) of every row as the
// constant bin code it names and every other column from the row itself; col0 < 0 is the data set as it is (the baseline).  The walk, the grouping
// of trees, the rates and the owner rule are predict_rowwalk.h's, started from the bias: a variant's rows are the bits predict_continue_codes.hip
// writes from a tiled bias for a data set that really holds those codes.  Per variant and output d one float64 partial per 64 consecutive positions
// of the row list: the wave's sum of (double)p[d] through predict_loss.h's butterfly, finished by staged_loss_finish_rows with (variant, d) as its
// row axis.
//
//   k_pd_rows          lane = row, one wave per block, k_continue_codes' LDS tile.  The block's 64 code records are staged ONCE
//                      (stream_stage_code_tile; with a row list lane j stages the records of rows[j]); then for every variant of the block's run
//                      the lane writes up to two constant codes into its own row's slots of the tile, walks the trees from the bias
//                      (stream_chain_group), stores the row when ICE, sums each output over the wave, lane 0 stores part[(v D + d) nb + block],
//                      and the slots are put back.  A lane touches only its own row's slots and the block is one wave: no barrier between
//                      variants.  Nothing is gathered: a variant costs the walk alone.
//   k_pd_rows_general  one thread per row, the records read in place through PatchedCodeRow (two columns answered from constants): D in 65..128,
//                      optimizers that share outputs, a greedy depth-0 tree, F too wide for the tile, a refused LDS opt-in, a model in which no
//                      optimizer owns an output (the baseline is then the bias), and the cross-check behind GBRL_HIP_PD_GENERIC=1.  Four waves
//                      per block: four partials per output.
//   the block's run    grid.y cuts the launch's variants into runs of per_block (pd_core.h: pd_variants_per_block).
// Stored: the partials and, when asked for, the ICE rows at ice[slot[v]][j][d].  The data set's codes are only ever read.
#include "kernels.h"
#include "kernels_common.h"
#include "pd_core.h"
#include "predict_rowwalk.h"
#include "predict_loss.h"

namespace gbrl {
namespace kern {

namespace {

static_assert(kPdPartialRows == kStagedRows && kStreamRows == kStagedRows, "a wave of either kernel writes exactly one partial per output");
static_assert(kPdMaxLaunchVariants == kPermLaunchVariants, "pd_core.h's launch size is the permutation kernels'");

// a row of a prepared data set with up to TWO columns answered from constants (PermutedCodeRow of perm_loss.hip with a second column)
struct PatchedCodeRow {
    const uint16_t *rec;
    size_t group_stride;
    int col0, code0, col1, code1;   // col < 0: that column is not replaced
    __device__ __forceinline__ bool numeric(const LeavesModel &cm, int f, int c) const {
        const int v = f == col0 ? code0 : f == col1 ? code1 : static_cast<int>(rec[static_cast<size_t>(f >> 4) * group_stride + (f & 15)]);
        return v > cm.feature_bins[c];
    }
    __device__ __forceinline__ bool categorical(const LeavesModel &, int, int) const { return false; }
};

// the wave's sum of every output of the lane's row (zeros for a lane without one); `store` names the lane and the partial that keeps them
template <int DMAX>
__device__ __forceinline__ void pd_store_partials(const float (&p)[DMAX], int D, bool live, bool store, double *__restrict__ part_v, int nb, int partial) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
        if (d < D) {   // (uniform)
            const double s = staged_wave_sum(live ? static_cast<double>(p[d]) : 0.0);
            if (store) part_v[static_cast<size_t>(d) * nb + partial] = s;
        }
}

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX, bool ICE>
__global__ __launch_bounds__(256) void k_pd_rows_general(ChainModel cm, CodeRows cr, int m, int n_trees, const PdVariant *__restrict__ variants,
                                                         const int32_t *__restrict__ slots, int n_variants, int per_block, double *__restrict__ part, int nb,
                                                         float *__restrict__ ice) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < m;   // (whole waves stay for the butterfly)
    const int D = cm.D;
    const int wave = j / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
    const bool store = (threadIdx.x & (kStagedRows - 1)) == 0 && wave < nb;
    const size_t src = live ? static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j) : 0;
    const int v0 = blockIdx.y * per_block, v1 = min(n_variants, v0 + per_block);
    for (int v = v0; v < v1; ++v) {
        const PdVariant pv = variants[v];
        float p[DMAX];
#pragma unroll
        for (int d = 0; d < DMAX; ++d) p[d] = (live && d < D) ? cm.bias[d] : 0.0f;
        if (live) {
            const PatchedCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup, pv.col0, pv.code0, pv.col1, pv.code1};
            for (int t = 0; t < n_trees; ++t)
                if (!general_chain_tree<DMAX>(cm, r, t, p)) break;   // a greedy search ran off the ensemble: the walk ends
            if constexpr (ICE) stream_store_row<DMAX>(ice + (static_cast<size_t>(slots[v]) * m + j) * D, D, false, p);
        }
        pd_store_partials<DMAX>(p, D, live, store, part + static_cast<size_t>(v) * D * nb, nb, wave);
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, bool ICE>
__global__ __launch_bounds__(kStreamRows) void k_pd_rows(ChainModel cm, StreamOwner<DMAX> own, uint64_t cover, CodeRows cr, int m, int n_trees,
                                                         const PdVariant *__restrict__ variants, const int32_t *__restrict__ slots, int n_variants, int per_block,
                                                         double *__restrict__ part, int nb, float *__restrict__ ice, int vec_values, int vec_ice) {
    extern __shared__ __align__(16) uint32_t pdtile[];   // [kStreamRows][stream_code_stride(G)]
    const int lane = threadIdx.x;
    const int D = cm.D;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, m - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    const int at = cr.row0 + r0 + (live ? lane : 0);   // (a lane without a row names the block's first: a valid record, never read back)
    const int my_row = cr.rows ? cr.rows[at] : at;
    stream_stage_code_tile(pdtile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
    __syncthreads();
    uint16_t *mine = reinterpret_cast<uint16_t *>(pdtile + lane * stream_code_stride(cr.groups));   // the lane's own row: the only slots it ever writes
    const StreamCodeRow x{mine};
    const int v0 = blockIdx.y * per_block, v1 = min(n_variants, v0 + per_block);
    for (int v = v0; v < v1; ++v) {
        const PdVariant pv = variants[v];   // (block-uniform)
        const bool patch0 = live && pv.col0 >= 0, patch1 = live && pv.col1 >= 0;
        uint16_t keep0 = 0, keep1 = 0;
        if (patch0) { keep0 = mine[pv.col0]; mine[pv.col0] = static_cast<uint16_t>(pv.code0); }
        if (patch1) { keep1 = mine[pv.col1]; mine[pv.col1] = static_cast<uint16_t>(pv.code1); }
        float p[DMAX];
#pragma unroll
        for (int d = 0; d < DMAX; ++d) p[d] = (live && d < D) ? cm.bias[d] : 0.0f;
        if (live) {
            for (int t0 = 0; t0 < n_trees; t0 += kStreamGroup<DMAX>)
                stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, static_cast<const int32_t *>(nullptr), t0, n_trees, vec_values, p);
            if constexpr (ICE) stream_store_row<DMAX>(ice + (static_cast<size_t>(slots[v]) * m + row) * D, D, vec_ice != 0, p);
        }
        pd_store_partials<DMAX>(p, D, live, lane == 0, part + static_cast<size_t>(v) * D * nb, nb, static_cast<int>(blockIdx.x));
        if (patch1) mine[pv.col1] = keep1;   // (distinct columns: the order does not matter)
        if (patch0) mine[pv.col0] = keep0;
    }
}

template <int DMAX, bool GREEDY, bool ICE>
bool launch_pd_rows(const ChainModel &cm, const PredictModel &pm, const CodeRows &cr, int m, int n_trees, const PdVariant *variants, const int32_t *slots,
                    int n_variants, double *part, float *ice, hipStream_t s) {
    const size_t lds = stream_code_tile_bytes(cr.groups);
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_pd_rows<DMAX, GREEDY, ICE>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_ice = d4 && (reinterpret_cast<uintptr_t>(ice) & 15) == 0;   // (every row of every slot then starts at a multiple of 16 bytes)
    const int nb = pd_partials(m);
    const int per_block = pd_variants_per_block(nb, n_variants, stream_cu_count());
    hipLaunchKernelGGL((k_pd_rows<DMAX, GREEDY, ICE>), dim3(nb, (n_variants + per_block - 1) / per_block), dim3(kStreamRows), lds, s, cm, stream_owner<DMAX>(pm),
                       pm.coef_cover, cr, m, n_trees, variants, slots, n_variants, per_block, part, nb, ice, vec_values, vec_ice);
    return true;
}

template <bool ICE>
void pd_rows_dispatch(const ChainModel &cm, const PredictModel &pm, const CodeRows &cr, int m, int n_trees, const PdVariant *variants, const int32_t *slots,
                      int n_variants, double *part, float *ice, bool generic, hipStream_t s) {
    if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_pd_rows<DMAX, false, ICE>(cm, pm, cr, m, n_trees, variants, slots, n_variants, part, ice, s)
                                : launch_pd_rows<DMAX, true, ICE>(cm, pm, cr, m, n_trees, variants, slots, n_variants, part, ice, s);
        }))
        return;
    with_general_dmax(pm.D, [&](auto dmax) {
        const int row_blocks = (m + 255) / 256;
        const int per_block = pd_variants_per_block(row_blocks, n_variants, stream_cu_count());
        hipLaunchKernelGGL((k_pd_rows_general<decltype(dmax)::value, ICE>), dim3(row_blocks, (n_variants + per_block - 1) / per_block), dim3(256), 0, s, cm, cr, m,
                           n_trees, variants, slots, n_variants, per_block, part, pd_partials(m), ice);
    });
}

}  // namespace

void pd_rows(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int n_trees, const PdVariant *variants, const int32_t *slots, int n_variants,
             double *part, float *ice, bool generic, hipStream_t s) {
    if (m <= 0 || n_variants <= 0) return;
    // the model view of the float walk with the threshold words replaced by bins, as predict_continue_codes builds it
    ChainModel cm = chain_model(pm);
    cm.walk.cond_pack = ct.cond_pack;
    cm.walk.grd_nodes = ct.grd_nodes;
    cm.walk.feature_bins = ct.bins;
    if (ice != nullptr) pd_rows_dispatch<true>(cm, pm, cr, m, n_trees, variants, slots, n_variants, part, ice, generic, s);
    else pd_rows_dispatch<false>(cm, pm, cr, m, n_trees, variants, slots, n_variants, part, ice, generic, s);
}

}  // namespace kern
}  // namespace gbrl
