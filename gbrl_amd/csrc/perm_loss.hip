// perm_loss.hip -- gfx950 kernels behind GBRL::permutation_importance_prepared: the loss of many "one column shuffled" variants of a prepared data
// set's rows, none of them materialised.  A variant (col, repeat) reads column col of row i from row pi(i), pi = perm(n, seed, col, repeat) of
// perm_core.h, and every other column from row i; col < 0 is the data set as it is.  The walk, the grouping of trees, the rates and the owner rule
// are predict_rowwalk.h's, the row losses and the wave sum predict_loss.h's: a variant's partials are the bits predict_continue_codes.hip's loss
// tail writes for a data set that holds the shuffled column, one float64 per 64 rows.
//
//   k_perm_loss          lane = row, one wave per block, k_continue_codes' LDS tile.  The block's 64 code records are staged ONCE
//                        (stream_stage_code_tile); then for every variant of the block's list the lane gathers codes[col >> 4][pi(row)][col & 15] --
//                        one 2-byte load -- into its own row's slot of the tile, walks the trees from the bias (stream_chain_group), sums the
//                        objective's row loss over the wave (staged_wave_sum), stores loss_part[variant][block] and puts the original code back.  A
//                        lane touches only its own row's slot and the block is one wave: no barrier between variants.  The targets of an rmse row
//                        stay in registers across the variants.
//   k_perm_loss_general  one thread per row, the records read in place through PermutedCodeRow (the gathered code answers for column col): D in
//                        65..128, optimizers that share outputs, a greedy depth-0 tree, F too wide for the tile, a refused LDS opt-in, and the
//                        cross-check behind GBRL_HIP_PERM_GENERIC=1.  Four waves per block: four partials.
//   the block's list     grid.y cuts the launch's variants into runs of per_block: 1 run when the rows alone fill the device (the tile is then read
//                        from HBM once per launch), more when they do not (few rows: the variants are the parallelism).
// Nothing is stored but the partials: no prediction, no gradient, and the data set's codes are only ever read.
#include "kernels.h"
#include "kernels_common.h"
#include "perm_core.h"
#include "predict_rowwalk.h"
#include "predict_loss.h"

namespace gbrl {
namespace kern {

namespace {

// a row of a prepared data set with ONE column answered from elsewhere: GeneralCodeRow beside it in predict_rowwalk.h reads every column in place
struct PermutedCodeRow {
    const uint16_t *rec;
    size_t group_stride;
    int col, code;   // col < 0: no column is replaced
    __device__ __forceinline__ bool numeric(const LeavesModel &cm, int f, int c) const {
        const int v = f == col ? code : static_cast<int>(rec[static_cast<size_t>(f >> 4) * group_stride + (f & 15)]);
        return v > cm.feature_bins[c];
    }
    __device__ __forceinline__ bool categorical(const LeavesModel &, int, int) const { return false; }
};

// the code of column col (>= 0) that row `row` of a variant reads
__device__ __forceinline__ uint16_t perm_gather(const uint16_t *__restrict__ codes, int n, uint64_t seed, const PermVariant &pv, uint32_t row) {
    const PermPlan pp = perm_plan(static_cast<uint32_t>(n), seed, pv.col, pv.repeat);
    const size_t src = perm_at(pp, row);
    return codes[(static_cast<size_t>(pv.col >> 4) * static_cast<size_t>(n) + src) * kCodeGroup + (pv.col & 15)];
}

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX, int OBJ>
__global__ __launch_bounds__(256) void k_perm_loss_general(ChainModel cm, const uint16_t *__restrict__ codes, int n, int n_trees, const float *__restrict__ targets,
                                                           const float *__restrict__ alpha, uint64_t seed, const PermVariant *__restrict__ variants,
                                                           int n_variants, int per_block, double *__restrict__ loss_part, int nb) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < n;   // (whole waves stay for the butterfly)
    const int D = cm.D;
    const int wave = j / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
    const int v0 = blockIdx.y * per_block, v1 = min(n_variants, v0 + per_block);
    for (int v = v0; v < v1; ++v) {
        const PermVariant pv = variants[v];
        double acc = 0.0;
        if (live) {
            float p[DMAX];
#pragma unroll
            for (int d = 0; d < DMAX; ++d) p[d] = d < D ? cm.bias[d] : 0.0f;
            const int code = pv.col >= 0 ? static_cast<int>(perm_gather(codes, n, seed, pv, static_cast<uint32_t>(j))) : 0;
            const PermutedCodeRow r{codes + static_cast<size_t>(j) * kCodeGroup, static_cast<size_t>(n) * kCodeGroup, pv.col, code};
            for (int t = 0; t < n_trees; ++t)
                if (!general_chain_tree<DMAX>(cm, r, t, p)) break;   // a greedy search ran off the ensemble: the walk ends
            if constexpr (OBJ == kObjRmse) acc = staged_row_loss<DMAX>(p, targets + static_cast<size_t>(j) * D, D);
            else acc = objective_loss_regs<OBJ, DMAX>(p, p, objective_target_row<OBJ>(targets, j, D), D, false, alpha);   // (the row itself stands in for a stored one)
        }
        acc = staged_wave_sum(acc);
        if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < nb) loss_part[static_cast<size_t>(v) * nb + wave] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, int OBJ>
__global__ __launch_bounds__(kStreamRows) void k_perm_loss(ChainModel cm, StreamOwner<DMAX> own, uint64_t cover, const uint16_t *__restrict__ codes, int n, int groups,
                                                           int n_trees, const float *__restrict__ targets, const float *__restrict__ alpha, uint64_t seed,
                                                           const PermVariant *__restrict__ variants, int n_variants, int per_block, double *__restrict__ loss_part,
                                                           int nb, int vec_values, int vec_loss) {
    extern __shared__ __align__(16) uint32_t pltile[];   // [kStreamRows][stream_code_stride(G)]
    const int lane = threadIdx.x;
    const int D = cm.D;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, n - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    const int my_row = r0 + (live ? lane : 0);   // (a lane without a row names the block's first: a valid record, never read back)
    stream_stage_code_tile(pltile, codes, static_cast<size_t>(n), groups, my_row, rows, lane);
    __syncthreads();
    uint16_t *mine = reinterpret_cast<uint16_t *>(pltile + lane * stream_code_stride(groups));   // the lane's own row: the only slots it ever writes
    const StreamCodeRow x{mine};
    float y[OBJ == kObjRmse ? DMAX : 1];
    if constexpr (OBJ == kObjRmse) {
        if (live) {
            stream_load_row<DMAX>(targets + row * D, D, vec_loss != 0, y);
        } else {
#pragma unroll
            for (int d = 0; d < DMAX; ++d) y[d] = 0.0f;
        }
    }
    const int v0 = blockIdx.y * per_block, v1 = min(n_variants, v0 + per_block);
    for (int v = v0; v < v1; ++v) {
        const PermVariant pv = variants[v];   // (block-uniform)
        const bool patch = live && pv.col >= 0;
        uint16_t keep = 0;
        if (patch) {
            keep = mine[pv.col];
            mine[pv.col] = perm_gather(codes, n, seed, pv, static_cast<uint32_t>(row));
        }
        double acc = 0.0;
        if (live) {
            float p[DMAX];
#pragma unroll
            for (int d = 0; d < DMAX; ++d) p[d] = d < D ? cm.bias[d] : 0.0f;
            for (int t0 = 0; t0 < n_trees; t0 += kStreamGroup<DMAX>)
                stream_chain_group<DMAX, GREEDY>(cm, own, cover, x, static_cast<const int32_t *>(nullptr), t0, n_trees, vec_values, p);
            if constexpr (OBJ == kObjRmse) acc = staged_row_loss<DMAX>(p, y, D);
            else acc = objective_loss_regs<OBJ, DMAX>(p, p, objective_target_row<OBJ>(targets, row, D), D, vec_loss != 0, alpha);
        }
        acc = staged_wave_sum(acc);
        if (lane == 0) loss_part[static_cast<size_t>(v) * nb + blockIdx.x] = acc;
        if (patch) mine[pv.col] = keep;
    }
}

// runs of variants per launch: one when the row blocks alone give every CU four blocks, more when they do not
int perm_variants_per_block(int row_blocks, int n_variants) {
    const int want = 4 * stream_cu_count();
    const int runs = std::min(n_variants, std::max(1, (want + row_blocks - 1) / row_blocks));
    return (n_variants + runs - 1) / runs;
}

template <int DMAX, bool GREEDY, int OBJ>
bool launch_perm_loss(const ChainModel &cm, const PredictModel &pm, const uint16_t *codes, int n, int groups, int n_trees, const float *targets, const float *alpha,
                      uint64_t seed, const PermVariant *variants, int n_variants, double *loss_part, hipStream_t s) {
    static_assert(kStreamRows == kStagedRows, "a block of the streaming kernel writes exactly one loss partial");
    const size_t lds = stream_code_tile_bytes(groups);
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_perm_loss<DMAX, GREEDY, OBJ>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_loss = d4 && (reinterpret_cast<uintptr_t>(targets) & 15) == 0;   // (softmax loads no vector)
    const int nb = staged_loss_partials(n);
    const int per_block = perm_variants_per_block(nb, n_variants);
    hipLaunchKernelGGL((k_perm_loss<DMAX, GREEDY, OBJ>), dim3(nb, (n_variants + per_block - 1) / per_block), dim3(kStreamRows), lds, s, cm, stream_owner<DMAX>(pm),
                       pm.coef_cover, codes, n, groups, n_trees, targets, alpha, seed, variants, n_variants, per_block, loss_part, nb, vec_values, vec_loss);
    return true;
}

}  // namespace

int perm_tile_rows() { return kStreamRows; }

void perm_loss(const PredictModel &pm, const CodeTables &ct, const uint16_t *codes, int n, int groups, int n_trees, int objective, const float *targets,
               const float *alpha, uint64_t seed, const PermVariant *variants, int n_variants, double *loss_part, bool generic, hipStream_t s) {
    if (n <= 0 || n_variants <= 0) return;
    // the model view of the float walk with the threshold words replaced by bins, as predict_continue_codes builds it
    ChainModel cm = chain_model(pm);
    cm.walk.cond_pack = ct.cond_pack;
    cm.walk.grd_nodes = ct.grd_nodes;
    cm.walk.feature_bins = ct.bins;
    with_objective(objective, [&](auto obj) {
        constexpr int OBJ = decltype(obj)::value;
        if (chain_streamable(pm, generic) && with_stream_dmax(pm.D, [&](auto dmax) {
                constexpr int DMAX = decltype(dmax)::value;
                return pm.oblivious ? launch_perm_loss<DMAX, false, OBJ>(cm, pm, codes, n, groups, n_trees, targets, alpha, seed, variants, n_variants, loss_part, s)
                                    : launch_perm_loss<DMAX, true, OBJ>(cm, pm, codes, n, groups, n_trees, targets, alpha, seed, variants, n_variants, loss_part, s);
            }))
            return;
        with_general_dmax(pm.D, [&](auto dmax) {
            const int row_blocks = (n + 255) / 256;
            const int per_block = perm_variants_per_block(row_blocks, n_variants);
            hipLaunchKernelGGL((k_perm_loss_general<decltype(dmax)::value, OBJ>), dim3(row_blocks, (n_variants + per_block - 1) / per_block), dim3(256), 0, s, cm, codes,
                               n, n_trees, targets, alpha, seed, variants, n_variants, per_block, loss_part, staged_loss_partials(n));
        });
    });
}

}  // namespace kern
}  // namespace gbrl
