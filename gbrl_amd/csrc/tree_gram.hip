// tree_gram.hip -- gfx950 kernels behind GBRL::tree_gram_prepared: the Gram matrix of the per-tree outputs over the rows of a prepared data set and
// their moments against a target (gram_core.h has the rule, the plan and the error argument).  The walk is predict_rowwalk.h's; what is new is
// that its result feeds the matrix cores: v_mfma_f64_16x16x4_f64.
//
//   k_tree_gram<GREEDY>    grid (row_blocks, chunk pairs a <= b), 4 waves per block.  A block takes the 64-row tiles blockIdx.x, + gridDim.x, ...;
//                          wave 0 stages the code tile as the family does (32-byte records, odd word stride, rows= gather).  Then every wave
//                          walks 16 of chunk a's 64 trees (and 16 of chunk b's when a != b) to leaf indices in registers, lane = row.
//                          K = 64 rows x D outputs is consumed in D slabs of one output each: for slab d a lane converts values[leaf][d] of its
//                          16 (+16) trees to float64 -- exact -- and writes them to the operand op[tree][row], kGramOpStride = 65 doubles per
//                          tree.  A lane without a row and a tree beyond the range write 0.0: the K tail and the T tail are zeros in LDS, and no
//                          slab has a K that is not a multiple of 4.  The write is 64 consecutive doubles per tree; the MFMA operand read
//                          (lane -> tree lane % 16, k = k0 + lane / 16) meets word banks 2 * tree + 2 * (lane / 16) (mod 32): each group of 16
//                          lanes covers the 32 banks once.
//                          Wave w owns the block row w of the 4 x 4 grid of 16 x 16 outputs: per k step one A read, four B reads, four MFMAs;
//                          16 steps per slab, the accumulators (16 doubles per lane) live across all tiles of the block.  On a diagonal pair
//                          the B operand is the A operand, and -- with targets -- a fifth MFMA multiplies by a 16-wide block whose first column
//                          is the slab of y: the moments come out of the same instruction, in the first column.  C layout of the instruction:
//                          register v of lane l is C[4 v + l / 16][l % 16].
//                          The block stores its tile to scratch[blockIdx.x][pair]; a non-finite value or target sets a bit of the status word
//                          (an integer OR: no floating-point atomic anywhere).
//   k_tree_gram_general    one thread per (t, u) of the pair tiles and row block, rows read in place (GeneralCodeRow), the reference's walk, no
//                          LDS, no MFMA: a tile too wide for the LDS, a model that is not streamable, a refused opt-in, GBRL_HIP_GRAM_GENERIC=1.
//                          It fills the same scratch.
//   k_gram_reduce          the partials summed in row-block order, one thread per entry: two calls, the same bytes.
#include "gram_core.h"
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {

namespace {

static_assert(kGramTileRows == kStreamRows && kGramLdsBudget == kStreamLdsBudget, "gram_core.h restates the family's constants for the host");

typedef double gram_acc_t __attribute__((ext_vector_type(4)));
constexpr int kGramWaves = kGramChunk / 16;   // a wave per block row of the pair tile
constexpr int kGramWalk = 16;                 // trees a wave walks per chunk

__device__ __forceinline__ int gram_row_of(const CodeRows &cr, int j) { return cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j; }

// the pair (a, b), a <= b, at position p of gram_pair_index's order
__device__ __forceinline__ void gram_pair_of(int p, int chunks, int &a, int &b) {
    a = 0;
    while (p >= chunks - a) { p -= chunks - a; ++a; }
    b = a + p;
}

struct GramIo {
    const float *values;   // [n_leaves][D]
    const float *y;        // [m][D], indexed by the sample, or null
    double *part;          // [row_blocks][per_block]
    int *status;
    int D, T, chunks, pairs;
    size_t per_block;
};

template <bool GREEDY>
__global__ __launch_bounds__(kGramWaves * kWave) void k_tree_gram(LeavesModel lm, CodeRows cr, int m, int n_tiles, int start_tree, GramIo io, int n_ops) {
    extern __shared__ __align__(16) uint32_t tg_lds[];   // [64][stream_code_stride(G)] words | n_ops x [64][65] doubles | [64] doubles
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int ws = stream_code_stride(cr.groups);
    double *op_a = reinterpret_cast<double *>(tg_lds + static_cast<size_t>(kStreamRows) * ws);   // (64 * ws words: a multiple of 256 bytes)
    double *op_b = op_a + kGramChunk * kGramOpStride;
    double *ys = op_a + static_cast<size_t>(n_ops) * kGramChunk * kGramOpStride;
    int a, b;
    gram_pair_of(blockIdx.y, io.chunks, a, b);
    const bool diag = a == b, with_y = diag && io.y != nullptr;   // (block-uniform)
    const int D = io.D, ta = a * kGramChunk + wave * kGramWalk, tb = b * kGramChunk + wave * kGramWalk;
    const int row16 = lane & 15, kq = lane >> 4;
    gram_acc_t acc[4], accm;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = gram_acc_t{0.0, 0.0, 0.0, 0.0};
    accm = gram_acc_t{0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (block-uniform)
        const int r0 = tile * kStreamRows;
        const int rows = min(kStreamRows, m - r0);
        const bool live = lane < rows;
        __syncthreads();   // the previous tile and its last slab have been read
        if (wave == 0) {
            const int my_row = gram_row_of(cr, r0 + (live ? lane : 0));   // (a lane without a row names the tile's first: a valid record, never used)
            stream_stage_code_tile(tg_lds, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
        }
        __syncthreads();
        const StreamCodeRow x{reinterpret_cast<const uint16_t *>(tg_lds + (live ? lane : 0) * ws)};
        int la[kGramWalk], lb[kGramWalk];
#pragma unroll
        for (int g = 0; g < kGramWalk; ++g) {
            la[g] = (live && ta + g < io.T) ? stream_leaf<GREEDY>(lm, x, static_cast<const int32_t *>(nullptr), start_tree + ta + g) : -1;
            lb[g] = -1;
        }
        if (!diag) {
#pragma unroll
            for (int g = 0; g < kGramWalk; ++g)
                lb[g] = (live && tb + g < io.T) ? stream_leaf<GREEDY>(lm, x, static_cast<const int32_t *>(nullptr), start_tree + tb + g) : -1;
        }
        for (int d = 0; d < D; ++d) {   // the K slabs
#pragma unroll
            for (int g = 0; g < kGramWalk; ++g) {
                float f = 0.0f;
                if (la[g] >= 0) {
                    f = io.values[static_cast<size_t>(la[g]) * D + d];
                    if (!isfinite(f)) bad |= kGramBadValue;
                }
                op_a[(wave * kGramWalk + g) * kGramOpStride + lane] = static_cast<double>(f);
            }
            if (!diag) {
#pragma unroll
                for (int g = 0; g < kGramWalk; ++g) {
                    float f = 0.0f;
                    if (lb[g] >= 0) {
                        f = io.values[static_cast<size_t>(lb[g]) * D + d];
                        if (!isfinite(f)) bad |= kGramBadValue;
                    }
                    op_b[(wave * kGramWalk + g) * kGramOpStride + lane] = static_cast<double>(f);
                }
            }
            if (with_y && wave == 0) {
                const float f = live ? io.y[(static_cast<size_t>(r0) + lane) * D + d] : 0.0f;
                if (!isfinite(f)) bad |= kGramBadTarget;
                ys[lane] = static_cast<double>(f);
            }
            __syncthreads();
            const double *pa = op_a + (wave * 16 + row16) * kGramOpStride + kq;
            const double *pb = (diag ? op_a : op_b) + row16 * kGramOpStride + kq;
#pragma unroll 4
            for (int k0 = 0; k0 < kGramTileRows; k0 += 4) {
                const double av = pa[k0];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[j * 16 * kGramOpStride + k0], acc[j], 0, 0, 0);
                if (with_y) accm = __builtin_amdgcn_mfma_f64_16x16x4f64(av, row16 == 0 ? ys[k0 + kq] : 0.0, accm, 0, 0, 0);
            }
            __syncthreads();   // the operands are rewritten by the next slab
        }
    }
    double *part = io.part + static_cast<size_t>(blockIdx.x) * io.per_block;
    double *tile_out = part + static_cast<size_t>(blockIdx.y) * kGramChunk * kGramChunk;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) tile_out[(wave * 16 + 4 * v + kq) * kGramChunk + j * 16 + row16] = acc[j][v];
    if (with_y && row16 == 0) {
        double *mo = part + static_cast<size_t>(io.pairs) * kGramChunk * kGramChunk + a * kGramChunk;
#pragma unroll
        for (int v = 0; v < 4; ++v) mo[wave * 16 + 4 * v + kq] = accm[v];
    }
    if (bad) atomicOr(io.status, bad);
}

// one thread per entry of the pair tiles (grid.x) and row block (grid.y): the rows [m rb / RB, m (rb + 1) / RB) in order
__global__ __launch_bounds__(256) void k_tree_gram_general(LeavesModel lm, CodeRows cr, int m, int start_tree, GramIo io) {
    const size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t n_entries = static_cast<size_t>(io.pairs) * kGramChunk * kGramChunk;
    if (idx >= n_entries) return;
    const int i = static_cast<int>((idx >> 6) & 63), j = static_cast<int>(idx & 63);
    int a, b;
    gram_pair_of(static_cast<int>(idx >> 12), io.chunks, a, b);
    const int t = a * kGramChunk + i, u = b * kGramChunk + j, D = io.D;
    const int rb = blockIdx.y, RB = gridDim.y;
    const int lo = static_cast<int>(static_cast<long long>(m) * rb / RB), hi = static_cast<int>(static_cast<long long>(m) * (rb + 1) / RB);
    const bool wanted = t < io.T && u < io.T && u >= t, with_y = io.y != nullptr && a == b && i == j;
    double s = 0.0, sm = 0.0;
    int bad = 0;
    if (wanted) {
        for (int r = lo; r < hi; ++r) {
            const GeneralCodeRow row{cr.codes + static_cast<size_t>(gram_row_of(cr, r)) * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
            const int lt = general_leaf(lm, row, start_tree + t);
            const int lu = u == t ? lt : general_leaf(lm, row, start_tree + u);
            if (lt < 0) continue;
            const float *vt = io.values + static_cast<size_t>(lt) * D;
            if (lu >= 0) {
                const float *vu = io.values + static_cast<size_t>(lu) * D;
                for (int d = 0; d < D; ++d) {
                    if (!isfinite(vt[d]) || !isfinite(vu[d])) bad |= kGramBadValue;
                    s += static_cast<double>(vt[d]) * static_cast<double>(vu[d]);
                }
            }
            if (with_y) {
                const float *yr = io.y + static_cast<size_t>(r) * D;
                for (int d = 0; d < D; ++d) {
                    if (!isfinite(yr[d])) bad |= kGramBadTarget;
                    sm += static_cast<double>(vt[d]) * static_cast<double>(yr[d]);
                }
            }
        }
    }
    double *part = io.part + static_cast<size_t>(rb) * io.per_block;
    part[idx] = s;
    if (with_y) part[n_entries + a * kGramChunk + i] = sm;   // (every moment slot, the T tail included: zero there)
    if (bad) atomicOr(io.status, bad);
}

__global__ __launch_bounds__(256) void k_gram_reduce(const double *__restrict__ part, int row_blocks, size_t per_block, size_t n, double *__restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int rb = 0; rb < row_blocks; ++rb) s += part[static_cast<size_t>(rb) * per_block + i];
    out[i] = s;
}

template <bool GREEDY>
bool launch_tree_gram(const LeavesModel &lm, const CodeRows &cr, int m, int start_tree, const GramPlan &p, const GramIo &io, hipStream_t s) {
    static StreamLdsOptIn optin;
    if (!optin.ok(k_tree_gram<GREEDY>, p.lds_bytes)) return false;
    hipLaunchKernelGGL((k_tree_gram<GREEDY>), dim3(p.row_blocks, p.pairs), dim3(kGramWaves * kWave), p.lds_bytes, s, lm, cr, m, p.tiles, start_tree, io,
                       p.chunks > 1 ? 2 : 1);
    return true;
}

}  // namespace

bool tree_gram_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int start_tree, int stop_tree, const float *targets,
                     double *part, double *tiles, int *status, bool generic, hipStream_t s) {
    const int T = stop_tree - start_tree;
    const GramPlan p = gram_plan(m, T, pm.D, cr.groups);
    // the model view of the float walk with the threshold words replaced by bins (predict_continue_codes' rule)
    LeavesModel lm = leaves_model(pm);
    lm.cond_pack = ct.cond_pack;
    lm.grd_nodes = ct.grd_nodes;
    lm.feature_bins = ct.bins;
    const GramIo io{pm.values, targets, part, status, pm.D, T, p.chunks, p.pairs, p.per_block};
    bool streamed = false;
    if (p.streaming && leaves_streamable(pm, generic))
        streamed = pm.oblivious ? launch_tree_gram<false>(lm, cr, m, start_tree, p, io, s) : launch_tree_gram<true>(lm, cr, m, start_tree, p, io, s);
    const size_t n_entries = static_cast<size_t>(p.pairs) * kGramChunk * kGramChunk;
    if (!streamed)
        hipLaunchKernelGGL(k_tree_gram_general, dim3(static_cast<unsigned>((n_entries + 255) / 256), p.row_blocks), dim3(256), 0, s, lm, cr, m, start_tree, io);
    const size_t n_out = targets ? p.per_block : n_entries;   // (without targets nobody wrote the moment slots)
    hipLaunchKernelGGL(k_gram_reduce, dim3(static_cast<unsigned>((n_out + 255) / 256)), dim3(256), 0, s, part, p.row_blocks, p.per_block, n_out, tiles);
    return streamed;
}

}  // namespace kern
}  // namespace gbrl
