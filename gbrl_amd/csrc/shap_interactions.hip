// shap_interactions.hip -- gfx950 kernels behind GBRL::shap_interactions_prepared / GBRL::shap_interaction_importance_prepared: exact SHAP interaction
// values (shapx_core.h has the rule and fixes every operation's order) of a prepared data set's rows.  The work per (row, tree) is cubic in the path
// length, but the row enters a leaf's term only through the PATTERN o -- one bit per merged feature of the leaf's path -- so the cubic part is done
// once per (leaf, pattern) and a row only looks its weights up and adds.
//
//   k_shapx_table     one block per leaf, one thread per pattern: shapx_leaf_weights (extend / unwind, O(n^3)) into table[leaf.tab + o * len(n) + item],
//                     len(n) = n + n (n - 1) / 2 weights (the n SHAP weights a_i, then the pair weights w_ij).  Row-independent: 4^depth threads per
//                     oblivious tree, not rows x leaves.
//   k_shapx_rows      a block of 256 threads owns `rows` consecutive positions of the row list (shapx_plan: as many as fit, at most 64).  Their 64 code
//                     records are staged ONCE by the first wave (stream_stage_code_tile).  LDS behind them: phi[row][K][K][D] float64, the rows'
//                     results; T[row][nt][nt][D] float64, the matrix of the tree at hand over that tree's own nt features; a pattern word and the
//                     decision bits per row.  Per tree: T is zeroed, an oblivious tree's decision bits are computed once per row (stream_leaf); then
//                     leaf by leaf, ascending: (A) thread r < rows writes the pattern of its row for the leaf -- from the decision bits (oblivious) or the
//                     code tile (greedy) -- (B) the ITEMS (row, weight p, output d) of the leaf are spread over the threads: one table read, one leaf
//                     value, T[a][b][d] += v * w and its mirror.  The items of a leaf touch distinct words, the leaves are separated by barriers: no
//                     atomics, and the order of the adds into a word is the leaf order whatever the scheduling.  After the last leaf thread (row, a, d)
//                     takes row a of T: the diagonal (shapx_core.h's order), then phi += T.  After the last tree the block stores float(phi),
//                     consecutive threads on consecutive words of the row-major result.
//   k_shapx_general   one thread per row, shapx_row (the host's function) on float64 scratch in global memory, the records read in place
//                     (GeneralCodeRow): whatever shapx_plan declines, a refused LDS opt-in, and the cross-check behind GBRL_HIP_SHAPX_GENERIC=1.
// No matrix instructions: the work is table look-ups and scalar float64 adds in a fixed order.  Stored: the table, the scratch, the result.  The data
// set's codes and the model are only ever read.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"
#include "shapx_core.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kShapxThreads = 256;
static_assert(kShapxStreamRows == kStreamRows, "the first wave stages one row per lane");

__host__ __device__ inline ShapxView shapx_view(const LeavesModel &cm, const float *values, int n_trees_model, int D, const ShapxTables &st) {
    return ShapxView{cm.tree_indices, cm.depths, cm.feature_indices, cm.inequality_directions, values, st.leaf, st.mslot, st.mz, st.cond_e, st.tree, st.tmap,
                     st.wtab, cm.n_leaves, n_trees_model, cm.max_depth, D, st.K, cm.oblivious};
}

// ------------------------------------------------------------------------------------------------------------ the weight table
__global__ __launch_bounds__(64) void k_shapx_table(ShapxTables st) {
    const ShapxLeafRec rec = st.leaf[blockIdx.x];
    if (rec.n == 0 || rec.tab < 0) return;
    const int len = shapx_weights_len(rec.n);
    for (uint32_t o = threadIdx.x; o < (1u << rec.n); o += blockDim.x)
        shapx_leaf_weights(rec.n, st.mz + rec.first, o, st.wtab, st.table + rec.tab + static_cast<size_t>(o) * len);
}

// ------------------------------------------------------------------------------------------------------------ general kernel
__global__ __launch_bounds__(256) void k_shapx_general(LeavesModel cm, const float *values, int n_trees_model, int D, ShapxTables st, CodeRows cr, int m, int n_trees,
                                                       size_t row_doubles, double *scratch, float *out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j);
    const GeneralCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const ShapxView v = shapx_view(cm, values, n_trees_model, D, st);
    const size_t KKD = static_cast<size_t>(st.K) * st.K * D;
    double *phi = scratch + static_cast<size_t>(j) * row_doubles, *T = phi + KKD, *w = T + static_cast<size_t>(st.nt_max) * st.nt_max * D;
    shapx_row(v, n_trees, [&](int c, int f) { return r.numeric(cm, f, c); }, phi, T, w);
    float *o = out + static_cast<size_t>(j) * KKD;
    for (size_t i = 0; i < KKD; ++i) o[i] = static_cast<float>(phi[i]);
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <bool GREEDY>
__global__ __launch_bounds__(kShapxThreads) void k_shapx_rows(LeavesModel cm, const float *__restrict__ values, int n_trees_model, int D, ShapxTables st, CodeRows cr,
                                                              int m, int n_trees, int block_rows, float *__restrict__ out) {
    extern __shared__ __align__(16) double sx[];   // phi [block_rows][KKD], T [block_rows][TT], then uint32: the code tile, pat [64], bits [64]
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * block_rows;
    const int rows = min(block_rows, m - r0);
    const int KKD = st.K * st.K * D, TT = st.nt_max * st.nt_max * D, md = cm.max_depth;
    double *phi = sx, *Tm = sx + static_cast<size_t>(block_rows) * KKD;
    uint32_t *tile = reinterpret_cast<uint32_t *>(Tm + static_cast<size_t>(block_rows) * TT);
    const int ws = stream_code_stride(cr.groups);
    uint32_t *pat = tile + kStreamRows * ws, *bits = pat + kStreamRows;
    if (tid < kStreamRows) {   // the first wave stages the tile: lane j the records of position r0 + j
        const int at = cr.row0 + r0 + (tid < rows ? tid : 0);
        const int my_row = cr.rows ? cr.rows[at] : at;
        stream_stage_code_tile(tile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, tid);
    }
    for (int i = tid; i < rows * KKD; i += kShapxThreads) phi[i] = 0.0;
    __syncthreads();
    const StreamCodeRow x{reinterpret_cast<const uint16_t *>(tile + (tid < rows ? tid : 0) * ws)};
    for (int t = 0; t < n_trees; ++t) {
        const ShapxTreeRec tr = st.tree[t];
        const int nt = tr.nt;
        if (nt == 0) continue;   // (block-uniform)
        const int tt = nt * nt * D, l0 = cm.tree_indices[t], l1 = t + 1 < n_trees_model ? cm.tree_indices[t + 1] : cm.n_leaves;
        for (int i = tid; i < rows * tt; i += kShapxThreads) Tm[(i / tt) * TT + i % tt] = 0.0;
        if (!GREEDY && tid < rows) bits[tid] = static_cast<uint32_t>(stream_leaf<false>(cm, x, static_cast<const int32_t *>(nullptr), t) - l0);
        __syncthreads();
        for (int leaf = l0; leaf < l1; ++leaf) {
            const ShapxLeafRec rec = st.leaf[leaf];
            const int n = rec.n;
            if (n == 0) continue;   // (block-uniform)
            if (tid < rows) {       // (A) the pattern of row tid for this leaf
                const size_t crow = GREEDY ? static_cast<size_t>(leaf) : static_cast<size_t>(t);
                const int depth = cm.depths[crow];
                uint32_t o = (1u << n) - 1u;
                if (!GREEDY) {
                    const uint32_t differ = bits[tid] ^ static_cast<uint32_t>(leaf - l0);
                    for (int d = 0; d < depth; ++d)
                        if ((differ >> (depth - 1 - d)) & 1u) o &= ~(1u << st.cond_e[static_cast<size_t>(leaf) * md + d]);
                } else {
                    for (int d = 0; d < depth; ++d) {
                        const size_t c = crow * md + d;
                        const bool pass = stream_numeric(x, cm.feature_indices[c], cm.feature_bins[c]);
                        if (pass != (cm.inequality_directions[c] != 0)) o &= ~(1u << st.cond_e[c]);
                    }
                }
                pat[tid] = o;
            }
            __syncthreads();
            const int len = shapx_weights_len(n), per_row = len * D;
            const uint16_t *ent = st.ent + st.ent_first[leaf];
            const double *tab = st.table + rec.tab;
            const float *val = values + static_cast<size_t>(leaf) * D;
            for (int i = tid; i < rows * per_row; i += kShapxThreads) {   // (B) items (row, weight, output)
                const int r = i / per_row, q = i - r * per_row, p = q / D, d = q - p * D;
                const double w = tab[static_cast<size_t>(pat[r]) * len + p], v = static_cast<double>(val[d]);
                const int a = ent[p] >> 8, b = ent[p] & 255;
                double *T = Tm + static_cast<size_t>(r) * TT;
                T[(a * nt + b) * D + d] = shapx_add(T[(a * nt + b) * D + d], v, w);
                if (a != b) T[(b * nt + a) * D + d] = shapx_add(T[(b * nt + a) * D + d], v, w);
            }
            __syncthreads();
        }
        // the tree's last leaf is in: thread (row, a, d) owns row a of T and of phi (shapx_finish_tree's order)
        const int32_t *km = st.tmap + tr.first;
        for (int i = tid; i < rows * nt * D; i += kShapxThreads) {
#pragma clang fp contract(off)
            const int r = i / (nt * D), q = i - r * nt * D, a = q / D, d = q - a * D;
            double *T = Tm + static_cast<size_t>(r) * TT;
            double dg = T[(a * nt + a) * D + d];
            for (int b = 0; b < nt; ++b)
                if (b != a) dg = dg - T[(a * nt + b) * D + d];
            double *ph = phi + static_cast<size_t>(r) * KKD + static_cast<size_t>(km[a]) * st.K * D;
            for (int b = 0; b < nt; ++b) {
                double *p = ph + km[b] * D + d;
                *p = *p + (b == a ? dg : T[(a * nt + b) * D + d]);
            }
        }
        __syncthreads();
    }
    float *o = out + static_cast<size_t>(r0) * KKD;
    for (int i = tid; i < rows * KKD; i += kShapxThreads) o[i] = static_cast<float>(phi[i]);
}

template <bool GREEDY>
bool launch_shapx_rows(const LeavesModel &cm, const PredictModel &pm, const ShapxTables &st, const CodeRows &cr, int m, int n_trees, float *out, hipStream_t s) {
    const ShapxPlan plan = shapx_plan(st.K, st.nt_max, st.n_max, cr.groups, pm.D, st.table_doubles);
    if (!plan.fits) return false;
    static StreamLdsOptIn optin;
    if (!optin.ok(k_shapx_rows<GREEDY>, plan.lds)) return false;
    hipLaunchKernelGGL((k_shapx_rows<GREEDY>), dim3((m + plan.rows - 1) / plan.rows), dim3(kShapxThreads), plan.lds, s, cm, pm.values, pm.n_trees, pm.D, st, cr, m,
                       n_trees, plan.rows, out);
    return true;
}

// the model view of the float walk with the threshold words replaced by bins, as predict_continue_codes builds it
LeavesModel code_walk(const PredictModel &pm, const CodeTables &ct) {
    LeavesModel cm = leaves_model(pm);
    cm.cond_pack = ct.cond_pack;
    cm.grd_nodes = ct.grd_nodes;
    cm.feature_bins = ct.bins;
    return cm;
}

}  // namespace

void shapx_build_table(const ShapxTables &st, hipStream_t s) {
    if (st.n_leaves <= 0 || st.table_doubles == 0) return;
    hipLaunchKernelGGL(k_shapx_table, dim3(st.n_leaves), dim3(64), 0, s, st);
}

bool shapx_rows_stream(const PredictModel &pm, const CodeTables &ct, const ShapxTables &st, const CodeRows &cr, int m, int n_trees, float *out, hipStream_t s) {
    if (pm.oblivious && ct.cond_pack == nullptr) return false;
    if (m <= 0) return shapx_plan(st.K, st.nt_max, st.n_max, cr.groups, pm.D, st.table_doubles).fits;
    const LeavesModel cm = code_walk(pm, ct);
    return pm.oblivious ? launch_shapx_rows<false>(cm, pm, st, cr, m, n_trees, out, s) : launch_shapx_rows<true>(cm, pm, st, cr, m, n_trees, out, s);
}

void shapx_rows_general(const PredictModel &pm, const CodeTables &ct, const ShapxTables &st, const CodeRows &cr, int m, int n_trees, double *scratch, float *out,
                        hipStream_t s) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_shapx_general, dim3((m + 255) / 256), dim3(256), 0, s, code_walk(pm, ct), pm.values, pm.n_trees, pm.D, st, cr, m, n_trees,
                       shapx_general_row_doubles(st.K, st.nt_max, st.n_max, pm.D), scratch, out);
}

}  // namespace kern
}  // namespace gbrl
