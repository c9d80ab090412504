// path_rows.hip -- gfx950 kernels behind GBRL::path_contrib_prepared / GBRL::path_importance_prepared: path attribution (path_core.h has the rule)
// of a prepared data set's rows.  A row needs only the leaf it reaches in every tree: the cost is the walk of predict_continue_codes.hip plus, per
// decision on the path, D float32 adds of a delta record -- never the SHAP recursion, and never the [m][F][D] matrix unless the caller asks for it.
// The walk, the code tile and the model view are predict_rowwalk.h's; the float64 tile sums are shap_core.h's.
//
//   k_path_rows          lane = row, one wave per block.  The block's 64 code records are staged ONCE (stream_stage_code_tile; with a row list lane
//                        j stages the records of rows[j]).  Behind the tile the contributions of the tile live in LDS as acc[slot][row][D | 1]
//                        float32: a SLOT is a feature some tree of the range tests (the host compacts them: a column no tree tests costs nothing
//                        and keeps its zeros), the row stride is odd, so the D adds of the 64 lanes to their own rows meet 64 banks.  A PASS
//                        covers as many slots as fit beside the tile in the opt-in LDS (path_slot_plan); when the used features need more, the
//                        trees are walked again over the same staged tile for the next slot group -- an oblivious tree none of whose levels
//                        tests a feature of the group is skipped without its walk (wave-uniform).  A lane zeroes, adds to and -- until the tail --
//                        reads only its own row: no atomics, no barrier inside a pass.  A decision's delta record (D floats of the table
//                        [n_leaves][max_depth][D]) is read through the cache, 16-byte loads when D is a multiple of 4; the records of a tree slice
//                        are NOT staged in LDS (not tried: the LDS goes to the slots).
//   tail of a pass       matrix form: the pass's slots go to phi[row][used[slot]][d], consecutive lanes on consecutive d, then slots, then rows --
//                        the LDS transpose of predict_leaves.hip (phi is zeroed by the caller: unused columns are never written).
//                        importance form (SUMS): lane i reduces one (slot, d) over the tile's rows in row order in float64 (shap_tile_sums) and
//                        writes the two partials part[tile][0 / 1][slot * D + d]; no float32 matrix exists at any point.
//   k_path_rows_general  one thread per row, the records read in place (GeneralCodeRow), general_leaf, plain read-modify-write of the thread's own
//                        row of phi: D in 65..128, a model that is not streamable, a tile too wide for the LDS, a refused opt-in, and the
//                        cross-check behind GBRL_HIP_PATH_GENERIC=1.  Same order of adds, same bytes.
// Stored: phi or the partials.  The data set's codes and the model are only ever read.
#include "kernels.h"
#include "kernels_common.h"
#include "path_core.h"
#include "predict_rowwalk.h"
#include "shap_core.h"

namespace gbrl {
namespace kern {

namespace {

static_assert(kPathRows == kStreamRows && kPathRows == kShapTileRows, "a wave holds the rows of one tile and of one float64 partial");

// ------------------------------------------------------------------------------------------------------------ general kernel
__global__ __launch_bounds__(256) void k_path_rows_general(LeavesModel cm, const float *__restrict__ delta, CodeRows cr, int D, int F, int m, int n_trees,
                                                           float *phi) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j);
    const GeneralCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const int md = cm.max_depth;
    float *o = phi + static_cast<size_t>(j) * F * D;
    for (int t = 0; t < n_trees; ++t) {
        const int leaf = general_leaf(cm, r, t);
        if (leaf < 0) break;   // (a greedy search ran off the ensemble: refused models only)
        const size_t row = cm.oblivious ? static_cast<size_t>(t) : static_cast<size_t>(leaf);
        const int depth = cm.depths[row];
        const float *dl = delta + static_cast<size_t>(leaf) * md * D;
        for (int k = 0; k < depth; ++k) {
            float *a = o + static_cast<size_t>(cm.feature_indices[row * md + k]) * D;
            for (int d = 0; d < D; ++d) a[d] = path_add(a[d], dl[k * D + d]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX, bool GREEDY, bool SUMS>
__global__ __launch_bounds__(kStreamRows) void k_path_rows(LeavesModel cm, PathTables pt, CodeRows cr, int D, int F, int m, int n_trees, int slots,
                                                           float *__restrict__ phi, double *__restrict__ part, int tile0, int vec_delta) {
    extern __shared__ __align__(16) uint32_t ptile[];   // [kStreamRows][stream_code_stride(G)] words, then acc[slots][kStreamRows][D | 1] floats
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, m - r0);
    const bool live = lane < rows;
    const int at = cr.row0 + r0 + (live ? lane : 0);   // (a lane without a row names the block's first: a valid record, never read back)
    const int my_row = cr.rows ? cr.rows[at] : at;
    const int ws = stream_code_stride(cr.groups);
    stream_stage_code_tile(ptile, cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
    __syncthreads();
    const StreamCodeRow x{reinterpret_cast<const uint16_t *>(ptile + lane * ws)};
    float *acc = reinterpret_cast<float *>(ptile + kStreamRows * ws);
    const int RS = path_row_stride(D), md = cm.max_depth;
    float *mine = acc + lane * RS;                      // the lane's row of slot 0; slot s is kStreamRows * RS floats further
    const int slot_floats = kStreamRows * RS;
    for (int s0 = 0; s0 < pt.n_used; s0 += slots) {     // (block-uniform) one pass per slot group
        const int ns = min(slots, pt.n_used - s0);
        for (int s = 0; s < ns; ++s)
            for (int d = 0; d < D; ++d) mine[s * slot_floats + d] = 0.0f;
        if (live) {
            for (int t = 0; t < n_trees; ++t) {
                if (!GREEDY) {   // the tree's levels are the wave's: skip the walk when none of them lands in this pass
                    const int depth = cm.depths[t];
                    bool any = false;
                    for (int k = 0; k < depth; ++k) any = any || static_cast<unsigned>(pt.slot_of[cm.feature_indices[t * md + k]] - s0) < static_cast<unsigned>(ns);
                    if (!any) continue;
                }
                const int leaf = stream_leaf<GREEDY>(cm, x, static_cast<const int32_t *>(nullptr), t);
                const size_t row = GREEDY ? static_cast<size_t>(leaf) : static_cast<size_t>(t);
                const int depth = cm.depths[row];
                const int32_t *fi = cm.feature_indices + row * md;
                const float *dl = pt.delta + static_cast<size_t>(leaf) * md * D;
                for (int k = 0; k < depth; ++k) {
                    const int s = pt.slot_of[fi[k]] - s0;
                    if (static_cast<unsigned>(s) >= static_cast<unsigned>(ns)) continue;
                    float v[DMAX];
                    stream_load_row<DMAX>(dl + k * D, D, vec_delta != 0, v);
                    float *a = mine + s * slot_floats;
#pragma unroll
                    for (int d = 0; d < DMAX; ++d)
                        if (d < D) a[d] = path_add(a[d], v[d]);
                }
            }
        }
        __syncthreads();   // the tail reads the other lanes' rows
        if constexpr (SUMS) {
            const int CU = pt.n_used * D;
            double *dst = part + static_cast<size_t>(tile0 + blockIdx.x) * 2 * CU;
            for (int i = lane; i < ns * D; i += kStreamRows) {
                const int s = i / D, d = i - s * D;
                double sum, sum_abs;
                shap_tile_sums(acc + s * slot_floats + d, static_cast<size_t>(RS), rows, &sum, &sum_abs);
                dst[(s0 + s) * D + d] = sum;
                dst[CU + (s0 + s) * D + d] = sum_abs;
            }
        } else {
            const size_t C = static_cast<size_t>(F) * D;
            float *o = phi + static_cast<size_t>(r0) * C;
            const int per_row = ns * D;
            for (int i = lane; i < rows * per_row; i += kStreamRows) {
                const int r = i / per_row, q = i - r * per_row, s = q / D, d = q - s * D;
                o[r * C + static_cast<size_t>(pt.used[s0 + s]) * D + d] = acc[s * slot_floats + r * RS + d];
            }
        }
        __syncthreads();   // the next pass zeroes the slots
    }
}

template <int DMAX, bool GREEDY, bool SUMS>
bool launch_path_rows(const LeavesModel &cm, const PathTables &pt, const CodeRows &cr, int D, int F, int m, int n_trees, float *phi, double *part, int tile0,
                      hipStream_t s) {
    const PathSlotPlan plan = path_slot_plan(pt.n_used, cr.groups, D);
    if (!plan.fits) return false;   // rows too wide for an LDS tile beside one slot
    static StreamLdsOptIn optin;
    if (!optin.ok(k_path_rows<DMAX, GREEDY, SUMS>, plan.lds)) return false;
    const int vec_delta = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(pt.delta) & 15) == 0;
    hipLaunchKernelGGL((k_path_rows<DMAX, GREEDY, SUMS>), dim3(path_tiles(m)), dim3(kStreamRows), plan.lds, s, cm, pt, cr, D, F, m, n_trees, plan.slots, phi, part,
                       tile0, vec_delta);
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

bool path_rows_stream(const PredictModel &pm, const CodeTables &ct, const PathTables &pt, const CodeRows &cr, int F, int m, int n_trees, float *phi, double *part,
                      int tile0, hipStream_t s) {
    if (!leaves_streamable(pm, false) || pm.D > 64) return false;
    if (m <= 0 || pt.n_used <= 0) return path_slot_plan(pt.n_used, cr.groups, pm.D).fits;   // nothing to add: no launch
    const LeavesModel cm = code_walk(pm, ct);
    return with_stream_dmax(pm.D, [&](auto dmax) {
        constexpr int DMAX = decltype(dmax)::value;
        if (part != nullptr)
            return pm.oblivious ? launch_path_rows<DMAX, false, true>(cm, pt, cr, pm.D, F, m, n_trees, phi, part, tile0, s)
                                : launch_path_rows<DMAX, true, true>(cm, pt, cr, pm.D, F, m, n_trees, phi, part, tile0, s);
        return pm.oblivious ? launch_path_rows<DMAX, false, false>(cm, pt, cr, pm.D, F, m, n_trees, phi, part, tile0, s)
                            : launch_path_rows<DMAX, true, false>(cm, pt, cr, pm.D, F, m, n_trees, phi, part, tile0, s);
    });
}

void path_rows_general(const PredictModel &pm, const CodeTables &ct, const float *delta, const CodeRows &cr, int F, int m, int n_trees, float *phi, hipStream_t s) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_path_rows_general, dim3((m + 255) / 256), dim3(256), 0, s, code_walk(pm, ct), delta, cr, pm.D, F, m, n_trees, phi);
}

}  // namespace kern
}  // namespace gbrl
