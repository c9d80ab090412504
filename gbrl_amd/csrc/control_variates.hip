// control_variates.hip -- gfx950 kernels behind GBRL::control_variates / control_variates_prepared (cv_core.h has the rule and the order of every sum).
// A call that walks is four launches in one enqueue, nothing read back in between:
//
//   k_cv_walk          the momentum walk.  Lane = row, one wave per block, the block's 64 rows in LDS -- floats at stride F | 1, or a data set's
//                      code records at stride (8 G) | 1 (the body is a template over the row accessor; staging is predict_rowwalk.h's) -- and the
//                      row's D averages in registers, loaded from the held momentum (or zero) before the tile is staged.  The trees are taken in
//                      groups of kCvWalkTrees: first every tree of the group is walked to a leaf INDEX -- the condition words have wave-uniform
//                      addresses, so this phase is scalar loads and compares and holds one register per tree -- then the leaf rows are gathered
//                      cv_value_group(DMAX) trees at a time and applied in tree order.  The chain step is cv_chain: fl32(c * v) does not depend on
//                      m, so the dependent chain per tree is one multiply and one add; there is no rate and no owner table.  Epilogue: the raw m
//                      is stored, ms = fl32(m * scale) is stored to the scratch, the row's gradients are read (once) and the block's float64
//                      sums of g and ms go to its slot by the wave butterfly.
//   k_cv_walk_general  one thread per row, rows read in place, the reference's walk (greedy: leaf by leaf): D in 65..128, a tile beyond the LDS
//                      budget, a model that is not streamable, a refused LDS opt-in, and GBRL_HIP_CV_GENERIC=1.  A wave is 64 consecutive rows: it
//                      writes the slot the streaming block would.  The same bytes.
//   k_cv_fold          the walk's slots to 2 D totals, one wave per column (cv_fold's order)
//   k_cv_moments       one pass over ms and g: a wave per moment slot q takes the 64-row tiles q, q + S, ...; a lane forms the means of 16 columns from
//                      the totals, reads those 16 entries of its rows with 16-byte loads and keeps the float64 sums of mc * mc and gc * mc in
//                      registers; the butterfly writes the slot
//   k_cv_apply         blocks of 16 waves, at most one per CU; every block folds the moment slots to var, cov and alpha in LDS (the same order in every block; block 0 stores the
//                      statistics), then g' = fl32(g - fl32(fl32(ms - mbar) * alpha)) over its share of the matrix, 16 bytes at a time when D is a
//                      multiple of 4 and the addresses allow it
//
// This file is compiled without the packed float32 instructions and with contraction off (build.py SRC_FLAGS): every float32 operation is one scalar rounding.
#include "cv_core.h"
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------ the chain on a lane's registers
// the trees [t0, min(t0 + kCvWalkTrees, t_end)) (wave-uniform) on the averages m of the lane's row: all walked to leaf indices, then the leaf rows
// gathered KV at a time and applied in tree order
template <int DMAX, bool GREEDY, typename Row>
__device__ __forceinline__ void cv_chain_group(const LeavesModel &lm, const float *__restrict__ values, int D, const Row &x, int t0, int t_end, float beta,
                                               float c, int vec_values, float (&m)[DMAX]) {
    constexpr int KV = cv_value_group(DMAX);
    int leaf[kCvWalkTrees];
#pragma unroll
    for (int g = 0; g < kCvWalkTrees; ++g) leaf[g] = t0 + g < t_end ? stream_leaf<GREEDY>(lm, x, static_cast<const int32_t *>(nullptr), t0 + g) : 0;
#pragma unroll
    for (int g0 = 0; g0 < kCvWalkTrees; g0 += KV) {
        if (t0 + g0 >= t_end) break;   // (wave-uniform)
        float v[KV][DMAX];
#pragma unroll
        for (int k = 0; k < KV; ++k)
            if (t0 + g0 + k < t_end) stream_load_row<DMAX>(values + static_cast<size_t>(leaf[g0 + k]) * D, D, vec_values != 0, v[k]);
#pragma unroll
        for (int k = 0; k < KV; ++k)
            if (t0 + g0 + k < t_end) {
#pragma unroll
                for (int j = 0; j < DMAX; ++j) m[j] = cv_chain(m[j], beta, c, v[k][j]);
            }
    }
}

// the slot of 64 rows: sum g and sum ms per output, by the butterfly; lane 0 stores.  A lane without a row adds 0.0
template <int DMAX>
__device__ __forceinline__ void cv_store_slot(const float (&ms)[DMAX], const float (&g)[DMAX], bool live, int D, double *__restrict__ slot, int lane) {
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < D) {   // (wave-uniform)
            const double sg = wave_sum(live ? static_cast<double>(g[j]) : 0.0);
            const double sm = wave_sum(live ? static_cast<double>(ms[j]) : 0.0);
            if (lane == 0) { slot[j] = sg; slot[D + j] = sm; }
        }
}

struct CvIo {
    const float *grads;      // [n][D], read
    const float *m_in;       // [n][D] the held raw averages, or null: zero
    float *m_out, *ms_out;   // [n][D] each
    double *slots;           // [cv_walk_slots(n)][2 D]
    float beta, c, scale;
};

// ------------------------------------------------------------------------------------------------------------ streaming walk
struct CvFloatTile {   // the float rows of a batch: obs [n][F]
    const float *obs;
    int F;
    __device__ __forceinline__ void stage(void *tile, int r0, int rows, int lane, bool) const { stream_stage_tile(static_cast<float *>(tile), obs, F, r0, rows, lane); }
    __device__ __forceinline__ const float *row(const void *tile, int lane) const { return static_cast<const float *>(tile) + lane * (F | 1); }
};
struct CvCodeTile {    // rows of a prepared data set, through the row list when there is one
    CodeRows cr;
    __device__ __forceinline__ void stage(void *tile, int r0, int rows, int lane, bool live) const {
        const int at = cr.row0 + r0 + (live ? lane : 0);   // (a lane without a row names the block's first: a valid record, never used)
        const int my_row = cr.rows ? cr.rows[at] : at;
        stream_stage_code_tile(static_cast<uint32_t *>(tile), cr.codes, static_cast<size_t>(cr.n_rows), cr.groups, my_row, rows, lane);
    }
    __device__ __forceinline__ StreamCodeRow row(const void *tile, int lane) const {
        return StreamCodeRow{reinterpret_cast<const uint16_t *>(static_cast<const uint32_t *>(tile) + lane * stream_code_stride(cr.groups))};
    }
};

template <int DMAX, bool GREEDY, typename Tile>
__global__ __launch_bounds__(kStreamRows) void k_cv_walk(LeavesModel lm, const float *__restrict__ values, int D, Tile tl, int n, int start_tree, int stop_tree,
                                                         CvIo io, int vec_values, int vec_io) {
    extern __shared__ __align__(16) uint32_t cv_tile[];
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * kStreamRows;
    const int rows = min(kStreamRows, n - r0);
    const bool live = lane < rows;
    const size_t at = (static_cast<size_t>(r0) + lane) * D;
    float m[DMAX];
    if (live && io.m_in != nullptr) {
        stream_load_row<DMAX>(io.m_in + at, D, vec_io != 0, m);
    } else {
#pragma unroll
        for (int j = 0; j < DMAX; ++j) m[j] = 0.0f;
    }
    tl.stage(cv_tile, r0, rows, lane, live);
    __syncthreads();
    float g[DMAX];
    if (live) {
        stream_load_row<DMAX>(io.grads + at, D, vec_io != 0, g);   // (in flight behind the walk)
        const auto x = tl.row(cv_tile, lane);
        for (int t0 = start_tree; t0 < stop_tree; t0 += kCvWalkTrees) cv_chain_group<DMAX, GREEDY>(lm, values, D, x, t0, stop_tree, io.beta, io.c, vec_values, m);
        stream_store_row<DMAX>(io.m_out + at, D, vec_io != 0, m);
#pragma unroll
        for (int j = 0; j < DMAX; ++j) m[j] = cv_mul(m[j], io.scale);
        stream_store_row<DMAX>(io.ms_out + at, D, vec_io != 0, m);
    } else {
#pragma unroll
        for (int j = 0; j < DMAX; ++j) g[j] = 0.0f;
    }
    cv_store_slot<DMAX>(m, g, live, D, io.slots + static_cast<size_t>(blockIdx.x) * 2 * D, lane);
}

// ------------------------------------------------------------------------------------------------------------ general walk
struct CvFloatRows {
    const float *obs;
    int F;
    __device__ __forceinline__ GeneralRow row(int j) const { return GeneralRow{obs + static_cast<size_t>(j) * F, nullptr}; }
};
struct CvCodeRows {
    CodeRows cr;
    __device__ __forceinline__ GeneralCodeRow row(int j) const {
        const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + j] : cr.row0 + j);
        return GeneralCodeRow{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    }
};

template <int DMAX, typename Rows>
__global__ __launch_bounds__(256) void k_cv_walk_general(LeavesModel lm, const float *__restrict__ values, int D, Rows rw, int n, int start_tree, int stop_tree,
                                                         CvIo io) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;   // (whole waves stay: the butterfly)
    const bool live = j < n;
    const size_t at = static_cast<size_t>(live ? j : 0) * D;
    float m[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) m[d] = (live && io.m_in != nullptr && d < D) ? io.m_in[at + d] : 0.0f;
    if (live) {
        const auto r = rw.row(j);
        for (int t = start_tree; t < stop_tree; ++t) {
            const int leaf = general_leaf(lm, r, t);
            if (leaf < 0) break;   // a greedy search ran off the ensemble: the walk ends
            const float *v = values + static_cast<size_t>(leaf) * D;
#pragma unroll
            for (int d = 0; d < DMAX; ++d)
                if (d < D) m[d] = cv_chain(m[d], io.beta, io.c, v[d]);
        }
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
            if (d < D) {
                io.m_out[at + d] = m[d];
                m[d] = cv_mul(m[d], io.scale);
                io.ms_out[at + d] = m[d];
            }
    }
    const int slot = j / kCvSlotRows, lane = threadIdx.x & (kCvSlotRows - 1);
    if (slot >= cv_walk_slots(n)) return;   // (wave-uniform: a wave wholly behind the last row)
    double *sl = io.slots + static_cast<size_t>(slot) * 2 * D;
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
        if (d < D) {
            const double sg = wave_sum(live ? static_cast<double>(io.grads[at + d]) : 0.0);
            const double sm = wave_sum(live ? static_cast<double>(m[d]) : 0.0);
            if (lane == 0) { sl[d] = sg; sl[D + d] = sm; }
        }
}

// ------------------------------------------------------------------------------------------------------------ the sums
// cv_fold on a wave: column c of S slots of C doubles; every lane returns the same bits
__device__ __forceinline__ double cv_fold_wave(const double *__restrict__ part, int S, int C, int c, int lane) {
    double acc = 0.0;
    for (int s = lane; s < S; s += kCvSlotRows) acc += part[static_cast<size_t>(s) * C + c];
    return wave_sum(acc);
}

__global__ __launch_bounds__(kCvSlotRows) void k_cv_fold(const double *__restrict__ slots, int S, int C, double *__restrict__ totals) {
    const double t = cv_fold_wave(slots, S, C, blockIdx.x, threadIdx.x);
    if (threadIdx.x == 0) totals[blockIdx.x] = t;
}

// a wave per moment slot; the block's four waves take four consecutive slots.  A lane reads kCvMomentCols consecutive entries of its row of ms and g
// at a time (16-byte loads when vec4) into registers and keeps their float64 sums there: the matrices are read once, whole 64-byte runs per lane; wider
// rows take one such pass per run of columns.  The order of every sum is cv_core.h's: per (slot, lane, column) the rows in turn, then the butterfly.
constexpr int kCvMomentCols = 16;
__global__ __launch_bounds__(256) void k_cv_moments(const float *__restrict__ g, const float *__restrict__ ms, long long n, int D, const double *__restrict__ totals,
                                                    int S2, double *__restrict__ part, int vec4) {
    const int lane = threadIdx.x & (kCvSlotRows - 1);
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= S2) return;   // (wave-uniform)
    double *sl = part + static_cast<size_t>(q) * 2 * D;
    for (int j0 = 0; j0 < D; j0 += kCvMomentCols) {
        float gbar[kCvMomentCols], mbar[kCvMomentCols];
        double a[kCvMomentCols], b[kCvMomentCols];
#pragma unroll
        for (int k = 0; k < kCvMomentCols; ++k) {
            const bool in = j0 + k < D;   // (wave-uniform)
            gbar[k] = in ? cv_mean(totals[j0 + k], n) : 0.0f;
            mbar[k] = in ? cv_mean(totals[D + j0 + k], n) : 0.0f;
            a[k] = b[k] = 0.0;
        }
        for (long long r = static_cast<long long>(q) * kCvSlotRows + lane; r < n; r += static_cast<long long>(S2) * kCvSlotRows) {
            const float *gr = g + r * D + j0, *mr = ms + r * D + j0;
            float gv[kCvMomentCols], mv[kCvMomentCols];
            if (vec4) {
#pragma unroll
                for (int k4 = 0; k4 < kCvMomentCols / 4; ++k4) {
                    const bool in = j0 + 4 * k4 < D;
                    const float4 x = in ? reinterpret_cast<const float4 *>(gr)[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 y = in ? reinterpret_cast<const float4 *>(mr)[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
                    gv[4 * k4] = x.x; gv[4 * k4 + 1] = x.y; gv[4 * k4 + 2] = x.z; gv[4 * k4 + 3] = x.w;
                    mv[4 * k4] = y.x; mv[4 * k4 + 1] = y.y; mv[4 * k4 + 2] = y.z; mv[4 * k4 + 3] = y.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < kCvMomentCols; ++k) {
                    gv[k] = j0 + k < D ? gr[k] : 0.0f;
                    mv[k] = j0 + k < D ? mr[k] : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < kCvMomentCols; ++k)
                if (j0 + k < D) {
                    const double mc = static_cast<double>(cv_sub(mv[k], mbar[k])), gc = static_cast<double>(cv_sub(gv[k], gbar[k]));
                    a[k] += mc * mc;   // (exact products: contracted or not, one rounding per add)
                    b[k] += gc * mc;
                }
        }
#pragma unroll
        for (int k = 0; k < kCvMomentCols; ++k)
            if (j0 + k < D) {
                const double sa = wave_sum(a[k]), sb = wave_sum(b[k]);
                if (lane == 0) { sl[j0 + k] = sa; sl[D + j0 + k] = sb; }
            }
    }
}

// blocks of 16 waves, at most one per CU: the fold of the moment slots is spread over the block's waves (a wave per output in turn), so a block reads
// the slot array once from L2 -- S2 x 2 D doubles -- and the chip reads it once per CU, not once per 256 threads
constexpr int kCvApplyThreads = 1024;
__global__ __launch_bounds__(kCvApplyThreads) void k_cv_apply(const float *__restrict__ g, const float *__restrict__ ms, long long n, int D, const double *__restrict__ totals,
                                                  const double *__restrict__ part, int S2, float *__restrict__ out, float *__restrict__ stats, int vec4) {
    extern __shared__ float cv_sh[];   // [2 D]: alpha, mbar
    float *alpha = cv_sh, *mbar = cv_sh + D;
    const int lane = threadIdx.x & (kCvSlotRows - 1), wave = threadIdx.x >> 6;
    for (int j = wave; j < D; j += kCvApplyThreads / kCvSlotRows) {   // (a wave per output; every block in the same order)
        const float var = cv_moment(cv_fold_wave(part, S2, 2 * D, j, lane), n), cov = cv_moment(cv_fold_wave(part, S2, 2 * D, D + j, lane), n);
        if (lane == 0) {
            const float a = cv_alpha(cov, var), gb = cv_mean(totals[j], n), mb = cv_mean(totals[D + j], n);
            alpha[j] = a;
            mbar[j] = mb;
            if (blockIdx.x == 0) {
                stats[kCvAlpha * D + j] = a; stats[kCvMeanGrads * D + j] = gb; stats[kCvMeanMomentum * D + j] = mb;
                stats[kCvVar * D + j] = var; stats[kCvCov * D + j] = cov;
            }
        }
    }
    __syncthreads();
    const size_t n_el = static_cast<size_t>(n) * D, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    if (vec4) {   // D is a multiple of 4: the four entries lie in one row
        const float4 *g4 = reinterpret_cast<const float4 *>(g), *m4 = reinterpret_cast<const float4 *>(ms);
        float4 *o4 = reinterpret_cast<float4 *>(out);
        for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el / 4; i += stride) {
            const int j = static_cast<int>((i * 4) % D);
            const float4 gv = g4[i], mv = m4[i];
            float4 o;
            o.x = cv_corrected(gv.x, cv_sub(mv.x, mbar[j]), alpha[j]);
            o.y = cv_corrected(gv.y, cv_sub(mv.y, mbar[j + 1]), alpha[j + 1]);
            o.z = cv_corrected(gv.z, cv_sub(mv.z, mbar[j + 2]), alpha[j + 2]);
            o.w = cv_corrected(gv.w, cv_sub(mv.w, mbar[j + 3]), alpha[j + 3]);
            o4[i] = o;
        }
    } else {
        for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el; i += stride) {
            const int j = static_cast<int>(i % D);
            out[i] = cv_corrected(g[i], cv_sub(ms[i], mbar[j]), alpha[j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ launches
template <int DMAX, bool GREEDY, typename Tile>
bool launch_cv_walk(const LeavesModel &lm, const PredictModel &pm, const Tile &tl, size_t lds, int n, int start_tree, int stop_tree, const CvIo &io, hipStream_t s) {
    if (lds > kStreamLdsBudget) return false;   // rows too wide for an LDS tile
    static StreamLdsOptIn optin;
    if (!optin.ok(k_cv_walk<DMAX, GREEDY, Tile>, lds)) return false;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_io = d4 && ((reinterpret_cast<uintptr_t>(io.grads) | reinterpret_cast<uintptr_t>(io.m_in) | reinterpret_cast<uintptr_t>(io.m_out) |
                               reinterpret_cast<uintptr_t>(io.ms_out)) & 15) == 0;
    hipLaunchKernelGGL((k_cv_walk<DMAX, GREEDY, Tile>), dim3((n + kStreamRows - 1) / kStreamRows), dim3(kStreamRows), lds, s, lm, pm.values, pm.D, tl, n, start_tree,
                       stop_tree, io, vec_values, vec_io);
    return true;
}

template <typename Tile, typename Rows>
void cv_walk(const PredictModel &pm, const LeavesModel &lm, const Tile &tl, size_t lds, const Rows &rw, int n, int start_tree, int stop_tree, const CvIo &io,
             bool generic, hipStream_t s) {
    static_assert(kCvSlotRows == kStreamRows, "a block of the streaming walk writes exactly one slot");
    if (leaves_streamable(pm, generic) && pm.D <= kCvStreamMaxD && with_stream_dmax(pm.D, [&](auto dmax) {
            constexpr int DMAX = decltype(dmax)::value;
            return pm.oblivious ? launch_cv_walk<DMAX, false>(lm, pm, tl, lds, n, start_tree, stop_tree, io, s)
                                : launch_cv_walk<DMAX, true>(lm, pm, tl, lds, n, start_tree, stop_tree, io, s);
        }))
        return;
    with_general_dmax(pm.D, [&](auto dmax) {
        hipLaunchKernelGGL((k_cv_walk_general<decltype(dmax)::value, Rows>), dim3((n + 255) / 256), dim3(256), 0, s, lm, pm.values, pm.D, rw, n, start_tree, stop_tree, io);
    });
}

// fold, moments, apply: the three launches behind either walk
void cv_statistics(const CvBuffers &b, int n, int D, hipStream_t s) {
    const int S1 = cv_walk_slots(n), S2 = cv_moment_slots(n);
    hipLaunchKernelGGL(k_cv_fold, dim3(2 * D), dim3(kCvSlotRows), 0, s, b.slots, S1, 2 * D, b.totals);
    const int vec4 = (D & 3) == 0 && ((reinterpret_cast<uintptr_t>(b.grads) | reinterpret_cast<uintptr_t>(b.ms) | reinterpret_cast<uintptr_t>(b.grads_out)) & 15) == 0;
    hipLaunchKernelGGL(k_cv_moments, dim3((S2 + 3) / 4), dim3(256), 0, s, b.grads, b.ms, static_cast<long long>(n), D, b.totals, S2, b.moments, vec4);
    const size_t n_el = static_cast<size_t>(n) * D, per_block = static_cast<size_t>(kCvApplyThreads) * (vec4 ? 4 : 1);
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n_el + per_block - 1) / per_block, static_cast<size_t>(stream_cu_count())));
    hipLaunchKernelGGL(k_cv_apply, dim3(std::max(blocks, 1u)), dim3(kCvApplyThreads), sizeof(float) * 2 * D, s, b.grads, b.ms, static_cast<long long>(n), D, b.totals,
                       b.moments, S2, b.grads_out, b.stats, vec4);
}

CvIo cv_io(const CvBuffers &b, float beta, float scale) { return CvIo{b.grads, b.momentum_in, b.momentum_out, b.ms, b.slots, beta, cv_sub(1.0f, beta), scale}; }

}  // namespace

void control_variates(const PredictModel &pm, const float *obs, int F, int n, int start_tree, int stop_tree, float beta, float scale, const CvBuffers &b, bool generic,
                      hipStream_t s) {
    const LeavesModel lm = leaves_model(pm);
    cv_walk(pm, lm, CvFloatTile{obs, F}, stream_tile_bytes(F), CvFloatRows{obs, F}, n, start_tree, stop_tree, cv_io(b, beta, scale), generic, s);
    cv_statistics(b, n, pm.D, s);
}

void control_variates_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int start_tree, int stop_tree, float beta, float scale,
                            const CvBuffers &b, bool generic, hipStream_t s) {
    // the model view of the float walk with the threshold words replaced by bins (the packed conditions, the greedy node records, the general table)
    LeavesModel lm = leaves_model(pm);
    lm.cond_pack = ct.cond_pack;
    lm.grd_nodes = ct.grd_nodes;
    lm.feature_bins = ct.bins;
    cv_walk(pm, lm, CvCodeTile{cr}, stream_code_tile_bytes(cr.groups), CvCodeRows{cr}, m, start_tree, stop_tree, cv_io(b, beta, scale), generic, s);
    cv_statistics(b, m, pm.D, s);
}

}  // namespace kern
}  // namespace gbrl
