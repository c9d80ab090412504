// predict_staged.hip -- gfx950 kernels behind GBRL::predict_staged / GBRL::staged_loss: every prefix [0, stops[s]) of the ensemble evaluated in
// ONE walk.  Per (row, output) a prediction is one chain in tree order, p = fma(-rate(t, optimizer of the output), value(leaf(row, t)), p)
// started from the bias (predict_continue.hip); a staged evaluation is that chain with checkpoints.  Stage s has, bit for bit, what
// kern::predict_continue(base = tiled bias, 0, stops[s]) returns: rates at the absolute tree index, an output that no optimizer owns keeps the
// bias bits, and the walk is never split over tree ranges.  stops[s] == 0 is the bias alone (0 never means "all trees" here).
//
//   k_staged          k_continue's layout: lane = row, one wave per block, the block's 64 rows in LDS at stride F | 1, the outputs of a row in
//                     registers, trees in groups of kG whose leaf values are in flight together.  A group ends at the next checkpoint and never
//                     straddles it.  At a checkpoint, predict mode stores the lane's D outputs to stage s (16-byte stores where D and the
//                     addresses allow); loss mode forms the row's sum_j (double)g_j^2, g_j = fl32(p_j - y_j), reduces the wave's 64 values by
//                     a fixed butterfly and lane 0 writes part[s][block].  The targets of a row are loaded once and held in registers next to
//                     the chain (D <= 64: at most 64 more VGPRs of the 512 a one-wave block may use); re-reading them per checkpoint would
//                     cost 4 D bytes per row and stage, more than the observation tile from a few dozen stages on.  The rows are read once:
//                     predict mode moves n (4 F + 4 D stages) bytes, loss mode n (4 F + 4 D) + 16 stages n / 64 (the partials written, then read).
//                     The tile staging and the row load are k_continue's own (predict_stream_common.h).
//                     Every output owned by at most one optimizer, D <= 64, a row tile that fits in LDS.
//   k_staged_general  anything the file format can hold: one thread per row, the reference's walk (greedy: leaf by leaf, Q7, its state carried
//                     across the checkpoints so that stage s is the walk over [0, stops[s]) and not a restart), optimizers that share outputs,
//                     D <= 128, rows too wide for an LDS tile.  The targets are re-read per checkpoint.  A wave still covers 64 consecutive rows
//                     and reduces them with the same butterfly, so both kernels write the same part[][] and staged_loss has the same bytes
//                     through either.  Also the cross-check behind GBRL_HIP_STAGED_GENERIC=1.
//   k_staged_finish   one block per stage: part[s][0 .. nb) summed in a fixed order (a strided serial sum per thread, then a fixed LDS tree).
//                     No floating-point atomics anywhere: two identical calls return identical bytes.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_stream_common.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

struct StagedModel {
    const int32_t *tree_indices, *depths, *feature_indices, *cat_ids, *cond_pack, *grd_nodes, *grd_node_off, *opt_start, *opt_stop;
    const float *feature_values, *values, *rate, *bias;
    const uint8_t *is_numerics, *inequality_directions;
    int n_leaves, max_depth, D, oblivious, n_opts, rate_stride;   // rate_stride: n_opts (rate table) or 0 (one rate per optimizer)
};

// what a checkpoint emits: predict mode (out != nullptr) or loss mode (targets, part)
struct StagedIo {
    const int32_t *stops;   // [n_stops] strictly ascending tree counts
    int n_stops;
    int walk;               // 0: no optimizer owns an output -- every stage is the bias, no tree is visited
    float *out;             // [n_stops][n][D]
    const float *targets;   // [n][D]
    double *part;           // [n_stops][nb], nb = ceil(n / 64)
    int nb;
};

constexpr int kStagedRows = kStreamRows;   // rows per wave = rows per loss partial, in both kernels

// sum of the wave's 64 values in a fixed order (xor butterfly: every lane ends with the same bits); called by whole waves only
__device__ __forceinline__ double staged_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum_j (double)g_j^2 of one row, j ascending; g_j = fl32(p_j - y_j) (loss.cpp:42-56).  (double)g * (double)g is exact.
template <int DMAX>
__device__ __forceinline__ double staged_row_loss(const float (&p)[DMAX], const float *y, int D) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < D) {
            const double g = static_cast<double>(__fsub_rn(p[j], y[j]));
            acc = fma(g, g, acc);
        }
    return acc;
}

// ------------------------------------------------------------------------------------------------------------ general kernel
template <int DMAX, bool LOSS>
__global__ __launch_bounds__(256) void k_staged_general(StagedModel cm, StagedIo io, const float *__restrict__ obs, int F,
                                                        const int32_t *__restrict__ cat_codes, int Fc, int n) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = row < static_cast<size_t>(n);
    const int D = cm.D, md = cm.max_depth;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? cm.bias[j] : 0.0f;
    const float *x = obs + (live ? row : 0) * F;
    const int32_t *xc = cat_codes ? cat_codes + (live ? row : 0) * Fc : nullptr;
    auto test = [&](int c) -> bool {
        const int f = cm.feature_indices[c];
        return cm.is_numerics[c] ? (x[f] > cm.feature_values[c]) : (xc != nullptr && xc[f] == cm.cat_ids[c]);
    };
    auto apply = [&](int t, const float *v) {
        for (int o = 0; o < cm.n_opts; ++o) {
            const float lr = cm.rate[static_cast<size_t>(t) * cm.rate_stride + o];
            const int a = cm.opt_start[o], b = cm.opt_stop[o];
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
                if (j >= a && j < b && j < D) p[j] = __fmaf_rn(-lr, v[j], p[j]);
        }
    };
    int t = 0, leaf = 0;
    bool at_root = true;   // greedy: the walk is about to enter tree t
    for (int s = 0; s < io.n_stops; ++s) {   // (uniform over the block)
        const int stop = io.walk ? io.stops[s] : 0;
        if (live) {
            if (cm.oblivious) {
                for (; t < stop; ++t) {
                    const int depth = cm.depths[t], cond = t * md;
                    int l = 0;
                    for (int d = 0; d < depth; ++d) l |= (test(cond + d) ? 1 : 0) << (depth - 1 - d);
                    apply(t, cm.values + static_cast<size_t>(cm.tree_indices[t] + l) * D);
                }
            } else {
                // k_continue_general's walk over [0, stop), suspended at the checkpoint: a leaf that never passes lets the walk run on into the
                // leaves of the following trees (Q7), so the state (t, leaf) is carried, not rebuilt per stage
                while (t < stop) {
                    if (at_root) { leaf = cm.tree_indices[t]; at_root = false; }
                    if (leaf >= cm.n_leaves) break;
                    const int depth = cm.depths[leaf], cond = leaf * md;
                    bool passed = false;
                    for (int d = depth - 1; d >= 0; --d) {
                        passed = (test(cond + d) == (cm.inequality_directions[cond + d] != 0));
                        if (!passed) break;
                    }
                    if (passed) {
                        apply(t, cm.values + static_cast<size_t>(leaf) * D);
                        ++t;
                        at_root = true;
                    } else {
                        ++leaf;
                    }
                }
            }
        }
        if constexpr (!LOSS) {
            if (live) {
                float *o = io.out + (static_cast<size_t>(s) * n + row) * D;
#pragma unroll
                for (int j = 0; j < DMAX; ++j)
                    if (j < D) o[j] = p[j];
            }
        } else {
            double acc = 0.0;
            if (live) acc = staged_row_loss<DMAX>(p, io.targets + row * D, D);   // (the targets are re-read per checkpoint)
            acc = staged_wave_sum(acc);
            const size_t wave = row / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
            if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < static_cast<size_t>(io.nb)) io.part[static_cast<size_t>(s) * io.nb + wave] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming kernel
template <int DMAX>
struct StagedOwner { uint8_t opt[DMAX]; };   // optimizer that owns output j (meaningful where bit j of `cover` is set)

template <int DMAX, bool GREEDY, bool LOSS>
__global__ __launch_bounds__(kStagedRows) void k_staged(StagedModel cm, StagedIo io, StagedOwner<DMAX> own, uint64_t cover, const float *__restrict__ obs,
                                                        int F, const int32_t *__restrict__ cat_codes, int Fc, int n, int vec_values, int vec_io) {
    extern __shared__ float stile[];   // [kStagedRows][F | 1]
    constexpr int kG = DMAX <= 4 ? 8 : DMAX <= 8 ? 4 : DMAX <= 16 ? 2 : 1;   // trees whose leaf values are in flight together
    const int lane = threadIdx.x;
    const int xs = F | 1;
    const int D = cm.D, md = cm.max_depth;
    const int r0 = blockIdx.x * kStagedRows;
    const int rows = min(kStagedRows, n - r0);
    const bool live = lane < rows;
    const size_t row = static_cast<size_t>(r0) + lane;
    float p[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) p[j] = j < D ? cm.bias[j] : 0.0f;   // (wave-uniform addresses: the scalar cache)
    float y[DMAX];   // loss mode: the row's targets, in flight together with the tile
    if constexpr (LOSS) {
        if (live) {
            stream_load_row<DMAX>(io.targets + row * D, D, vec_io != 0, y);
        } else {
#pragma unroll
            for (int j = 0; j < DMAX; ++j) y[j] = 0.0f;
        }
    }
    stream_stage_tile(stile, obs, F, r0, rows, lane);
    __syncthreads();
    const float *x = stile + (live ? lane : 0) * xs;
    const int32_t *xc = cat_codes ? cat_codes + (live ? row : 0) * Fc : nullptr;
    // feature word >= 0: numeric feature against a threshold; < 0: ~categorical feature against a dictionary id
    auto pass = [&](int fi, int tv) -> bool { return fi >= 0 ? (x[fi] > __int_as_float(tv)) : (xc != nullptr && xc[~fi] == tv); };
    int start_tree = 0;
    for (int s = 0; s < io.n_stops; ++s) {   // (wave-uniform)
        const int stop_tree = io.walk ? io.stops[s] : 0;
        if (live) {
            for (int t0 = start_tree; t0 < stop_tree; t0 += kG) {   // a group ends at the checkpoint
                int leaf[kG];
#pragma unroll
                for (int g = 0; g < kG; ++g) {
                    const int t = t0 + g;
                    leaf[g] = 0;
                    if (t < stop_tree) {   // (wave-uniform)
                        if (!GREEDY) {
                            const int depth = cm.depths[t];
                            const int32_t *cp = cm.cond_pack + static_cast<size_t>(t) * 2 * md;
                            int l = 0;
                            for (int d = 0; d < depth; ++d) l |= pass(cp[2 * d], cp[2 * d + 1]) ? (1 << (depth - 1 - d)) : 0;
                            leaf[g] = cm.tree_indices[t] + l;
                        } else {
                            // descent of the rebuilt binary tree: a child >= 0 is a node of the tree, < 0 is ~(leaf within the tree); a leaf lies
                            // at most max_depth steps below the root
                            const int4 *nodes = reinterpret_cast<const int4 *>(cm.grd_nodes) + cm.grd_node_off[t];
                            int node = 0;
                            for (int d = 0; d < md && node >= 0; ++d) {
                                const int4 nd = nodes[node];
                                node = pass(nd.x, nd.y) ? nd.w : nd.z;
                            }
                            leaf[g] = cm.tree_indices[t] + (node < 0 ? ~node : 0);
                        }
                    }
                }
                float v[kG][DMAX];
#pragma unroll
                for (int g = 0; g < kG; ++g)
                    if (t0 + g < stop_tree) stream_load_row<DMAX>(cm.values + static_cast<size_t>(leaf[g]) * D, D, vec_values != 0, v[g]);
#pragma unroll
                for (int g = 0; g < kG; ++g) {
                    const int t = t0 + g;
                    if (t < stop_tree) {
                        const float *rt = cm.rate + static_cast<size_t>(t) * cm.rate_stride;
#pragma unroll
                        for (int j = 0; j < DMAX; ++j)
                            if (j < D && ((cover >> j) & 1ull)) p[j] = __fmaf_rn(-rt[own.opt[j]], v[g][j], p[j]);
                    }
                }
            }
        }
        start_tree = max(start_tree, stop_tree);
        if constexpr (!LOSS) {
            if (live) {
                float *o = io.out + (static_cast<size_t>(s) * n + row) * D;
                if (vec_io) {
                    float4 *o4 = reinterpret_cast<float4 *>(o);
#pragma unroll
                    for (int q = 0; q < DMAX / 4; ++q)
                        if (4 * q < D) o4[q] = make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
                } else {
#pragma unroll
                    for (int j = 0; j < DMAX; ++j)
                        if (j < D) o[j] = p[j];
                }
            }
        } else {
            double acc = 0.0;
            if (live) acc = staged_row_loss<DMAX>(p, y, D);
            acc = staged_wave_sum(acc);
            if (lane == 0) io.part[static_cast<size_t>(s) * io.nb + blockIdx.x] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ finishing kernel
constexpr int kFinishThreads = 256;
__global__ __launch_bounds__(kFinishThreads) void k_staged_finish(const double *__restrict__ part, int nb, double *__restrict__ sums) {
    __shared__ double sh[kFinishThreads];
    const double *ps = part + static_cast<size_t>(blockIdx.x) * nb;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += kFinishThreads) acc += ps[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kFinishThreads / 2; w >= 1; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

// the loss checkpoint of k_staged_general on predictions that already exist (kern::staged_loss_of_predictions): the same row sum, the same
// butterfly over the same 64 rows, the same part[] entry
__global__ __launch_bounds__(256) void k_loss_of_predictions(const float *__restrict__ preds, const float *__restrict__ targets, int n, int D,
                                                             double *__restrict__ part, int nb) {
    const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    double acc = 0.0;
    if (row < static_cast<size_t>(n)) {
        const float *p = preds + row * D, *y = targets + row * D;
        for (int j = 0; j < D; ++j) {
            const double g = static_cast<double>(__fsub_rn(p[j], y[j]));
            acc = fma(g, g, acc);
        }
    }
    acc = staged_wave_sum(acc);
    const size_t wave = row / kStagedRows;
    if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < static_cast<size_t>(nb)) part[wave] = acc;
}

template <int DMAX, bool GREEDY, bool LOSS>
bool launch_staged(const StagedModel &cm, const StagedIo &io, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n,
                   hipStream_t s) {
    const size_t lds = static_cast<size_t>(kStagedRows) * (F | 1) * sizeof(float);
    if (lds > 156 * 1024) return false;   // rows too wide for an LDS tile
    static PerDeviceOnce attr;
    static uint64_t unsupported = 0;   // devices that refused the LDS opt-in: tiles above the default 64 KiB take the general kernel there
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0;
    if (attr.first() && hipFuncSetAttribute(reinterpret_cast<const void *>(k_staged<DMAX, GREEDY, LOSS>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024) != hipSuccess) {
        (void)hipGetLastError();
        unsupported |= bit;
    }
    if ((unsupported & bit) && lds > 64 * 1024) return false;
    StagedOwner<DMAX> own;
    for (int j = 0; j < DMAX; ++j) own.opt[j] = j < pm.D ? pm.owner[j] : 0;
    const bool d4 = (pm.D & 3) == 0;
    const int vec_values = d4 && (reinterpret_cast<uintptr_t>(pm.values) & 15) == 0;
    const int vec_io = d4 && (reinterpret_cast<uintptr_t>(LOSS ? static_cast<const void *>(io.targets) : static_cast<const void *>(io.out)) & 15) == 0;
    hipLaunchKernelGGL((k_staged<DMAX, GREEDY, LOSS>), dim3((n + kStagedRows - 1) / kStagedRows), dim3(kStagedRows), lds, s, cm, io, own, pm.coef_cover,
                       obs, F, cat_codes, Fc, n, vec_values, vec_io);
    return true;
}

template <bool GREEDY, bool LOSS>
bool launch_staged_d(const StagedModel &cm, const StagedIo &io, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n,
                     hipStream_t s) {
    if (pm.D <= 4) return launch_staged<4, GREEDY, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s);
    if (pm.D <= 8) return launch_staged<8, GREEDY, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s);
    if (pm.D <= 16) return launch_staged<16, GREEDY, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s);
    if (pm.D <= 32) return launch_staged<32, GREEDY, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s);
    return launch_staged<64, GREEDY, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s);
}

template <bool LOSS>
void staged_dispatch(const StagedModel &cm, const StagedIo &io, const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n,
                     bool generic, hipStream_t s) {
    // the streaming family: every output owned by at most one optimizer (owner[] is valid), the packed conditions / rebuilt node records
    const bool fast = !generic && pm.coef_ok && pm.D <= 64 && pm.max_depth >= 1 &&
                      (pm.oblivious ? pm.cond_pack != nullptr : (pm.grd_ok && pm.grd_nodes != nullptr && pm.grd_node_off != nullptr));
    if (fast) {
        if (pm.oblivious ? launch_staged_d<false, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s) : launch_staged_d<true, LOSS>(cm, io, pm, obs, F, cat_codes, Fc, n, s))
            return;
    }
    dim3 grid((n + 255) / 256), block(256);
    if (pm.D <= 8)
        hipLaunchKernelGGL((k_staged_general<8, LOSS>), grid, block, 0, s, cm, io, obs, F, cat_codes, Fc, n);
    else if (pm.D <= 32)
        hipLaunchKernelGGL((k_staged_general<32, LOSS>), grid, block, 0, s, cm, io, obs, F, cat_codes, Fc, n);
    else
        hipLaunchKernelGGL((k_staged_general<128, LOSS>), grid, block, 0, s, cm, io, obs, F, cat_codes, Fc, n);
}

}  // namespace

int staged_loss_partials(int n) { return (n + kStagedRows - 1) / kStagedRows; }

void staged_loss_of_predictions(const float *preds, const float *targets, int n, int D, double *part, double *sum, hipStream_t s) {
    const int nb = staged_loss_partials(n);
    hipLaunchKernelGGL(k_loss_of_predictions, dim3((n + 255) / 256), dim3(256), 0, s, preds, targets, n, D, part, nb);
    hipLaunchKernelGGL(k_staged_finish, dim3(1), dim3(kFinishThreads), 0, s, part, nb, sum);
}

void predict_staged(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, const StagedStops &st, float *out,
                    const float *targets, double *part, double *sums, bool generic, hipStream_t s) {
    StagedModel cm{};
    cm.tree_indices = pm.tree_indices; cm.depths = pm.depths; cm.feature_indices = pm.feature_indices; cm.cat_ids = pm.cat_ids;
    cm.cond_pack = pm.cond_pack; cm.grd_nodes = pm.grd_nodes; cm.grd_node_off = pm.grd_node_off;
    cm.opt_start = pm.opt_start; cm.opt_stop = pm.opt_stop;
    cm.feature_values = pm.feature_values; cm.values = pm.values; cm.bias = pm.bias;
    cm.rate = pm.rate != nullptr ? pm.rate : pm.opt_lr;
    cm.rate_stride = pm.rate != nullptr ? pm.n_opts : 0;
    cm.is_numerics = pm.is_numerics; cm.inequality_directions = pm.inequality_directions;
    cm.n_leaves = pm.n_leaves; cm.max_depth = pm.max_depth; cm.D = pm.D; cm.oblivious = pm.oblivious; cm.n_opts = pm.n_opts;
    StagedIo io{};
    io.stops = st.stops; io.n_stops = st.n_stops;
    io.walk = (pm.n_opts > 0 && pm.n_trees > 0 && st.last_stop > 0) ? 1 : 0;   // as kern::predict_continue: no optimizer, no tree to apply
    io.out = out; io.targets = targets; io.part = part; io.nb = staged_loss_partials(n);
    if (targets == nullptr) {
        staged_dispatch<false>(cm, io, pm, obs, F, cat_codes, Fc, n, generic, s);
    } else {
        staged_dispatch<true>(cm, io, pm, obs, F, cat_codes, Fc, n, generic, s);
        hipLaunchKernelGGL(k_staged_finish, dim3(st.n_stops), dim3(kFinishThreads), 0, s, part, io.nb, sums);
    }
}

}  // namespace kern
}  // namespace gbrl
