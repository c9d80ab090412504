// leaf_accum.h -- per-leaf integer sums, once: what refit.hip, newton.hip, predict_leaves.hip (k_leaf_counts*) and leaf_quantile.hip (k_lq_route) do
// with a row after the walk of predict_rowwalk.h has routed it to a leaf of one tree.  Every sum is an integer: exact and order-free, so every run
// and both kernel families produce the same bytes.  Two schemes:
//   streaming    one wave per block, lane = row, the tree's accumulators in LDS behind the row tile (LeafAccLds: [n_leaves][W] int64, value v of
//                output j at [v * D + j], the row count at [NV * D]), tiles in a grid-stride loop, one global atomic per non-zero word at the
//                block's end: global atomics are blocks x leaves x W, not rows.  The LDS is private to the wave.  A tree of at most
//                kLeafAccWaveLeaves leaves puts 16 or more lanes on every address; there the wave reduces each leaf's contributions with a
//                butterfly and lane 0 adds the result with a plain LDS add.  Deeper trees use one 64-bit LDS atomic per lane and value.
//                The uint32 row counters of k_leaf_counts and k_lq_route share only the zero and flush loops (leaf_acc_zero, leaf_acc_flush).
//   general      one thread per row, accumulators in global memory, one add per distinct leaf and wave (for_each_wave_leaf + wave_sum).
// A new user supplies the walk (a leaf per lane), its values already quantised to int64, and the tile bytes and block cap of its launch.
#pragma once

#include <algorithm>
#include <cstddef>
#ifdef __HIPCC__
#include "kernels_common.h"
#endif

namespace gbrl {
namespace kern {

// ------------------------------------------------------------------------------------------------------------ host side (compiles without HIP)
constexpr size_t kStreamLdsBudget = 156 * 1024;   // the dynamic LDS the streaming kernels opt in to (StreamLdsOptIn, predict_rowwalk.h)

struct TreeSpan { int t, leaf0, n_leaves; };   // the tree, its first global leaf, its leaves

// Launch geometry of a streaming kernel that keeps acc_bytes of accumulators behind a tile: whether both fit the budget, the dynamic LDS, and as
// many blocks as the chip holds at once (160 KiB of LDS per CU, at most per_cu_cap one-wave blocks counted per CU): each then flushes once.
struct LeafAccPlan { bool fits; size_t lds; int blocks; };
inline LeafAccPlan leaf_acc_plan(size_t tile_bytes, size_t acc_bytes, int n_tiles, int per_cu_cap, int cus) {
    const size_t lds = tile_bytes + acc_bytes;
    const int per_cu = static_cast<int>(std::min<size_t>(per_cu_cap, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(lds, 1))));
    return {lds <= kStreamLdsBudget, lds, std::min(n_tiles, cus * per_cu)};
}

#ifdef __HIPCC__
namespace {
// ------------------------------------------------------------------------------------------------------------ device side
constexpr int kLeafAccWaveLeaves = 4;   // up to this many leaves: reduce within the wave (>= 16 lanes per address otherwise)

// sum over the wave (every lane ends with it), offsets 32, 16, ..., 1; integers: exact, order-free (a double: the loss partials' fixed order)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// the in-tree index of a global leaf; -1 when the search left the tree: the row joins no sum
__device__ __forceinline__ int local_leaf(int leaf, int leaf0, int n_leaves) {
    const int l = leaf - leaf0;
    return l < 0 || l >= n_leaves ? -1 : l;
}

// fn(k, mine, same, leader) once per distinct l >= 0 of the wave, wave-uniformly (every lane of the wave must call this): mine = this lane holds
// k, same = the ballot of the lanes that do, leader = the lowest of them -- the lane that adds what the wave summed
template <typename Fn>
__device__ __forceinline__ void for_each_wave_leaf(int l, int lane, Fn fn) {
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {   // (wave-uniform)
        const int first = __ffsll(static_cast<long long>(todo)) - 1;
        const int k = __shfl(l, first, kWave);
        const bool mine = l == k;
        const unsigned long long same = __ballot(mine);
        fn(k, mine, same, lane == first);
        todo &= ~same;
    }
}

// n words of LDS counters zeroed / added to their global counterparts, one atomic per non-zero word, by the block's nthreads threads
template <typename T>
__device__ __forceinline__ void leaf_acc_zero(T *lds, int n, int tid, int nthreads) {
    for (int i = tid; i < n; i += nthreads) lds[i] = 0;
}
template <typename T>
__device__ __forceinline__ void leaf_acc_flush(const T *lds, T *global, int n, int tid, int nthreads) {
    for (int i = tid; i < n; i += nthreads) {
        const T v = lds[i];
        if (v) atomicAdd(&global[i], v);
    }
}

// the streaming scheme's accumulators of one tree, NV values per output; the block is one wave
template <int NV>
struct LeafAccLds {
    unsigned long long *a;   // [n_leaves][W] in LDS
    int n_leaves, W;         // W = NV * D + 1

    // (no barrier: the first tile's barrier stands between this and the first add)
    __device__ __forceinline__ void zero(int lane) const { leaf_acc_zero(a, n_leaves * W, lane, kWave); }

    // the row of lane `lane` joins leaf l (-1: none); q(v, j) is the quantised value v of output j.  Every lane of the wave calls this.
    template <int DMAX, typename Q>
    __device__ __forceinline__ void add(int l, int lane, int D, Q q) const {
        if (n_leaves <= kLeafAccWaveLeaves) {   // (uniform)
            for (int k = 0; k < n_leaves; ++k) {
                const bool mine = l == k;
                const unsigned long long same = __ballot(mine);
                if (same == 0ull) continue;   // (wave-uniform)
                unsigned long long *row = a + k * W;
#pragma unroll
                for (int j = 0; j < DMAX; ++j)
#pragma unroll
                    for (int v = 0; v < NV; ++v)
                        if (j < D) {
                            const long long s = wave_sum(mine ? q(v, j) : 0ll);
                            if (lane == 0) row[v * D + j] += static_cast<unsigned long long>(s);
                        }
                if (lane == 0) row[NV * D] += static_cast<unsigned long long>(__popcll(same));
            }
        } else if (l >= 0) {
            unsigned long long *row = a + l * W;
#pragma unroll
            for (int j = 0; j < DMAX; ++j)
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    if (j < D) atomicAdd(&row[v * D + j], static_cast<unsigned long long>(q(v, j)));
            atomicAdd(&row[NV * D], 1ull);
        }
    }

    // after the last tile: the wave's adds are done, then one global atomic per non-zero word
    __device__ __forceinline__ void flush(unsigned long long *global, int lane) const {
        __syncthreads();
        leaf_acc_flush(a, global, n_leaves * W, lane, kWave);
    }
};

}  // namespace
#endif

}  // namespace kern
}  // namespace gbrl
