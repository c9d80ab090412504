// metric.hip -- gfx950 kernels of the classifier metrics (metric_core.h has the definitions): integer counts only, added with integer atomics,
// so a result does not depend on scheduling; every floating-point step happens on the host from these integers.
//
//   k_metric_error     lane = row.  The wrong flags of a wave become a count through __ballot + popcount, the waves of a block meet in LDS, and a
//                      block adds one integer per counter to the unsigned long long counters [D] (softmax: one).
//   k_auc_keys         lane = row: key[d][i] = metric_key(P[i][d]), val[d][i] = (Y[i][d] > 0.5) -- the transposed, column-major [D][n] arrays the
//                      segmented sort works on -- and the positives per column counted like the errors.  Without P it only counts (fit_prepared's
//                      refusal of a validation column with one class).
//   radix_sort_pass    x 4 (radix_sort.hip): every column sorted by key, ascending, the flag riding along; the columns are the segments.
//   k_auc_neg_tiles /  an exclusive prefix count of the negatives along each sorted column, n + 1 entries per column: the negatives per tile of
//   k_auc_neg_scan /   2048 positions, one block per column that turns the tile counts into exclusive offsets, and the positions of a tile
//   k_auc_neg_prefix   from its offset and ballots -- the way sample_rows.hip places its block counts.  No block waits for another.
//   k_auc_pairs        every positive finds the first position lo and the one-past-last position hi of its key in its sorted column by two binary
//                      searches (lo <= i < hi: each search covers one side of i) and adds negprefix[lo] + negprefix[hi] = #{negatives below} +
//                      #{negatives below or equal}.  A block sums in uint64 and adds once to U2[d].
// Reads stay below n * D of the inputs; the sorted arrays and the prefix are indexed with d * n + i, i < n, and d * (n + 1) + i, i <= n.
#include "kernels.h"
#include "kernels_common.h"
#include "metric_core.h"
#include "objective_core.h"

#include <utility>

namespace gbrl {
namespace kern {

namespace {

constexpr int kMetricThreads = 256, kMetricWaves = kMetricThreads / kWave;
constexpr int kMetricMaxD = 128;
constexpr int kTileRounds = kRadixSortTile / kMetricThreads;
static_assert(kRadixSortTile % kMetricThreads == 0, "a tile is whole rounds of the block");

// flags of a block's rows for counter d -> one LDS add per wave
__device__ __forceinline__ void count_flags(bool flag, uint32_t *cnt_d) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0 && b != 0ull) atomicAdd(cnt_d, static_cast<uint32_t>(__popcll(b)));
}

template <bool kSoftmax>
__global__ __launch_bounds__(kMetricThreads) void k_metric_error(const float *__restrict__ P, const void *__restrict__ T, int n, int D,
                                                                 unsigned long long *__restrict__ wrong) {
    __shared__ uint32_t cnt[kMetricMaxD];
    for (int d = threadIdx.x; d < kMetricMaxD; d += kMetricThreads) cnt[d] = 0;
    __syncthreads();
    const int r = blockIdx.x * kMetricThreads + threadIdx.x;
    const bool live = r < n;
    const float *p = P + static_cast<size_t>(live ? r : 0) * D;
    if (kSoftmax) {
        const int32_t label = live ? static_cast<const int32_t *>(T)[r] : 0;
        count_flags(live && metric_argmax(p, D) != label, &cnt[0]);
    } else {
        const float *y = static_cast<const float *>(T) + static_cast<size_t>(live ? r : 0) * D;
        for (int d = 0; d < D; ++d) count_flags(live && metric_logistic_wrong(p[d], y[d]), &cnt[d]);
    }
    __syncthreads();
    const int C = kSoftmax ? 1 : D;
    for (int d = threadIdx.x; d < C; d += kMetricThreads)
        if (cnt[d] != 0) atomicAdd(&wrong[d], static_cast<unsigned long long>(cnt[d]));
}

__global__ __launch_bounds__(kMetricThreads) void k_auc_keys(const float *__restrict__ P /*nullable*/, const float *__restrict__ Y, uint32_t n, int D,
                                                             uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                             unsigned long long *__restrict__ pos /*nullable*/) {
    __shared__ uint32_t cnt[kMetricMaxD];
    for (int d = threadIdx.x; d < kMetricMaxD; d += kMetricThreads) cnt[d] = 0;
    __syncthreads();
    const uint32_t r = blockIdx.x * static_cast<uint32_t>(kMetricThreads) + threadIdx.x;
    const bool live = r < n;
    const size_t row = static_cast<size_t>(live ? r : 0) * D;
    for (int d = 0; d < D; ++d) {
        const bool positive = live && metric_positive(Y[row + d]);
        if (P != nullptr && live) {
            const size_t at = static_cast<size_t>(d) * n + r;
            key[at] = metric_key(P[row + d]);
            val[at] = positive ? 1u : 0u;
        }
        if (pos != nullptr) count_flags(positive, &cnt[d]);
    }
    if (pos == nullptr) return;
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += kMetricThreads)
        if (cnt[d] != 0) atomicAdd(&pos[d], static_cast<unsigned long long>(cnt[d]));
}

// block (tile, column): the negatives among the tile's sorted positions
__global__ __launch_bounds__(kMetricThreads) void k_auc_neg_tiles(const uint32_t *__restrict__ val, uint32_t n, uint32_t n_tiles, uint32_t *__restrict__ tile_neg) {
    __shared__ uint32_t tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    val += static_cast<size_t>(blockIdx.y) * n;
    const uint32_t t0 = blockIdx.x * static_cast<uint32_t>(kRadixSortTile);
    uint32_t c = 0;
    for (int k = 0; k < kTileRounds; ++k) {
        const uint32_t i = t0 + k * kMetricThreads + threadIdx.x;
        c += static_cast<uint32_t>(__popcll(__ballot(i < n && val[i] == 0u)));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_neg[static_cast<size_t>(blockIdx.y) * n_tiles + blockIdx.x] = tot;
}

// one block per column: the tile counts become exclusive offsets, in slices of the block's width with a carry
__global__ __launch_bounds__(kMetricThreads) void k_auc_neg_scan(uint32_t *__restrict__ tile_neg, uint32_t n_tiles) {
    __shared__ uint32_t sc[kMetricThreads];
    tile_neg += static_cast<size_t>(blockIdx.x) * n_tiles;
    const int tid = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += kMetricThreads) {
        const uint32_t b = b0 + tid;
        const uint32_t c = b < n_tiles ? tile_neg[b] : 0u;
        sc[tid] = c;
        __syncthreads();
        for (int o = 1; o < kMetricThreads; o <<= 1) {
            const uint32_t add = tid >= o ? sc[tid - o] : 0u;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        if (b < n_tiles) tile_neg[b] = carry + sc[tid] - c;
        carry += sc[kMetricThreads - 1];
        __syncthreads();   // sc is rewritten by the next slice
    }
}

// block (tile, column): negprefix[d][i] = negatives among the sorted positions below i, for the tile's i; the last position also writes entry n
__global__ __launch_bounds__(kMetricThreads) void k_auc_neg_prefix(const uint32_t *__restrict__ val, uint32_t n, uint32_t n_tiles,
                                                                   const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ negprefix) {
    __shared__ uint32_t s_wave[kMetricWaves];
    val += static_cast<size_t>(blockIdx.y) * n;
    negprefix += static_cast<size_t>(blockIdx.y) * (static_cast<size_t>(n) + 1);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t t0 = blockIdx.x * static_cast<uint32_t>(kRadixSortTile);
    uint32_t run = tile_off[static_cast<size_t>(blockIdx.y) * n_tiles + blockIdx.x];   // negatives before this round (the same in every thread)
    for (int k = 0; k < kTileRounds; ++k) {
        const uint32_t i = t0 + k * kMetricThreads + threadIdx.x;
        const bool neg = i < n && val[i] == 0u;
        const unsigned long long b = __ballot(neg);
        if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__popcll(b));
        __syncthreads();
        uint32_t before = 0, round = 0;
#pragma unroll
        for (int w = 0; w < kMetricWaves; ++w) {
            const uint32_t t = s_wave[w];
            before += w < wave ? t : 0u;
            round += t;
        }
        const uint32_t excl = run + before + static_cast<uint32_t>(__popcll(b & ((1ull << lane) - 1ull)));
        if (i < n) {
            negprefix[i] = excl;
            if (i == n - 1) negprefix[n] = excl + (neg ? 1u : 0u);
        }
        run += round;
        __syncthreads();   // s_wave is rewritten by the next round
    }
}

__global__ __launch_bounds__(kMetricThreads) void k_auc_pairs(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t n,
                                                              const uint32_t *__restrict__ negprefix, unsigned long long *__restrict__ u2) {
    __shared__ unsigned long long part[kMetricThreads];
    key += static_cast<size_t>(blockIdx.y) * n;
    val += static_cast<size_t>(blockIdx.y) * n;
    negprefix += static_cast<size_t>(blockIdx.y) * (static_cast<size_t>(n) + 1);
    const uint32_t t0 = blockIdx.x * static_cast<uint32_t>(kRadixSortTile);
    unsigned long long sum = 0;
    for (int k = 0; k < kTileRounds; ++k) {
        const uint32_t i = t0 + k * kMetricThreads + threadIdx.x;
        if (i >= n || val[i] == 0u) continue;
        const uint32_t mine = key[i];
        uint32_t a = 0, b = i;          // first position in [0, i] whose key is not below mine
        while (a < b) {
            const uint32_t m = a + (b - a) / 2;
            if (key[m] < mine) a = m + 1; else b = m;
        }
        const uint32_t lo = a;
        a = i + 1; b = n;               // first position in (i, n] whose key is above mine
        while (a < b) {
            const uint32_t m = a + (b - a) / 2;
            if (key[m] <= mine) a = m + 1; else b = m;
        }
        sum += static_cast<unsigned long long>(negprefix[lo]) + negprefix[a];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = kMetricThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < static_cast<unsigned>(o)) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0] != 0ull) atomicAdd(&u2[blockIdx.y], part[0]);
}

inline size_t up256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
struct AucLayout { size_t ka, kb, va, vb, hist, tiles, prefix, bytes; uint32_t n_tiles; };
AucLayout auc_layout(int n, int D) {
    AucLayout L{};
    const size_t cells = static_cast<size_t>(n) * D;
    L.n_tiles = radix_sort_tiles(static_cast<size_t>(n));
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += up256(b); return at; };
    L.ka = take(4 * cells); L.kb = take(4 * cells); L.va = take(4 * cells); L.vb = take(4 * cells);
    L.hist = take(4 * 256 * static_cast<size_t>(L.n_tiles) * D);
    L.tiles = take(4 * static_cast<size_t>(L.n_tiles) * D);
    L.prefix = take(4 * (static_cast<size_t>(n) + 1) * D);
    L.bytes = o;
    return L;
}

}  // namespace

void metric_error(int objective, const float *P, const void *T, int n, int D, unsigned long long *wrong, hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid((static_cast<unsigned>(n) + kMetricThreads - 1) / kMetricThreads);
    if (objective == kObjSoftmax) hipLaunchKernelGGL(k_metric_error<true>, grid, dim3(kMetricThreads), 0, s, P, T, n, D, wrong);
    else hipLaunchKernelGGL(k_metric_error<false>, grid, dim3(kMetricThreads), 0, s, P, T, n, D, wrong);
}

bool metric_auc_fits(int n, int D) {
    return n > 0 && D > 0 && D <= kMetricMaxD && static_cast<size_t>(n) * D < (size_t(1) << 31) - kRadixSortTile;
}

size_t metric_auc_scratch_bytes(int n, int D) { return auc_layout(n, D).bytes; }

void metric_positives(const float *Y, int n, int D, unsigned long long *pos, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_auc_keys, dim3((static_cast<unsigned>(n) + kMetricThreads - 1) / kMetricThreads), dim3(kMetricThreads), 0, s, nullptr, Y,
                       static_cast<uint32_t>(n), D, nullptr, nullptr, pos);
}

void metric_auc(const float *P, const float *Y, int n, int D, void *scratch, unsigned long long *pos, unsigned long long *u2, hipStream_t s) {
    if (n <= 0) return;
    const AucLayout L = auc_layout(n, D);
    char *base = static_cast<char *>(scratch);
    uint32_t *ka = reinterpret_cast<uint32_t *>(base + L.ka), *kb = reinterpret_cast<uint32_t *>(base + L.kb);
    uint32_t *va = reinterpret_cast<uint32_t *>(base + L.va), *vb = reinterpret_cast<uint32_t *>(base + L.vb);
    uint32_t *hist = reinterpret_cast<uint32_t *>(base + L.hist), *tiles = reinterpret_cast<uint32_t *>(base + L.tiles);
    uint32_t *prefix = reinterpret_cast<uint32_t *>(base + L.prefix);
    const uint32_t un = static_cast<uint32_t>(n);
    hipLaunchKernelGGL(k_auc_keys, dim3((un + kMetricThreads - 1) / kMetricThreads), dim3(kMetricThreads), 0, s, P, Y, un, D, ka, va, pos);
    for (int shift = 0; shift < 32; shift += 8) {
        radix_sort_pass(ka, va, un, D, shift, hist, kb, vb, s);
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    const dim3 grid(L.n_tiles, static_cast<unsigned>(D));
    hipLaunchKernelGGL(k_auc_neg_tiles, grid, dim3(kMetricThreads), 0, s, va, un, L.n_tiles, tiles);
    hipLaunchKernelGGL(k_auc_neg_scan, dim3(static_cast<unsigned>(D)), dim3(kMetricThreads), 0, s, tiles, L.n_tiles);
    hipLaunchKernelGGL(k_auc_neg_prefix, grid, dim3(kMetricThreads), 0, s, va, un, L.n_tiles, tiles, prefix);
    hipLaunchKernelGGL(k_auc_pairs, grid, dim3(kMetricThreads), 0, s, ka, va, un, prefix, u2);
}

}  // namespace kern
}  // namespace gbrl
