// radix_sort.hip -- stable LSD radix sort of (key, value) pairs of 32 bits each, 8 bits per pass, over `segments` independent arrays of n
// elements laid out one behind the other ([segments][n]).  A pass is three launches on one stream:
//   k_radix_hist     block (tile, segment): the digit counts of the tile's kRadixSortTile elements, stored digit-major per segment
//                    ([segment][digit][tile]), so that
//   k_radix_scan     one block per segment, an exclusive scan over the segment's 256 * n_tiles counts, IS the output offset of every
//                    (digit, tile) relative to the segment's base
//   k_radix_scatter  block (tile, segment): the stable scatter of the tile
// kern::cat_rank sorts its cells with one segment (and as many passes as its keys have digits); kern::metric_auc sorts the D score columns of
// a prediction matrix with four.  Every index is below segments * n, which the callers keep below 2^31 - kRadixSortTile.
#include "kernels.h"
#include "kernels_common.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kRadixThreads = 256;        // four waves
constexpr int kRadixRounds = 8;           // elements per thread and tile
constexpr int kRadixTile = kRadixThreads * kRadixRounds;
static_assert(kRadixTile == kRadixSortTile, "kernels.h names the tile");

__global__ __launch_bounds__(kRadixThreads) void k_radix_hist(const uint32_t *__restrict__ key, uint32_t n, int shift, uint32_t n_tiles,
                                                              uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    key += static_cast<size_t>(blockIdx.y) * n;
    hist += static_cast<size_t>(blockIdx.y) * 256u * n_tiles;
    const uint32_t t0 = blockIdx.x * static_cast<uint32_t>(kRadixTile);
    for (int r = 0; r < kRadixRounds; ++r) {
        const uint32_t i = t0 + r * kRadixThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[static_cast<size_t>(threadIdx.x) * n_tiles + blockIdx.x] = h[threadIdx.x];
}
// The counts of a segment in slices of kScanSlice consecutive words, kScanPer per thread: neighbouring threads read neighbouring words, the
// scan inside a wave is a shuffle scan of the threads' sums, the waves meet in LDS, and a carry runs from slice to slice (the way
// sample_rows.hip places its block counts).  The next slice is loaded before the current one is scanned.
constexpr int kScanThreads = 1024, kScanPer = 4, kScanSlice = kScanThreads * kScanPer;
__global__ __launch_bounds__(kScanThreads) void k_radix_scan(uint32_t *__restrict__ hist, uint32_t total) {
    constexpr int kWaves = kScanThreads / kWave;
    __shared__ uint32_t s_tot[kWaves];
    hist += static_cast<size_t>(blockIdx.x) * total;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t mine = threadIdx.x * static_cast<uint32_t>(kScanPer);
    uint32_t nxt[kScanPer];
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) nxt[j] = mine + j < total ? hist[mine + j] : 0u;
    uint32_t carry = 0;   // the counts of every slice before this one (the same in every thread)
    for (uint32_t b0 = 0; b0 < total; b0 += kScanSlice) {
        uint32_t c[kScanPer], sum = 0;
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) { c[j] = nxt[j]; sum += c[j]; }
        const uint32_t ahead = b0 + kScanSlice + mine;
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) nxt[j] = ahead + j < total ? hist[ahead + j] : 0u;
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == kWave - 1) s_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, slice = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t t = s_tot[w];
            before += w < wave ? t : 0u;
            slice += t;
        }
        uint32_t run = carry + before + incl - sum;
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            if (b0 + mine + j < total) hist[b0 + mine + j] = run;
            run += c[j];
        }
        carry += slice;
        __syncthreads();   // s_tot is rewritten by the next slice
    }
}
// One tile per block, in kRadixRounds rounds of 256 consecutive elements.  Inside a round the position of an element is
//   run[digit] (everything before this round) + the counts of the digit in the lower waves + its rank among the wave's lanes with the digit,
// the latter from ballots over the digit's bits (wave64: the lanes below mine that hold my digit).
__global__ __launch_bounds__(kRadixThreads) void k_radix_scatter(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t n,
                                                                 int shift, uint32_t n_tiles, const uint32_t *__restrict__ hist,
                                                                 uint32_t *__restrict__ key_out, uint32_t *__restrict__ val_out) {
    constexpr int kWaves = kRadixThreads / kWave;
    __shared__ uint32_t run[256];
    __shared__ uint32_t wcnt[kWaves][256];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const size_t seg = static_cast<size_t>(blockIdx.y) * n;
    key += seg; val += seg; key_out += seg; val_out += seg;
    hist += static_cast<size_t>(blockIdx.y) * 256u * n_tiles;
    run[tid] = hist[static_cast<size_t>(tid) * n_tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const uint32_t t0 = blockIdx.x * static_cast<uint32_t>(kRadixTile);
    for (int r = 0; r < kRadixRounds; ++r) {
        const uint32_t i = t0 + r * kRadixThreads + tid;
        const bool valid = i < n;
        const uint32_t k = valid ? key[i] : 0u, v = valid ? val[i] : 0u;
        const uint32_t d = (k >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long m = __ballot(valid && one);
            peers &= one ? m : ~m;
        }
        const int below = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && below == 0) wcnt[wave][d] = static_cast<uint32_t>(__popcll(peers));
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + static_cast<uint32_t>(below);
            for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
            if (pos < n) { key_out[pos] = k; val_out[pos] = v; }   // (pos < n always: the offsets are a permutation of [0, n))
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { add += wcnt[w][tid]; wcnt[w][tid] = 0; }
        run[tid] += add;
        __syncthreads();
    }
}

}  // namespace

uint32_t radix_sort_tiles(size_t n) { return static_cast<uint32_t>((n + kRadixTile - 1) / kRadixTile); }

void radix_sort_pass(const uint32_t *key, const uint32_t *val, uint32_t n, int segments, int shift, uint32_t *hist, uint32_t *key_out, uint32_t *val_out,
                     hipStream_t s) {
    if (n == 0 || segments <= 0) return;
    const uint32_t n_tiles = radix_sort_tiles(n);
    const dim3 grid(n_tiles, static_cast<unsigned>(segments));
    hipLaunchKernelGGL(k_radix_hist, grid, dim3(kRadixThreads), 0, s, key, n, shift, n_tiles, hist);
    hipLaunchKernelGGL(k_radix_scan, dim3(static_cast<unsigned>(segments)), dim3(kScanThreads), 0, s, hist, 256u * n_tiles);
    hipLaunchKernelGGL(k_radix_scatter, grid, dim3(kRadixThreads), 0, s, key, val, n, shift, n_tiles, hist, key_out, val_out);
}

}  // namespace kern
}  // namespace gbrl
