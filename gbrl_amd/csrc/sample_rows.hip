// sample_rows.hip -- gfx950 kernels of the row sampler (sample_core.h): the kept rows of [row0, row0 + n) as an ascending index vector and,
// in the same pass, the gathered rows of a matrix (fit_prepared's batch gradients).
//
// The position of a kept row is its RANK among the kept rows, so the output does not depend on scheduling: no atomic hands out a position and
// no block waits for another.  Three launches on one stream:
//   k_sample_count   block b owns the kSampleRowsPerBlock consecutive rows from b * kSampleRowsPerBlock, in kSampleSweeps sweeps of 256: in a
//                    sweep lane l of wave w looks at row base + 256 sweep + 64 w + l, so the 64-bit __ballot of the keep flags IS the wave's
//                    piece of the flag vector in row order.  The block's count is the sum of the popcounts.  The flags are never stored.
//   k_sample_scan    ONE block walks the block counts kSampleScanWidth at a time (shuffle scan within a wave, the wave totals through LDS, a
//                    carry from slice to slice) and turns them into exclusive offsets in place; the total m lands in a word of its own, which
//                    the host reads back (4 bytes).  Any n up to 2^31 - 1: 2^20 block counts are 2048 slices.
//   k_sample_write   recomputes the hash.  The rank of a kept row inside its block is (kept rows of the (sweep, wave) pieces before its piece)
//                    + popcount(ballot below the lane); the block collects its kept LOCAL indices in LDS in that order and then writes
//                    rows_out[off + j] = row0 + base + local[j] and G_out[off + j][:] = G[base + local[j]][:] with consecutive threads on
//                    consecutive words: 16-byte accesses when D % 4 == 0 and both matrices are 16-byte aligned, 4-byte accesses otherwise.
// Reads stay below row n of G (a row is kept only if it is below n), writes below row m of the outputs (an offset is a count of kept rows).
//
// The count and the write kernel take their keep predicate from a RULE: HashRule is the sampler above (its instantiations are the kernels as they
// were); GossRule is sample_core.h's one-side rule behind goss.hip's selection -- a row is kept iff it is TOP (its key above tau, or equal to tau
// with a tie rank below `take`) or its hash of the "gossrest" stream is below the threshold.  The tie rank of a row is (ties of the blocks before:
// tie_off, an exclusive scan of goss.hip's tie counts by k_sample_scan) + (ties of the block's pieces before its piece) + popcount(tie ballot
// below the lane): a rank again, so the scan of the tie counts comes BEFORE the count of the kept rows.  The write pass then also stores the
// factor of every kept row (1 or amp), applies it to the gathered gradient row (a top row is copied: no bit changes) and, for fit_prepared's
// Newton sums, stores the effective weight fl32(w * amp) (top: w) by ABSOLUTE row.
#include "kernels.h"
#include "sample_core.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

constexpr int kSampleThreads = 256, kSampleWaves = kSampleThreads / 64;
constexpr int kSampleSweeps = kSampleRowsPerBlock / kSampleThreads;
constexpr int kSamplePieces = kSampleSweeps * kSampleWaves;   // (sweep, wave) pieces of a block, in row order
static_assert(kSampleRowsPerBlock % kSampleThreads == 0 && kSampleSweeps <= 32, "the keep flags of a thread's rows live in one 32-bit word");
static_assert(kSampleScanWidth % 64 == 0 && kSampleScanWidth <= 1024, "the scan block is whole waves");

struct SampleArgs { uint64_t seed; uint32_t row0, n, thr; int32_t draw; };

// the keep flags of this thread's kSampleSweeps rows of block `blk`, bit k = sweep k
__device__ __forceinline__ uint32_t keep_bits(const SampleArgs &a, uint32_t blk) {
    uint32_t bits = 0;
    const uint32_t base = blk * static_cast<uint32_t>(kSampleRowsPerBlock) + threadIdx.x;   // (n < 2^31: no wrap)
#pragma unroll
    for (int k = 0; k < kSampleSweeps; ++k) {
        const uint32_t i = base + static_cast<uint32_t>(k * kSampleThreads);
        const bool keep = i < a.n && sample_keeps(a.seed, a.draw, a.row0 + i, a.thr);
        bits |= (keep ? 1u : 0u) << k;
    }
    return bits;
}

// the sampler's own rule: the hash of (seed, draw, row) below the threshold
struct HashRule {
    static constexpr bool kGoss = false;
    SampleArgs a;
    __device__ __forceinline__ uint32_t keep(uint32_t blk, uint32_t &top) const { top = 0; return keep_bits(a, blk); }
};

// the one-side rule; a.seed is already the "gossrest" stream's.  Every thread of the block calls keep() (it synchronises the block).
struct GossRule {
    static constexpr bool kGoss = true;
    SampleArgs a;
    const uint32_t *keys;      // [n]
    const uint32_t *state;     // goss.hip: {tau, #{key > tau}, take}
    const int32_t *tie_off;    // [blocks]: ties in the blocks before
    float amp;
    float *factor_out;         // [m] (write pass)
    const float *weights;      // by absolute row, nullable: 1
    float *eff_out;            // by absolute row, nullable
    __device__ __forceinline__ uint32_t keep(uint32_t blk, uint32_t &top) const {
        __shared__ int s_tie[kSamplePieces];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint32_t tau = state[0], take = state[2];
        const uint32_t base = blk * static_cast<uint32_t>(kSampleRowsPerBlock) + threadIdx.x;
        uint32_t above = 0, tie = 0, hash = 0;
#pragma unroll
        for (int k = 0; k < kSampleSweeps; ++k) {
            const uint32_t i = base + static_cast<uint32_t>(k * kSampleThreads);
            if (i < a.n) {
                const uint32_t key = keys[i];
                above |= (key > tau ? 1u : 0u) << k;
                tie |= (key == tau ? 1u : 0u) << k;
                hash |= (sample_keeps(a.seed, a.draw, a.row0 + i, a.thr) ? 1u : 0u) << k;
            }
        }
#pragma unroll
        for (int k = 0; k < kSampleSweeps; ++k) {
            const int c = __popcll(__ballot((tie >> k) & 1u));
            if (lane == 0) s_tie[k * kSampleWaves + wave] = c;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int run = tie_off[blk];
            for (int p = 0; p < kSamplePieces; ++p) { const int c = s_tie[p]; s_tie[p] = run; run += c; }
        }
        __syncthreads();
        const unsigned long long below = (1ull << lane) - 1ull;
        top = above;
#pragma unroll
        for (int k = 0; k < kSampleSweeps; ++k) {
            const unsigned long long mask = __ballot((tie >> k) & 1u);
            const uint32_t rank = static_cast<uint32_t>(s_tie[k * kSampleWaves + wave] + __popcll(mask & below));
            top |= (((tie >> k) & 1u) && rank < take ? 1u : 0u) << k;
        }
        __syncthreads();   // s_tie may be written again by a second call
        return top | hash;
    }
};

template <class Rule>
__global__ __launch_bounds__(kSampleThreads) void k_sample_count(Rule r, int32_t *__restrict__ blk_count) {
    __shared__ int s_wave[kSampleWaves];
    uint32_t top;
    const uint32_t bits = r.keep(blockIdx.x, top);
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kSampleSweeps; ++k) cnt += __popcll(__ballot((bits >> k) & 1u));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kSampleWaves; ++w) tot += s_wave[w];
        blk_count[blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(kSampleScanWidth) void k_sample_scan(int32_t *__restrict__ blk /*[n_blk]: counts in, exclusive offsets out*/, int n_blk,
                                                                  int32_t *__restrict__ m_out) {
    constexpr int kWaves = kSampleScanWidth / 64;
    __shared__ int s_tot[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;   // kept rows of every slice before this one (the same in every thread)
    for (int b0 = 0; b0 < n_blk; b0 += kSampleScanWidth) {
        const int b = b0 + static_cast<int>(threadIdx.x);
        const int c = b < n_blk ? blk[b] : 0;
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_tot[wave] = incl;
        __syncthreads();
        int before = 0, slice = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int t = s_tot[w];
            before += w < wave ? t : 0;
            slice += t;
        }
        if (b < n_blk) blk[b] = carry + before + incl - c;
        carry += slice;
        __syncthreads();   // s_tot is rewritten by the next slice
    }
    if (threadIdx.x == 0) *m_out = carry;
}

template <class Rule, bool kVec>
__global__ __launch_bounds__(kSampleThreads) void k_sample_write(Rule r, const int32_t *__restrict__ blk_off, int32_t *__restrict__ rows_out,
                                                                 const float *__restrict__ G, int D, float *__restrict__ G_out) {
    constexpr uint16_t kTopFlag = 0x8000, kLocalMask = 0x7fff;   // GossRule: bit 15 of a kept local index marks a top row
    static_assert(kSampleRowsPerBlock <= 0x8000, "a local index and the top flag share 16 bits");
    const SampleArgs &a = r.a;
    __shared__ int s_piece[kSamplePieces];                 // kept rows per (sweep, wave) piece, then their exclusive prefix
    __shared__ uint16_t s_local[kSampleRowsPerBlock];      // the block's kept local indices, ascending
    __shared__ int s_cnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t top;
    const uint32_t bits = r.keep(blockIdx.x, top);
#pragma unroll
    for (int k = 0; k < kSampleSweeps; ++k) {
        const int c = __popcll(__ballot((bits >> k) & 1u));
        if (lane == 0) s_piece[k * kSampleWaves + wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int p = 0; p < kSamplePieces; ++p) { const int c = s_piece[p]; s_piece[p] = run; run += c; }
        s_cnt = run;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < kSampleSweeps; ++k) {
        const unsigned long long mask = __ballot((bits >> k) & 1u);
        uint16_t local = static_cast<uint16_t>(k * kSampleThreads + threadIdx.x);
        if (Rule::kGoss && ((top >> k) & 1u)) local |= kTopFlag;
        if ((bits >> k) & 1u) s_local[s_piece[k * kSampleWaves + wave] + __popcll(mask & below)] = local;
    }
    __syncthreads();
    const int cnt = s_cnt;
    const size_t off = static_cast<size_t>(blk_off[blockIdx.x]);
    const uint32_t base = blockIdx.x * static_cast<uint32_t>(kSampleRowsPerBlock);
    if constexpr (!Rule::kGoss) {
        for (int j = threadIdx.x; j < cnt; j += kSampleThreads) rows_out[off + j] = static_cast<int32_t>(a.row0 + base + s_local[j]);
    } else {
        for (int j = threadIdx.x; j < cnt; j += kSampleThreads) {
            const uint16_t l = s_local[j];
            const bool is_top = (l & kTopFlag) != 0;
            const uint32_t row = a.row0 + base + (l & kLocalMask);
            rows_out[off + j] = static_cast<int32_t>(row);
            r.factor_out[off + j] = is_top ? 1.0f : r.amp;
            if (r.eff_out) {
                const float w = r.weights ? r.weights[row] : 1.0f;
                r.eff_out[row] = is_top ? w : obj_weighted(w, r.amp);
            }
        }
    }
    if (G == nullptr) return;
    if (kVec) {
        const int D4 = D >> 2;
        const uint4 *src = reinterpret_cast<const uint4 *>(G) + static_cast<size_t>(base) * D4;
        uint4 *dst = reinterpret_cast<uint4 *>(G_out) + off * D4;
        const int total = cnt * D4;   // at most 2048 * 128
        for (int e = threadIdx.x; e < total; e += kSampleThreads) {
            const int j = e / D4, d = e - j * D4;
            if constexpr (!Rule::kGoss) {
                dst[e] = src[static_cast<size_t>(s_local[j]) * D4 + d];
            } else {
                const uint16_t l = s_local[j];
                uint4 v = src[static_cast<size_t>(l & kLocalMask) * D4 + d];
                if (!(l & kTopFlag)) {
                    v.x = __float_as_uint(obj_weighted(r.amp, __uint_as_float(v.x))); v.y = __float_as_uint(obj_weighted(r.amp, __uint_as_float(v.y)));
                    v.z = __float_as_uint(obj_weighted(r.amp, __uint_as_float(v.z))); v.w = __float_as_uint(obj_weighted(r.amp, __uint_as_float(v.w)));
                }
                dst[e] = v;
            }
        }
    } else {
        const float *src = G + static_cast<size_t>(base) * D;
        float *dst = G_out + off * D;
        const int total = cnt * D;    // at most 2048 * 512
        for (int e = threadIdx.x; e < total; e += kSampleThreads) {
            const int j = e / D, d = e - j * D;
            if constexpr (!Rule::kGoss) {
                dst[e] = src[static_cast<size_t>(s_local[j]) * D + d];
            } else {
                const uint16_t l = s_local[j];
                const float g = src[static_cast<size_t>(l & kLocalMask) * D + d];
                dst[e] = (l & kTopFlag) ? g : obj_weighted(r.amp, g);
            }
        }
    }
}

}  // namespace

int sample_rows_blocks(int n) { return n <= 0 ? 0 : static_cast<int>((static_cast<int64_t>(n) + kSampleRowsPerBlock - 1) / kSampleRowsPerBlock); }

void sample_rows(int row0, int n, uint32_t thr, uint64_t seed, int32_t draw, const float *G, int D, int32_t *rows_out, float *G_out, int32_t *scratch,
                 hipStream_t s) {
    if (n <= 0) return;
    const int n_blk = sample_rows_blocks(n);
    const HashRule a{SampleArgs{seed, static_cast<uint32_t>(row0), static_cast<uint32_t>(n), thr, draw}};
    int32_t *m_out = scratch, *blk = scratch + 1;
    hipLaunchKernelGGL(k_sample_count<HashRule>, dim3(n_blk), dim3(kSampleThreads), 0, s, a, blk);
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(kSampleScanWidth), 0, s, blk, n_blk, m_out);
    const bool gather = G != nullptr && G_out != nullptr && D > 0;
    const bool vec = gather && D % 4 == 0 && ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(G_out)) & 15u) == 0;
    if (vec) hipLaunchKernelGGL((k_sample_write<HashRule, true>), dim3(n_blk), dim3(kSampleThreads), 0, s, a, blk, rows_out, G, D, G_out);
    else hipLaunchKernelGGL((k_sample_write<HashRule, false>), dim3(n_blk), dim3(kSampleThreads), 0, s, a, blk, rows_out, gather ? G : nullptr, D, G_out);
}

void goss_sample_passes(int row0, int n, uint32_t thr, float amp, uint64_t seed, int32_t draw, const GossScratch &gs, const float *G, int D, int32_t *rows_out,
                        float *factor_out, float *G_out, const float *weights, float *eff_out, hipStream_t s) {
    if (n <= 0) return;
    const int n_blk = sample_rows_blocks(n);
    const GossRule r{SampleArgs{seed ^ kGossStream, static_cast<uint32_t>(row0), static_cast<uint32_t>(n), thr, draw},
                     gs.keys, gs.state, gs.tie_off, amp, factor_out, weights, eff_out};
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(kSampleScanWidth), 0, s, gs.tie_off, n_blk, gs.m_out + 1);   // the tie counts -> the ties before a block
    hipLaunchKernelGGL(k_sample_count<GossRule>, dim3(n_blk), dim3(kSampleThreads), 0, s, r, gs.blk);
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(kSampleScanWidth), 0, s, gs.blk, n_blk, gs.m_out);
    const bool gather = G != nullptr && G_out != nullptr && D > 0;
    const bool vec = gather && D % 4 == 0 && ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(G_out)) & 15u) == 0;
    if (vec) hipLaunchKernelGGL((k_sample_write<GossRule, true>), dim3(n_blk), dim3(kSampleThreads), 0, s, r, gs.blk, rows_out, G, D, G_out);
    else hipLaunchKernelGGL((k_sample_write<GossRule, false>), dim3(n_blk), dim3(kSampleThreads), 0, s, r, gs.blk, rows_out, gather ? G : nullptr, D, G_out);
}

}  // namespace kern
}  // namespace gbrl
