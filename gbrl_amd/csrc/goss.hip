// goss.hip -- gfx950 kernels of one-side sampling (sample_core.h: GOSS) in front of the sampler's passes (sample_rows.hip): the scores and keys of a
// batch's gradient rows and the EXACT k-th largest key, left in device memory.
//
// The selection is an MSD radix count over the 32-bit keys, kGossDigitBits = 8 bits a pass, integer counts only:
//   k_goss_score     one thread per row: s = goss_score(row) by sample_core.h's float32 multiply and add (never contracted), key = bits & 0x7FFFFFFF
//                    stored to keys[]; the same pass counts digit 0 (the key's top 8 bits) -- an LDS histogram per block, its non-zero counters added
//                    to hist[0] by integer atomics (a sum of integers: the order of arrival does not show).
//   k_goss_hist<P>   P = 1, 2, 3: every block first RESOLVES the passes before it from their finished histograms (goss_resolve: a suffix scan of
//                    256 counters from the top digit down finds the digit that holds the k-th largest key, the keys above it are counted off
//                    k), then counts digit P of the keys whose upper digits are that prefix.  No pick kernel between the passes, no block waits.
//   k_goss_ties      resolves all four passes: tau = the prefix, n_gt = #{key > tau}, take = k - n_gt; block b (the SAMPLER's block: the same
//                    kSampleRowsPerBlock rows) counts its keys == tau into tie_cnt[b]; block 0 stores {tau, n_gt, take, k} to `state`.  k == 0: no pass
//                    runs, tau = kGossNoTau (above every key), no ties.
// Ties are the normal case (the first tree of a softmax fit: every row of a class has one gradient), so a wave whose 64 keys fall into one counter
// adds its lane count once (the ballot test radix_select.hip uses); otherwise one LDS atomic per lane.  8-bit digits keep the histogram at 1 KiB
// and the resolve at one counter per thread; 11-bit digits would save one launch for eight counters per thread and 8 KiB.
// Reads stay below key n and row n of G; hist / state / tie_cnt are the caller's scratch (goss_scratch).
#include "kernels.h"
#include "sample_core.h"

namespace gbrl {
namespace kern {

namespace {

constexpr int kGossThreads = 256, kGossWaves = kGossThreads / 64;
constexpr int kGossRowsPerBlock = 4096, kGossSweeps = kGossRowsPerBlock / kGossThreads;   // score and count passes (few blocks: few global atomics)
constexpr int kTieSweeps = kSampleRowsPerBlock / kGossThreads;
static_assert(kGossDigits == kGossThreads, "the resolve scans one counter per thread");

// one key's digit into the block's LDS histogram; idx < 0: nothing.  Every lane of the wave calls it.
__device__ __forceinline__ void count_digit(uint32_t *cnt, int idx) {
    const int first = __builtin_amdgcn_readfirstlane(idx);
    const unsigned long long active = __ballot(1), same = __ballot(idx == first);
    if (same == active) {
        if (first >= 0 && __lane_id() == static_cast<unsigned>(__ffsll(static_cast<long long>(active)) - 1)) atomicAdd(&cnt[first], static_cast<uint32_t>(__popcll(active)));
    } else if (idx >= 0) {
        atomicAdd(&cnt[idx], 1u);
    }
}

__device__ __forceinline__ void flush_digits(const uint32_t *cnt, uint32_t *hist) {
    __syncthreads();
    const uint32_t c = cnt[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

// The first `passes` digits of the k-th largest key (k >= 1) from their histograms: prefix = those digits, n_gt = the keys above every key with
// that prefix, k_rem = the rank left inside it (>= 1).  Every thread of the block calls it and gets the same values.
__device__ __forceinline__ void goss_resolve(const uint32_t *hist, int passes, uint32_t k, uint32_t &prefix, uint32_t &n_gt, uint32_t &k_rem) {
    __shared__ uint32_t s_tot[kGossWaves], s_pick[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    prefix = 0; n_gt = 0; k_rem = k;
    for (int q = 0; q < passes; ++q) {
        const uint32_t digit = static_cast<uint32_t>(kGossDigits - 1) - threadIdx.x;   // thread 0 holds the top digit
        const uint32_t c = hist[q * kGossDigits + digit];
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_tot[wave] = incl;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kGossWaves; ++w) incl += w < wave ? s_tot[w] : 0u;
        // incl = the keys of this level with a digit >= mine: exactly one thread has incl >= k_rem > incl - c
        if (incl >= k_rem && incl - c < k_rem) { s_pick[0] = digit; s_pick[1] = incl - c; }
        __syncthreads();
        prefix = (prefix << kGossDigitBits) | s_pick[0];
        n_gt += s_pick[1];
        k_rem -= s_pick[1];
        __syncthreads();   // s_tot and s_pick are rewritten by the next level
    }
}

template <bool kVec>
__global__ __launch_bounds__(kGossThreads) void k_goss_score(const float *__restrict__ G, uint32_t n, int D, uint32_t *__restrict__ keys, uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_cnt[kGossDigits];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * static_cast<uint32_t>(kGossRowsPerBlock) + threadIdx.x;   // (n < 2^31: no wrap)
    for (int sw = 0; sw < kGossSweeps; ++sw) {
        const uint32_t i = base + static_cast<uint32_t>(sw * kGossThreads);
        int digit = -1;
        if (i < n) {
            float s = 0.0f;
            if (kVec) {
                const int D4 = D >> 2;
                const float4 *row = reinterpret_cast<const float4 *>(G) + static_cast<size_t>(i) * D4;
                for (int q = 0; q < D4; ++q) {
                    const float4 v = row[q];
                    s = goss_score_add(goss_score_add(goss_score_add(goss_score_add(s, v.x), v.y), v.z), v.w);
                }
            } else {
                s = goss_score(G + static_cast<size_t>(i) * D, D);
            }
            const uint32_t key = goss_key(s);
            keys[i] = key;
            digit = static_cast<int>(key >> (32 - kGossDigitBits));
        }
        count_digit(s_cnt, digit);
    }
    flush_digits(s_cnt, hist);
}

template <int PASS>
__global__ __launch_bounds__(kGossThreads) void k_goss_hist(const uint32_t *__restrict__ keys, uint32_t n, uint32_t k, uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_cnt[kGossDigits];
    s_cnt[threadIdx.x] = 0;   // (the resolve's barriers come before the first count)
    uint32_t prefix, n_gt, k_rem;
    goss_resolve(hist, PASS, k, prefix, n_gt, k_rem);
    constexpr int kUpper = 32 - PASS * kGossDigitBits, kShift = kUpper - kGossDigitBits;
    const uint32_t base = blockIdx.x * static_cast<uint32_t>(kGossRowsPerBlock) + threadIdx.x;
#pragma unroll 4
    for (int sw = 0; sw < kGossSweeps; ++sw) {
        const uint32_t i = base + static_cast<uint32_t>(sw * kGossThreads);
        int digit = -1;
        if (i < n) {
            const uint32_t key = keys[i];
            if ((key >> kUpper) == prefix) digit = static_cast<int>((key >> kShift) & (kGossDigits - 1));
        }
        count_digit(s_cnt, digit);
    }
    flush_digits(s_cnt, hist + PASS * kGossDigits);
}

__global__ __launch_bounds__(kGossThreads) void k_goss_ties(const uint32_t *__restrict__ keys, uint32_t n, uint32_t k, const uint32_t *__restrict__ hist,
                                                            uint32_t *__restrict__ state, int32_t *__restrict__ tie_cnt) {
    __shared__ int s_wave[kGossWaves];
    uint32_t tau = kGossNoTau, n_gt = 0, take = 0;
    if (k > 0) goss_resolve(hist, kGossPasses, k, tau, n_gt, take);   // (k is the same in every thread)
    const uint32_t base = blockIdx.x * static_cast<uint32_t>(kSampleRowsPerBlock) + threadIdx.x;
    int cnt = 0;
#pragma unroll
    for (int sw = 0; sw < kTieSweeps; ++sw) {
        const uint32_t i = base + static_cast<uint32_t>(sw * kGossThreads);
        const bool tie = i < n && keys[i] == tau;
        cnt += __popcll(__ballot(tie));
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kGossWaves; ++w) tot += s_wave[w];
        tie_cnt[blockIdx.x] = tot;
        if (blockIdx.x == 0) { state[0] = tau; state[1] = n_gt; state[2] = take; state[3] = k; }
    }
}

}  // namespace

size_t goss_scratch_words(int n) {
    return 6 + static_cast<size_t>(kGossPasses) * kGossDigits + 2 * static_cast<size_t>(sample_rows_blocks(n)) + static_cast<size_t>(n > 0 ? n : 0);
}

GossScratch goss_scratch(int32_t *words, int n) {
    const size_t n_blk = static_cast<size_t>(sample_rows_blocks(n));
    GossScratch gs;
    gs.m_out = words;
    gs.state = reinterpret_cast<uint32_t *>(words + 2);
    gs.hist = reinterpret_cast<uint32_t *>(words + 6);
    gs.tie_off = words + 6 + kGossPasses * kGossDigits;
    gs.blk = gs.tie_off + n_blk;
    gs.keys = reinterpret_cast<uint32_t *>(gs.blk + n_blk);
    return gs;
}

void goss_select(int n, int k, const float *G, int D, const GossScratch &gs, hipStream_t s) {
    if (n <= 0) return;
    const uint32_t un = static_cast<uint32_t>(n), uk = static_cast<uint32_t>(k);
    const int n_cnt = static_cast<int>((static_cast<int64_t>(n) + kGossRowsPerBlock - 1) / kGossRowsPerBlock);
    (void)hipMemsetAsync(gs.hist, 0, sizeof(uint32_t) * kGossPasses * kGossDigits, s);   // (an error surfaces through hipGetLastError in the engine)
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(G) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(k_goss_score<true>, dim3(n_cnt), dim3(kGossThreads), 0, s, G, un, D, gs.keys, gs.hist);
    else hipLaunchKernelGGL(k_goss_score<false>, dim3(n_cnt), dim3(kGossThreads), 0, s, G, un, D, gs.keys, gs.hist);
    if (k > 0) {
        hipLaunchKernelGGL(k_goss_hist<1>, dim3(n_cnt), dim3(kGossThreads), 0, s, gs.keys, un, uk, gs.hist);
        hipLaunchKernelGGL(k_goss_hist<2>, dim3(n_cnt), dim3(kGossThreads), 0, s, gs.keys, un, uk, gs.hist);
        hipLaunchKernelGGL(k_goss_hist<3>, dim3(n_cnt), dim3(kGossThreads), 0, s, gs.keys, un, uk, gs.hist);
    }
    hipLaunchKernelGGL(k_goss_ties, dim3(sample_rows_blocks(n)), dim3(kGossThreads), 0, s, gs.keys, un, uk, gs.hist, gs.state, gs.tie_off);
}

void sample_goss(int row0, int n, int k, uint32_t thr, float amp, uint64_t seed, int32_t draw, const float *G, int D, int32_t *rows_out, float *factor_out,
                 float *G_out, const float *weights, float *eff_out, const GossScratch &gs, hipStream_t s) {
    goss_select(n, k, G, D, gs, s);
    goss_sample_passes(row0, n, thr, amp, seed, draw, gs, G, D, rows_out, factor_out, G_out, weights, eff_out, s);
}

}  // namespace kern
}  // namespace gbrl
