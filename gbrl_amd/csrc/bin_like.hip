// bin_like.hip -- gfx950 kernel behind a data set bound to another data set's thresholds (Engine::prepare_dataset_like): rows that the
// thresholds were NOT made from are put on them.  Row-major float32 obs [n][F] becomes the group-major code records [G][n][16] u16 of
// kern::bin_cols in one pass: no transposed key copy, no selection.
//
//   code(r, f) = min(B, #{b : thr_keys[f][b] < float_to_key(obs[r][f])})      (-0.0 == +0.0; NaN has key 0: code 0)
//
//   k_bin_like<LDS>   block = one group of 16 features x tiles of 256 rows, thread = row.  The row's 16 floats of the group are 64 contiguous
//                     bytes: four 16-byte loads where F % 4 == 0 and obs is 16-byte aligned (a piece then lies wholly inside or wholly outside
//                     the row, also in the last group), scalar loads otherwise; all of them are in flight before the first search.  The search
//                     is a branch-free lower bound over the feature's ascending keys, eight features of a row in flight: count += step while
//                     count + step <= B and key[count + step - 1] < x, step = top, top / 2, .., 1 with top the largest power of two <= B, so
//                     the count can reach 2 top - 1 >= B and never exceeds B (the bound check is k_bin_cols' pad with the maximal key and its
//                     min(code, B)).  The record leaves as two 16-byte stores of ONE lane: lane i of a wave writes bytes [32 i, 32 i + 32) of a
//                     2 KiB run.  Padding slots (f >= F) are zero; their searches read the group's last real feature and are discarded.
//                     LDS = true: the group's keys, 16 * B * 4 bytes, staged once per block and reused for up to kLikeTiles tiles.
//                     LDS = false: the same search in global memory -- bin counts whose keys do not fit the opt-in (n_bins = 4096 is 256 KiB),
//                     or a device that refused it.  The path is chosen by shape only.
// Bounds: r < n guards every row access; the feature index is clamped to the group's real features before any key is read; probes are
// clamped to [0, B).
#include "kernels.h"
#include "kernels_common.h"
#include "predict_rowwalk.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

constexpr int kLikeThreads = 256;
constexpr int kLikeTiles = 16;   // most row tiles per block (amortises staging the keys); fewer for small batches

template <bool LDS>
__global__ __launch_bounds__(kLikeThreads) void k_bin_like(const float *__restrict__ obs, int n, int F, const uint32_t *__restrict__ thr, int B, int top,
                                                           int tiles_per_block, int vec, uint4 *__restrict__ codes) {
    extern __shared__ __align__(16) uint32_t like_keys[];   // [nf][B]
    const int g = blockIdx.y;
    const int f0 = g * kCodeGroup;
    const int nf = min(kCodeGroup, F - f0);   // real features of this group (>= 1)
    const uint32_t *gkeys = thr + static_cast<size_t>(f0) * B;
    if (LDS) {
        for (int i = threadIdx.x; i < nf * B; i += kLikeThreads) like_keys[i] = gkeys[i];
        __syncthreads();
    }
    const uint32_t *keys = LDS ? like_keys : gkeys;
    for (int tile = 0; tile < tiles_per_block; ++tile) {
        const long long r0 = (static_cast<long long>(blockIdx.x) * tiles_per_block + tile) * kLikeThreads;
        if (r0 >= n) break;
        const long long r = r0 + threadIdx.x;
        if (r >= n) continue;
        const float *src = obs + static_cast<size_t>(r) * F + f0;
        float x[kCodeGroup];
        if (vec) {
#pragma unroll
            for (int q = 0; q < kCodeGroup / 4; ++q) {   // all loads in flight before the first search
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (4 * q < nf) v = *reinterpret_cast<const float4 *>(src + 4 * q);
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int fl = 0; fl < kCodeGroup; ++fl) x[fl] = fl < nf ? src[fl] : 0.f;
        }
        uint32_t w[kCodeGroup / 2];
#pragma unroll
        for (int fl0 = 0; fl0 < kCodeGroup; fl0 += 8) {   // 8 independent searches in flight
            uint32_t key[8], cnt[8];
            int off[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                key[q] = float_to_key(x[fl0 + q]);
                cnt[q] = 0;
                off[q] = min(fl0 + q, nf - 1) * B;
            }
            for (int step = top; step > 0; step >>= 1) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const uint32_t probe = cnt[q] + static_cast<uint32_t>(step);
                    const uint32_t t = keys[off[q] + static_cast<int>(min(probe, static_cast<uint32_t>(B))) - 1];
                    cnt[q] = (probe <= static_cast<uint32_t>(B) && t < key[q]) ? probe : cnt[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const uint32_t lo = fl0 + q < nf ? cnt[q] : 0u, hi = fl0 + q + 1 < nf ? cnt[q + 1] : 0u;
                w[(fl0 + q) / 2] = lo | (hi << 16);
            }
        }
        uint4 *dst = codes + ((static_cast<size_t>(g) * n + static_cast<size_t>(r)) << 1);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}

}  // namespace

void bin_like(const float *obs, int n, int F, const uint32_t *thr_keys, int B, uint16_t *codes, hipStream_t s) {
    if (n <= 0 || F <= 0 || B <= 0) return;
    int top = 1;
    while (2 * top <= B) top <<= 1;
    // enough blocks to fill the chip first, then up to kLikeTiles tiles per block to amortise the staging (bin_cols' rule)
    const int groups = (F + kCodeGroup - 1) / kCodeGroup;
    const long long tiles = (static_cast<long long>(n) + kLikeThreads - 1) / kLikeThreads;
    const int tpb = static_cast<int>(std::min<long long>(kLikeTiles, std::max<long long>(1, tiles * groups / 1024)));
    const dim3 grid(static_cast<unsigned>((tiles + tpb - 1) / tpb), static_cast<unsigned>(groups));
    const int vec = (F % 4 == 0) && (reinterpret_cast<uintptr_t>(obs) & 15) == 0;
    uint4 *out = reinterpret_cast<uint4 *>(codes);
    const size_t lds = static_cast<size_t>(kCodeGroup) * B * sizeof(uint32_t);
    static StreamLdsOptIn optin;
    if (lds <= kStreamLdsBudget && optin.ok(k_bin_like<true>, lds)) {
        hipLaunchKernelGGL(k_bin_like<true>, grid, dim3(kLikeThreads), lds, s, obs, n, F, thr_keys, B, top, tpb, vec, out);
        return;
    }
    hipLaunchKernelGGL(k_bin_like<false>, grid, dim3(kLikeThreads), 0, s, obs, n, F, thr_keys, B, top, tpb, vec, out);
}

}  // namespace kern
}  // namespace gbrl
