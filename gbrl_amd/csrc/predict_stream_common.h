// predict_stream_common.h -- what the lane-per-row streaming kernels share (k_continue of predict_continue.hip, k_staged of predict_staged.hip):
// one wave per block, the block's 64 rows in LDS at stride F | 1, the outputs of a row in registers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace gbrl {
namespace kern {
namespace {

constexpr int kStreamRows = 64;   // rows per block = one wave

// D floats of one row into registers: 16-byte accesses when the row is a whole number of them and its address allows it
template <int DMAX>
__device__ __forceinline__ void stream_load_row(const float *src, int D, bool vec4, float (&v)[DMAX]) {
    if (vec4) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q) {
            const float4 w = 4 * q < D ? s4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < DMAX; ++j) v[j] = j < D ? src[j] : 0.0f;
    }
}

// coalesced staging of a block's `rows` rows from r0 on (contiguous in the row-major matrix) into tile[kStreamRows][F | 1], 16 x 16 bytes in flight
// per lane; the caller synchronises the block afterwards
__device__ __forceinline__ void stream_stage_tile(float *tile, const float *__restrict__ obs, int F, int r0, int rows, int lane) {
    const int xs = F | 1;
    const float *src = obs + static_cast<size_t>(r0) * F;
    if (F > 0 && (F & 3) == 0 && (reinterpret_cast<uintptr_t>(obs) & 15) == 0) {
        const float4 *src4 = reinterpret_cast<const float4 *>(src);
        const int F4 = F >> 2, tot4 = rows * F4;
        constexpr int UL = 16;
        for (int i0 = lane; i0 < tot4; i0 += kStreamRows * UL) {
            float4 v[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * kStreamRows;
                v[u] = i < tot4 ? src4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * kStreamRows;
                if (i < tot4) {
                    const int r = i / F4, f = (i - r * F4) << 2;
                    float *dst = tile + r * xs + f;
                    dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
                }
            }
        }
    } else {
        const int tot = rows * F;
        for (int i = lane; i < tot; i += kStreamRows) {
            const int r = i / F, f = i - r * F;
            tile[r * xs + f] = src[i];
        }
    }
}

}  // namespace
}  // namespace kern
}  // namespace gbrl
