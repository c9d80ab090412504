// kernels_common.h -- device helpers shared by the kernel translation units (the step_*.hip units, predict.hip, categorical.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace gbrl {
namespace kern {
namespace {

constexpr int kWave = 64;

__device__ __forceinline__ uint32_t float_to_key(float x) {
    // order-preserving map float -> uint32; -0.0 and +0.0 map to the same key (they compare equal as floats)
    uint32_t u = __float_as_uint(x);
    if ((u << 1) == 0) u = 0;
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;   // NaN: below every threshold, like the float comparison `x > t` (false)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

__device__ __forceinline__ int ilog2_floor_dev(double x) { int e; (void)frexp(x, &e); return e - 1; }

// Bits of the int64 fixed point of the leaf sums: 2^lbits scales the raw gradients of a batch of n rows whose largest magnitude is hraw, so
// that n * hraw * 2^lbits < 2^61 and no exact sum can wrap.  40 when hraw is 0 or not finite (the caller rejects the latter).  ONE rule for
// the step (k_stats_finish, small_stats_body) and for kern::refit_leaves, which must store what the step would have stored.
__device__ __forceinline__ int leaf_sum_bits_dev(long long n, float hraw) {
    int lbits = 40;
    if (hraw > 0.f && hraw < INFINITY) lbits = min(60, ilog2_floor_dev(4.0e18 / (static_cast<double>(n) * hraw)) - 1);
    return lbits;
}

inline int grid_for(size_t n, int bs, int cap) {
    size_t b = (n + bs - 1) / bs;
    if (b < 1) b = 1;
    return static_cast<int>(b > static_cast<size_t>(cap) ? cap : b);
}

}  // namespace
}  // namespace kern
}  // namespace gbrl
