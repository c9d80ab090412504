// refit_common.h -- what refit.hip (the float rows) and refit_codes.hip (a data set's bin codes) share on the device: the magnitude-bits maximum of
// a gradient, the quantum of the gradient leaf sums and the value a leaf gets from its sum.  One definition, so both refits store the same bytes.
#pragma once

#include "kernels_common.h"

namespace gbrl {
namespace kern {
namespace {

// bits of |g| as an unsigned integer: ordered like the magnitudes; NaN is carried as +inf
__device__ __forceinline__ uint32_t refit_abs_bits(float g) {
    const uint32_t u = __float_as_uint(g) & 0x7fffffffu;
    return u > 0x7f800000u ? 0x7f800000u : u;
}
__device__ __forceinline__ double refit_scale(int n, const uint32_t *gmax) {
    return ldexp(1.0, leaf_sum_bits_dev(static_cast<long long>(n), __uint_as_float(*gmax)));
}
__device__ __forceinline__ long long refit_quantise(float g, double scale) { return __double2ll_rn(__dmul_rn(static_cast<double>(g), scale)); }
// maximum over the block, then one atomic per block
__device__ __forceinline__ void refit_block_max(uint32_t m, uint32_t *dst) {
    __shared__ uint32_t sh[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), off, kWave)));
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < static_cast<int>(blockDim.x) / kWave; ++w) m = max(m, sh[w]);
        if (m) atomicMax(dst, m);
    }
}

// decay * old + keep * v, two rounded float64 products and one rounded sum; decay == 0 is v itself
__device__ __forceinline__ float refit_mix(double decay, double keep, float old, double v) {
    return decay == 0.0 ? static_cast<float>(v) : static_cast<float>(__dadd_rn(__dmul_rn(decay, static_cast<double>(old)), __dmul_rn(keep, v)));
}
// the value of a leaf from its gradient sum S (in the quantum of gmax, n rows) and its row count; a leaf without rows and a leaf of depth 0 keep theirs
__device__ __forceinline__ float refit_mean_value(long long S, long long cnt, int depth, float old, int n, const uint32_t *gmax, double decay, double keep) {
    if (!(cnt > 0 && depth > 0)) return old;
    // append_tree's expression: (sum / scale) / count, every operation rounded once (the first is exact: a power of two)
    const double mean = __ddiv_rn(__ddiv_rn(static_cast<double>(S), refit_scale(n, gmax)), static_cast<double>(cnt));
    return refit_mix(decay, keep, old, mean);
}

}  // namespace
}  // namespace kern
}  // namespace gbrl
