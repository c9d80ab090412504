// predict_loss.h -- the MultiRMSE row sum and its wave reduction, shared by every kernel that writes loss partials (predict_staged.hip:
// k_staged, k_staged_general, k_loss_of_predictions; predict_continue_codes.hip: the loss tail).  One float64 partial per 64 consecutive rows,
// reduced by a fixed butterfly: whichever kernel wrote part[], k_staged_finish sums the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {
namespace {

constexpr int kStagedRows = kStreamRows;   // rows per wave = rows per loss partial, in every kernel

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

}  // namespace
}  // namespace kern
}  // namespace gbrl
