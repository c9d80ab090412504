// predict_loss.h -- the MultiRMSE row sum, the row losses of the classification objectives and their wave reduction, shared by every kernel that writes loss partials (predict_staged.hip:
// k_staged, k_staged_general, k_loss_of_predictions; predict_continue_codes.hip: the loss tail).  One float64 partial per 64 consecutive rows,
// reduced by a fixed butterfly: whichever kernel wrote part[], k_staged_finish sums the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "objective_core.h"
#include "quantile_core.h"
#include "predict_rowwalk.h"

namespace gbrl {
namespace kern {
namespace {

constexpr int kStagedRows = kStreamRows;   // rows per wave = rows per loss partial, in every kernel

// sum of the wave's 64 values in a fixed order (leaf_accum.h's xor butterfly, offsets 32 down to 1: every lane ends with the same bits); whole waves only
__device__ __forceinline__ double staged_wave_sum(double v) { return wave_sum(v); }

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

// The row losses of the classification objectives (objective_core.h has the definitions), float64 from the float32 scores, j ascending.
// logistic: sum_j [max(p, 0) - y p + log1p(exp(-|p|))], y float32 [D] read four at a time (no second register row: at DMAX = 128 there is no room).
__device__ __forceinline__ double logistic_loss_term(float p, float y) {
    const double pj = static_cast<double>(p);
    return fma(-static_cast<double>(y), pj, pj > 0.0 ? pj : 0.0) + log1p(exp(-fabs(pj)));   // (y p is exact: two float32 factors)
}
// four targets of a row from entry 4 q on (zeros behind D)
__device__ __forceinline__ float4 objective_load4(const float *y_row, int q, int D, bool vec4) {
    if (vec4) return reinterpret_cast<const float4 *>(y_row)[q];
    float4 y;
    y.x = 4 * q < D ? y_row[4 * q] : 0.0f;
    y.y = 4 * q + 1 < D ? y_row[4 * q + 1] : 0.0f;
    y.z = 4 * q + 2 < D ? y_row[4 * q + 2] : 0.0f;
    y.w = 4 * q + 3 < D ? y_row[4 * q + 3] : 0.0f;
    return y;
}
template <int DMAX>
__device__ __forceinline__ double logistic_row_loss(const float (&p)[DMAX], const float *y_row, int D, bool vec4) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < DMAX / 4; ++q)
        if (4 * q < D) {
            const float4 y = objective_load4(y_row, q, D, vec4);
            acc += logistic_loss_term(p[4 * q], y.x);
            if (4 * q + 1 < D) acc += logistic_loss_term(p[4 * q + 1], y.y);
            if (4 * q + 2 < D) acc += logistic_loss_term(p[4 * q + 2], y.z);
            if (4 * q + 3 < D) acc += logistic_loss_term(p[4 * q + 3], y.w);
        }
    return acc;
}
// softmax: log(sum_j exp((double)p_j - m)) + m - p_label, m = max_j p_j.
template <int DMAX>
__device__ __forceinline__ double softmax_row_loss(const float (&p)[DMAX], int label, int D) {
    float m = p[0], py = p[0];
#pragma unroll
    for (int j = 1; j < DMAX; ++j)
        if (j < D) {
            m = p[j] > m ? p[j] : m;
            py = j == label ? p[j] : py;
        }
    const double md = static_cast<double>(m);
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < DMAX; ++j)
        if (j < D) sum += exp(static_cast<double>(p[j]) - md);
    return log(sum) + md - static_cast<double>(py);
}

// The gradient row of an objective from the scores p and the row's targets, stored to g_row.  y_row: float32 [D] of the row (rmse, logistic: read
// four at a time) or its int32 label (softmax: one entry, the row's probabilities in a second register row).  WEIGHTED: every entry is
// obj_weighted(w, g), w the row's weight, one float32 multiply behind the rule; without it w is not read and the code is what it was.
// kObjQuantile (quantile_core.h; never WEIGHTED): alpha is the device table of the D levels, read only by that instantiation.
template <int OBJ, int DMAX, bool WEIGHTED = false>
__device__ __forceinline__ void objective_grad_store(const float (&p)[DMAX], const float *y_row, int D, bool vec_y, bool vec_g, float *g_row, float w = 1.0f,
                                                     const float *alpha = nullptr) {
    if constexpr (OBJ == kObjSoftmax) {
        float g[DMAX];
#pragma unroll
        for (int d = 0; d < DMAX; ++d) g[d] = p[d];
        obj_softmax_grad_regs<DMAX>(g, D, *reinterpret_cast<const int32_t *>(y_row));
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int d = 0; d < DMAX; ++d) g[d] = obj_weighted(w, g[d]);
        }
        stream_store_row<DMAX>(g_row, D, vec_g, g);
    } else {
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q)
            if (4 * q < D) {
                const float4 y = objective_load4(y_row, q, D, vec_y);
                float4 g;
                if constexpr (OBJ == kObjLogistic) {
                    g.x = obj_logistic_grad(p[4 * q], y.x);
                    g.y = 4 * q + 1 < D ? obj_logistic_grad(p[4 * q + 1], y.y) : 0.0f;
                    g.z = 4 * q + 2 < D ? obj_logistic_grad(p[4 * q + 2], y.z) : 0.0f;
                    g.w = 4 * q + 3 < D ? obj_logistic_grad(p[4 * q + 3], y.w) : 0.0f;
                } else if constexpr (OBJ == kObjQuantile) {
                    g.x = obj_quantile_grad(p[4 * q], y.x, alpha[4 * q]);
                    g.y = 4 * q + 1 < D ? obj_quantile_grad(p[4 * q + 1], y.y, alpha[4 * q + 1]) : 0.0f;
                    g.z = 4 * q + 2 < D ? obj_quantile_grad(p[4 * q + 2], y.z, alpha[4 * q + 2]) : 0.0f;
                    g.w = 4 * q + 3 < D ? obj_quantile_grad(p[4 * q + 3], y.w, alpha[4 * q + 3]) : 0.0f;
                } else {
                    g.x = __fsub_rn(p[4 * q], y.x); g.y = __fsub_rn(p[4 * q + 1], y.y); g.z = __fsub_rn(p[4 * q + 2], y.z); g.w = __fsub_rn(p[4 * q + 3], y.w);
                }
                if constexpr (WEIGHTED) {
                    g.x = obj_weighted(w, g.x); g.y = obj_weighted(w, g.y); g.z = obj_weighted(w, g.z); g.w = obj_weighted(w, g.w);
                }
                if (vec_g) {
                    reinterpret_cast<float4 *>(g_row)[q] = g;
                } else {
                    g_row[4 * q] = g.x;
                    if (4 * q + 1 < D) g_row[4 * q + 1] = g.y;
                    if (4 * q + 2 < D) g_row[4 * q + 2] = g.z;
                    if (4 * q + 3 < D) g_row[4 * q + 3] = g.w;
                }
            }
    }
}

// ... and its loss.  p_row: the row as the lane itself has stored it (or read it).  The widest family (DMAX = 128) sums the logistic loss from
// there in a rolled loop -- the same terms in the same order: 128 unrolled float64 exp / log1p beside p[128] do not fit the register file.
template <int OBJ, int DMAX>
__device__ __forceinline__ double objective_loss_regs(const float (&p)[DMAX], const float *p_row, const float *y_row, int D, bool vec4,
                                                      const float *alpha = nullptr) {
    if constexpr (OBJ == kObjSoftmax) {
        return softmax_row_loss<DMAX>(p, *reinterpret_cast<const int32_t *>(y_row), D);
    } else if constexpr (OBJ == kObjQuantile && DMAX > 64) {   // the pinball terms, j ascending (quantile_core.h: every step rounded on its own)
        double acc = 0.0;
#pragma unroll 1
        for (int j = 0; j < D; ++j) acc = quantile_loss_add(acc, quantile_loss_term(p_row[j], y_row[j], alpha[j]));
        return acc;
    } else if constexpr (OBJ == kObjQuantile) {   // the same terms in the same order from the registers, the targets read four at a time
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q)
            if (4 * q < D) {
                const float4 y = objective_load4(y_row, q, D, vec4);
                const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * q + k < D) acc = quantile_loss_add(acc, quantile_loss_term(p[4 * q + k], yy[k], alpha[4 * q + k]));
            }
        return acc;
    } else if constexpr (OBJ == kObjLogistic && DMAX > 64) {
        double acc = 0.0;
#pragma unroll 1
        for (int j = 0; j < D; ++j) acc += logistic_loss_term(p_row[j], y_row[j]);
        return acc;
    } else if constexpr (OBJ == kObjLogistic) {
        return logistic_row_loss<DMAX>(p, y_row, D, vec4);
    } else {
        double acc = 0.0;   // staged_row_loss's sum, the targets read four at a time
#pragma unroll
        for (int q = 0; q < DMAX / 4; ++q)
            if (4 * q < D) {
                const float4 y = objective_load4(y_row, q, D, vec4);
                const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * q + k < D) {
                        const double g = static_cast<double>(__fsub_rn(p[4 * q + k], yy[k]));
                        acc = fma(g, g, acc);
                    }
            }
        return acc;
    }
}

// the targets of row `row`: D floats, or one label
template <int OBJ>
__device__ __forceinline__ const float *objective_target_row(const float *targets, size_t row, int D) {
    return OBJ == kObjSoftmax ? targets + row : targets + row * D;
}

// f(std::integral_constant<int, OBJ>) for the objective (the caller has refused every other value)
template <typename Fn>
auto with_objective(int objective, Fn &&f) {
    if (objective == kObjLogistic) return f(std::integral_constant<int, kObjLogistic>{});
    if (objective == kObjSoftmax) return f(std::integral_constant<int, kObjSoftmax>{});
    if (objective == kObjQuantile) return f(std::integral_constant<int, kObjQuantile>{});
    return f(std::integral_constant<int, kObjRmse>{});
}

}  // namespace
}  // namespace kern
}  // namespace gbrl
