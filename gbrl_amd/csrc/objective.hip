// objective.hip -- gfx950 kernels behind GBRL::objective_gradient and the parts of fit_prepared(objective=) that are not the code walk:
//
//   k_objective_rows   the objective's gradient and / or loss of a prediction matrix [n][D]: one lane per row, 256 threads, the row in p[DMAX]
//                      registers (16-byte loads where D % 4 == 0 and the pointers allow it, as stream_load_row decides), then the device functions
//                      of predict_continue_codes.hip's two tails (predict_loss.h: objective_grad_store, objective_loss_regs) -- the same bits as the
//                      fused tails.  Loss: one float64 partial per wave of 64 rows through staged_wave_sum, finished by k_staged_finish.
//                      WEIGHTED (a template flag) with weights float32 [n]: the row's weight is loaded with the row; the gradient is fl32(w * g) and
//                      the row loss (double)w * L in front of the butterfly.  Without the flag the pointer is never read -- except by the
//                      kObjQuantile instantiations (quantile_core.h; they take no weights), whose level table alpha [D] arrives in that argument: hence its name, row_operand.
//   k_weight_stats     a weight vector in one pass: the first row whose weight is refused, the largest weight, and the sum of the weights as
//                      float64 partials per wave in the loss partials' order (finished by k_staged_finish: fixed order, the same bits every call).
//   k_label_counts     class counts of an int32 label vector by integer atomics (an LDS histogram per block, then one global add per class), and
//                      the smallest row whose label is outside [0, D): fit_prepared's softmax bias and the range check, one pass, D + 1 ints back.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_loss.h"

namespace gbrl {
namespace kern {

namespace {

template <int DMAX, int OBJ, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_objective_rows(const float *__restrict__ pred, const float *__restrict__ targets, int n, int D, float *__restrict__ grad_out,
                                                        double *__restrict__ loss_part, int loss_nb, int vec_pred, int vec_tar, int vec_grad,
                                                        const float *__restrict__ row_operand) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < n;
    if (!live && loss_part == nullptr) return;   // (with the loss whole waves stay for the butterfly)
    float p[DMAX];
    float w = 1.0f;
    if constexpr (WEIGHTED) w = live ? row_operand[j] : 0.0f;
    if (live) {
        stream_load_row<DMAX>(pred + static_cast<size_t>(j) * D, D, vec_pred != 0, p);
        if (grad_out != nullptr)
            objective_grad_store<OBJ, DMAX, WEIGHTED>(p, objective_target_row<OBJ>(targets, j, D), D, vec_tar != 0, vec_grad != 0,
                                                      grad_out + static_cast<size_t>(j) * D, w, row_operand);
    }
    if (loss_part != nullptr) {
        double acc = 0.0;
        if (live) acc = objective_loss_regs<OBJ, DMAX>(p, pred + static_cast<size_t>(j) * D, objective_target_row<OBJ>(targets, j, D), D, vec_tar != 0, row_operand);
        if constexpr (WEIGHTED) acc = obj_weighted_loss(w, acc);
        acc = staged_wave_sum(acc);
        const int wave = j / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
        if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < loss_nb) loss_part[wave] = acc;
    }
}

__global__ __launch_bounds__(256) void k_weight_stats(const float *__restrict__ weights, int n, int32_t *__restrict__ stat, double *__restrict__ part, int nb) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;   // (whole waves stay for the butterfly)
    const float w = j < n ? weights[j] : 0.0f;
    const bool bad = obj_weight_bad(w);
    if (bad) atomicMin(&stat[0], j);
    else if (w > 0.0f) atomicMax(&stat[1], static_cast<int32_t>(__float_as_uint(w)));   // (in [0, 65536]: the bits are a non-negative int32 in the floats' order)
    const double sum = staged_wave_sum(bad ? 0.0 : static_cast<double>(w));
    const int wave = j / kStagedRows;
    if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < nb) part[wave] = sum;
}

constexpr int kLabelClasses = 128;   // output_dim <= 128 wherever labels are taken

__global__ __launch_bounds__(256) void k_label_counts(const int32_t *__restrict__ labels, int n, int D, int32_t *__restrict__ counts) {
    __shared__ int32_t hist[kLabelClasses];
    __shared__ int32_t bad;
    for (int c = threadIdx.x; c < kLabelClasses; c += blockDim.x) hist[c] = 0;
    if (threadIdx.x == 0) bad = 0x7fffffff;
    __syncthreads();
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < static_cast<size_t>(n); i += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const int32_t y = labels[i];
        if (y >= 0 && y < D) atomicAdd(&hist[y], 1);
        else atomicMin(&bad, static_cast<int32_t>(i));
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += blockDim.x)
        if (hist[c] != 0) atomicAdd(&counts[c], hist[c]);
    if (threadIdx.x == 0 && bad != 0x7fffffff) atomicMin(&counts[D], bad);
}

}  // namespace

void objective_rows(int objective, const float *pred, const void *targets, int n, int D, float *grad_out, double *loss_part, hipStream_t s, const float *weights,
                    const float *alpha) {
    if (n <= 0 || (grad_out == nullptr && loss_part == nullptr)) return;
    const bool d4 = (D & 3) == 0;
    const int vec_pred = d4 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0;
    const int vec_tar = d4 && (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    const int vec_grad = d4 && (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0;
    auto run = [&](auto obj, auto weighted) {
        with_general_dmax(D, [&](auto dmax) {
            hipLaunchKernelGGL((k_objective_rows<decltype(dmax)::value, decltype(obj)::value, decltype(weighted)::value>), dim3((n + 255) / 256), dim3(256), 0, s,
                               pred, static_cast<const float *>(targets), n, D, grad_out, loss_part, staged_loss_partials(n), vec_pred, vec_tar, vec_grad,
                               decltype(obj)::value == kObjQuantile ? alpha : weights);
        });
    };
    with_objective(objective, [&](auto obj) {
        if constexpr (decltype(obj)::value == kObjQuantile) run(obj, std::false_type{});   // (no weighted form: the caller has refused weights)
        else if (weights != nullptr) run(obj, std::true_type{});
        else run(obj, std::false_type{});
    });
}

void weight_stats(const float *weights, int n, int32_t *stat, double *part, double *sum, hipStream_t s) {
    if (n <= 0) return;
    const int nb = staged_loss_partials(n);
    hipLaunchKernelGGL(k_weight_stats, dim3((n + 255) / 256), dim3(256), 0, s, weights, n, stat, part, nb);
    staged_loss_finish(part, nb, sum, s);
}

void label_counts(const int32_t *labels, int n, int D, int32_t *counts, hipStream_t s) {
    if (n <= 0) return;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(n) + 255) / 256, 1024));
    hipLaunchKernelGGL(k_label_counts, dim3(blocks), dim3(256), 0, s, labels, n, D, counts);
}

}  // namespace kern
}  // namespace gbrl
