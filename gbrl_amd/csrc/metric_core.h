// metric_core.h -- the validation metrics of classifiers (fit_prepared(eval_metric=), GBRL.eval_metric): ONE definition of what the host rule
// (Engine::eval_metric_host) and the device kernels (metric.hip) both count, and of the value built from the counts.  Both metrics are
// integers before they are numbers: the host, a brute force and the device agree exactly or not at all, and every floating-point step is taken
// on the host, from the integers, by metric_value below -- the same bits wherever the integers came from.
//
//   "error", softmax     row r is wrong iff argmax_c p[r][c] != label[r]; the arg-max is the LOWEST index among equal maxima, compared as floats
//                        (a NaN is never above the running maximum).  E = wrong rows; value = (double)E / n.  counts [1] = E.
//   "error", logistic    cell (r, d) is wrong iff (p[r][d] > 0) != (y[r][d] > 0.5): a score of exactly 0 (or NaN) predicts the negative class.
//                        E_d = wrong cells of column d; value = (double)(sum_d E_d) / (n D).  counts [D] = E_d.
//   "auc", logistic      per column d: positives are the rows with y[r][d] > 0.5, P_d of them, the other N_d = n - P_d are negatives.  Scores
//                        compare through metric_key: -0.0 first becomes +0.0, then u = bits(p), key = u ^ (u >> 31 ? 0xffffffff : 0x80000000)
//                        -- unsigned order of the keys is float order of the scores, -inf lowest, +inf highest.  A NaN has a key like any
//                        other bit pattern (above +inf with the sign clear, below -inf with it set): defined, and meaningless.
//                        2U_d = sum over positives i of (#{negatives j : key_j < key_i} + #{negatives j : key_j <= key_i}), a uint64: twice the
//                        Mann-Whitney U with ties counted half.  AUC_d = (double)(2U_d) / (2.0 * (double)P_d * (double)N_d);
//                        value = (sum_d AUC_d, d ascending, in double) / D.  counts [D][3] = (2U_d, P_d, N_d).
//                        A column with P_d == 0 or N_d == 0 has no AUC: refused.
// Multi-class AUC and metrics for rmse are not defined here.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_METRIC_HD __host__ __device__
#else
#define GBRL_METRIC_HD
#endif

namespace gbrl {
namespace kern {

constexpr int kMetricNone = 0, kMetricError = 1, kMetricAuc = 2;   // GBRL_HIP_METRIC_* (include/gbrl_hip.h)

GBRL_METRIC_HD inline uint32_t metric_key(float p) {
    if (p == 0.0f) p = 0.0f;   // -0.0 == 0.0f: both zeros leave as +0.0
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(p);
#else
    std::memcpy(&u, &p, sizeof(u));
#endif
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

GBRL_METRIC_HD inline bool metric_positive(float y) { return y > 0.5f; }
GBRL_METRIC_HD inline bool metric_logistic_wrong(float p, float y) { return (p > 0.0f) != metric_positive(y); }

// the lowest index among the maxima of p[0 .. D)
template <typename Row>
GBRL_METRIC_HD inline int metric_argmax(const Row &p, int D) {
    int best = 0;
    float m = p[0];
    for (int c = 1; c < D; ++c) {
        const float v = p[c];
        if (v > m) { m = v; best = c; }
    }
    return best;
}

// integers per column in `counts`, and columns: error / softmax 1 x 1, error / logistic D x 1, auc D x 3
inline int metric_count_columns(int objective_is_softmax, int D) { return objective_is_softmax ? 1 : D; }
inline int metric_count_width(int metric) { return metric == kMetricAuc ? 3 : 1; }

inline double metric_auc_column(uint64_t u2, uint64_t P, uint64_t N) {
    return static_cast<double>(u2) / (2.0 * static_cast<double>(P) * static_cast<double>(N));
}

// the value from the integers (the one place a metric becomes a floating-point number); cells = n for softmax, n * D for logistic
inline double metric_value(int metric, const uint64_t *counts, int columns, uint64_t cells) {
    if (metric == kMetricAuc) {
        double sum = 0.0;
        for (int d = 0; d < columns; ++d) sum += metric_auc_column(counts[3 * d], counts[3 * d + 1], counts[3 * d + 2]);
        return sum / static_cast<double>(columns);
    }
    uint64_t wrong = 0;
    for (int d = 0; d < columns; ++d) wrong += counts[d];
    return static_cast<double>(wrong) / static_cast<double>(cells);
}

}  // namespace kern
}  // namespace gbrl
