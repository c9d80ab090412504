// newton_core.h -- the second-order leaf step of fit_prepared(leaf_update="newton") and GBRL.newton_leaves_prepared: ONE definition of the hessian, of the
// quantum the sums are taken in and of the leaf value, compiled by the host (Engine::objective_hessian_host, Engine::newton_values_host) and by the
// device (newton.hip).  The gradient is objective_core.h's, unchanged: the g summed here is bit for bit the g the tree was grown on.  As there,
// every float32 operation is written out, contraction is off and every division is correctly rounded.
//
//   "logistic"   e = obj_exp_f32(-|p|), den = 1 + e as in obj_logistic_grad;  h = fl32(fl32(1 / den) * fl32(e / den)): both factors are correctly
//                rounded quotients, so no 1 - s cancels.  h is symmetric in p bit for bit (only |p| enters), h(0) = 0.25 exactly, h in [0, 0.25].
//   "softmax"    q_c exactly as obj_softmax_grad_row computes it;  h_c = fl32(q_c * fl32(1 - q_c)): the diagonal of the hessian only, as
//                scikit-learn, XGBoost and LightGBM take it.
//   sums         bits = newton_sum_bits(m) = min(40, 62 - bit_length(m)) for m summed rows;  the quantum q(x) = llrint((double)x * 2^bits), the same
//                bits for g and h.  |g| <= 1 and h <= 0.25, so |sum| <= m * 2^bits < 2^62.  Per leaf: Sg[D], Sh[D], cnt -- int64, exact, order-free.
//   row weights  g_w = fl32(w * g), h_w = fl32(w * h) (objective_core.h: obj_weighted) are what is quantised: Sg += q(g_w), Sh += q(h_w), cnt counts rows
//                as before.  The quantum makes room for the weight: bits = newton_sum_bits(m, weight_max) = min(40, 62 - bit_length(m) - e), e the smallest
//                integer >= 0 with weight_max <= 2^e, so |g_w| <= 2^e and |sum| < 2^62 still; e = 0 (weight_max <= 1) is the rule above.  weight_max is an
//                INPUT of the rule (fit_prepared: the maximum over the training weights of the whole data set), never something a kernel discovers.
//   value        G = Sg / 2^bits, H = Sh / 2^bits, den = H + leaf_l2 in double;  v = (float)(G / den).  A leaf keeps the value the step gave it when
//                cnt == 0, when its depth is 0 (refit_leaves' rule for a leaf no row reaches) or when !(den > 0).  Predictions move by -rate * v.
#pragma once

#include "objective_core.h"

namespace gbrl {
namespace kern {

constexpr int kLeafGradient = 0, kLeafNewton = 1;   // GBRL_HIP_LEAF_* (include/gbrl_hip.h)
constexpr int kNewtonBadTarget = 1, kNewtonBadPred = 2;   // bits of the kernels' flag word
// not an objective of the C ABI: the sums' kernels read g and h per row from two float32 buffers (in the places of pred and targets) that another
// kernel wrote -- a ranking gradient is a sum over the row's query (rank_core.h) and cannot be computed from (p, y) inline
constexpr int kObjGiven = -1;

// logistic: gradient and hessian of one output from one exp (g has obj_logistic_grad's bits)
GBRL_OBJ_HD inline void obj_logistic_grad_hess(float p, float y, float &g, float &h) {
#pragma clang fp contract(off)
    const float e = obj_exp_f32(p >= 0.0f ? -p : p);
    const float den = 1.0f + e;
    const float a = obj_div(1.0f, den), b = obj_div(e, den);
    g = (p >= 0.0f ? a : b) - y;
    h = a * b;
}
GBRL_OBJ_HD inline float obj_logistic_hess(float p) {
    float g, h;
    obj_logistic_grad_hess(p, 0.0f, g, h);
    return h;
}

// softmax: one output's gradient and hessian from its probability q
GBRL_OBJ_HD inline float obj_softmax_grad_of(float q, bool is_label) {
#pragma clang fp contract(off)
    return q - (is_label ? 1.0f : 0.0f);
}
GBRL_OBJ_HD inline float obj_softmax_hess_of(float q) {
#pragma clang fp contract(off)
    const float r = 1.0f - q;
    return q * r;
}

// softmax: p[0 .. D) becomes the gradient row in place (obj_softmax_grad_row's bits), h[0 .. D) the hessian row
template <typename Row, typename HRow>
GBRL_OBJ_HD inline void obj_softmax_grad_hess_row(Row &p, HRow &h, int D, int label) {
#pragma clang fp contract(off)
    float m = p[0];
    for (int c = 1; c < D; ++c) m = p[c] > m ? p[c] : m;
    float S = 0.0f;
    for (int c = 0; c < D; ++c) {
        const float e = obj_exp_f32(p[c] == m ? 0.0f : p[c] - m);
        p[c] = e;
        S = S + e;
    }
    for (int c = 0; c < D; ++c) {
        const float q = obj_div(p[c], S);
        h[c] = obj_softmax_hess_of(q);
        p[c] = obj_softmax_grad_of(q, c == label);
    }
}

// the same on register rows of DMAX entries, next to obj_softmax_grad_regs: g and h from one pass over the row
template <int DMAX>
GBRL_OBJ_HD inline void obj_softmax_grad_hess_regs(float (&p)[DMAX], float (&h)[DMAX], int D, int label) {
#pragma clang fp contract(off)
    float m = p[0];
#pragma unroll
    for (int c = 1; c < DMAX; ++c)
        if (c < D) m = p[c] > m ? p[c] : m;
    float S = 0.0f;
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < D) {
            const float e = obj_exp_f32(p[c] == m ? 0.0f : p[c] - m);
            p[c] = e;
            S = S + e;
        }
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
        if (c < D) {
            const float q = obj_div(p[c], S);
            h[c] = obj_softmax_hess_of(q);
            p[c] = obj_softmax_grad_of(q, c == label);
        } else {
            h[c] = 0.0f;
        }
}

// what the kernels refuse: a logistic target outside [0, 1] (a NaN counts), a prediction that is not finite
GBRL_OBJ_HD inline bool newton_bad_target(float y) { return !(y >= 0.0f && y <= 1.0f); }
GBRL_OBJ_HD inline bool newton_bad_pred(float p) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(p);
#else
    std::memcpy(&u, &p, sizeof(u));
#endif
    return (u & 0x7f800000u) == 0x7f800000u;
}

// bits of the quantum for m summed rows: min(40, 62 - bit_length(m))
GBRL_OBJ_HD inline int newton_sum_bits(long long m) {
    int len = 0;
    for (unsigned long long v = m > 0 ? static_cast<unsigned long long>(m) : 0ull; v != 0; v >>= 1) ++len;
    const int b = 62 - len;
    return b < 40 ? b : 40;
}

// ... with row weights up to weight_max (finite, in [0, kWeightMax]: the caller has checked): e fewer bits, weight_max <= 2^e
GBRL_OBJ_HD inline int newton_weight_exponent(float weight_max) {
    int e = 0;
    for (float cap = 1.0f; cap < weight_max; cap = cap + cap) ++e;   // (exact doublings; at most 16 of them)
    return e;
}
GBRL_OBJ_HD inline int newton_sum_bits(long long m, float weight_max) {
    int len = 0;
    for (unsigned long long v = m > 0 ? static_cast<unsigned long long>(m) : 0ull; v != 0; v >>= 1) ++len;
    const int b = 62 - len - newton_weight_exponent(weight_max);
    return b < 40 ? b : 40;
}

// q(x) = llrint((double)x * scale), scale = 2^bits (the product is exact: a power of two)
GBRL_OBJ_HD inline long long newton_quantise(float x, double scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(__dmul_rn(static_cast<double>(x), scale));
#else
    return __builtin_llrint(static_cast<double>(x) * scale);
#endif
}

// the leaf value from its integers (host only: double division)
inline float newton_leaf_value(long long Sg, long long Sh, long long cnt, int depth, double scale, double leaf_l2, float old) {
    if (cnt <= 0 || depth <= 0) return old;
    const double G = static_cast<double>(Sg) / scale, H = static_cast<double>(Sh) / scale;
    const double den = H + leaf_l2;
    if (!(den > 0.0)) return old;
    return static_cast<float>(G / den);
}

}  // namespace kern
}  // namespace gbrl
