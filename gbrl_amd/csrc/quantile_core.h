// quantile_core.h -- quantile regression in fit_prepared(objective="quantile") and GBRL.quantile_leaves_prepared: ONE definition of the pinball gradient
// and loss, of the rank a level selects in a leaf, and of the key the selection orders by, compiled by the host (Engine::objective_gradient_host,
// Engine::leaf_quantile_host, Engine::quantile_rank) and by the device (leaf_quantile.hip, the tails of predict_loss.h).  As in objective_core.h and
// newton_core.h every float32 operation is written out, contraction is off and nothing comes from libm.
//
//   levels       alpha float32 [D], one per output, every entry finite and strictly inside (0, 1) (quantile_bad_level).
//   "quantile"   D >= 1, targets float32 [n, D];  x = fl32(p - y): the bits of the rmse gradient;  g = x > 0 ? fl32(1 - a_d) : (x < 0 ? -a_d : 0).
//                Row loss in float64 from the float32 inputs: u = (double)y - (double)p, sum_d (u >= 0 ? a_d * u : (a_d - 1) * u), d ascending, every
//                product and every sum rounded on its own.  g is dL/dp, as everywhere.
//   rank         a leaf of m >= 1 rows: k = clamp(ceil(a_d * m), 1, m) with the product taken EXACTLY: a_d = M * 2^-s, M < 2^24, m < 2^31, so M * m
//                fits 64 bits and the ceiling is an integer shift; a shift that leaves the word (a tiny a_d) gives k = 1.  No double product: it can
//                round across an integer.
//   key          x with -0 canonicalised to +0 through metric_core.h's order-preserving map (quantile_key; quantile_key_value is its inverse).  A
//                p, y or x that is not finite sets kQuantileBadPred / kQuantileBadTarget / kQuantileBadResidual in the kernels' flag word.
//   leaf value   v[leaf][d] = the k-th LARGEST x among the rows of the leaf: an element of the data, bit for bit, no arithmetic on it.  Predictions
//                move by -rate * v, and -v is the k-th smallest residual y - p: NumPy's quantile(method="inverted_cdf"), a minimiser of the leaf's
//                pinball sum.  A leaf without rows or of depth 0 keeps the value the step gave it (newton_core.h's rule).
//   bias         of a fresh model: the same rule on one leaf of every row at p = 0: bias_d = the k-th smallest y_d, k from n.
#pragma once

#include "metric_core.h"
#include "newton_core.h"

namespace gbrl {
namespace kern {

constexpr int kObjQuantile = 3;    // GBRL_HIP_OBJ_QUANTILE (include/gbrl_hip.h), beside objective_core.h's three
constexpr int kLeafQuantile = 2;   // GBRL_HIP_LEAF_QUANTILE, beside newton_core.h's two
constexpr int kQuantileBadTarget = kNewtonBadTarget, kQuantileBadPred = kNewtonBadPred, kQuantileBadResidual = 4;   // bits of the kernels' flag word

// not a finite number strictly inside (0, 1) (a NaN counts)
GBRL_OBJ_HD inline bool quantile_bad_level(float a) { return !(a > 0.0f && a < 1.0f); }
GBRL_OBJ_HD inline bool quantile_not_finite(float x) { return newton_bad_pred(x); }

// x = fl32(p - y)
GBRL_OBJ_HD inline float quantile_residual(float p, float y) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(p, y);
#else
    return p - y;
#endif
}

// dL/dp of one output from x = fl32(p - y) (a NaN gives 0)
GBRL_OBJ_HD inline float quantile_grad_of(float x, float a) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    const float up = __fsub_rn(1.0f, a);
#else
    const float up = 1.0f - a;
#endif
    return x > 0.0f ? up : (x < 0.0f ? -a : 0.0f);
}
GBRL_OBJ_HD inline float obj_quantile_grad(float p, float y, float a) { return quantile_grad_of(quantile_residual(p, y), a); }

// one output's pinball loss in float64 from the float32 inputs (u is exact or rounded once; one rounded product)
GBRL_OBJ_HD inline double quantile_loss_term(float p, float y, float a) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    const double u = __dsub_rn(static_cast<double>(y), static_cast<double>(p));
    return u >= 0.0 ? __dmul_rn(static_cast<double>(a), u) : __dmul_rn(__dsub_rn(static_cast<double>(a), 1.0), u);
#else
    const double u = static_cast<double>(y) - static_cast<double>(p);
    return u >= 0.0 ? static_cast<double>(a) * u : (static_cast<double>(a) - 1.0) * u;
#endif
}
GBRL_OBJ_HD inline double quantile_loss_add(double acc, double term) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(acc, term);
#else
    return acc + term;
#endif
}

// k = clamp(ceil(a * m), 1, m), the product exact.  a is a good level (the caller has checked); m <= 0 gives 0.
GBRL_OBJ_HD inline long long quantile_rank(long long m, float a) {
    if (m <= 0) return 0;
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(a);
#else
    std::memcpy(&u, &a, sizeof(u));
#endif
    const int e = static_cast<int>((u >> 23) & 0xffu);
    const uint64_t M = e == 0 ? static_cast<uint64_t>(u & 0x7fffffu) : static_cast<uint64_t>((u & 0x7fffffu) | 0x800000u);   // a = M * 2^-s
    const int s = e == 0 ? 149 : 150 - e;                                                                                      // a < 1: s >= 24
    const uint64_t rows = static_cast<uint64_t>(m) > 0x7fffffffull ? 0x7fffffffull : static_cast<uint64_t>(m);                 // (the product fits: M * rows < 2^55)
    const uint64_t P = M * rows;
    long long k = s >= 64 ? 1ll : static_cast<long long>((P + ((1ull << s) - 1ull)) >> s);
    if (k < 1) k = 1;
    return k > m ? m : k;
}

// the order-preserving key of a residual (both zeros are +0) and the float a key came from
GBRL_OBJ_HD inline uint32_t quantile_key(float x) { return metric_key(x); }
GBRL_OBJ_HD inline float quantile_key_value(uint32_t key) { return obj_bits_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu)); }

}  // namespace kern
}  // namespace gbrl
