// objective_core.h -- the classification objectives of fit_prepared(objective=) and GBRL.objective_gradient: ONE definition of the gradient that
// the host (Engine::objective_gradient_host) and the device (objective.hip, the tails of predict_continue_codes.hip) both call, so that a gradient is
// the same bits wherever it is computed.  Every float32 operation is written out: no libm call, no fast intrinsic, contraction off inside every
// function here (hipcc contracts a * b + c in its device pass and not in its host pass by default), every product-sum an explicit fmaf or a
// separate multiply and add.
//
//   obj_exp(t), t <= 0      k = rint(t * log2(e)) by the 1.5 * 2^23 trick;  r = t - k * ln2 in two parts (fmaf; |r| <= 0.3466);
//                           p = exp(r) = 1 + (r + r^2 * (c2 + c3 r + .. + c7 r^5));  the value p * 2^k, scaled through the exponent bits.  Below
//                           t = -87.34 the value is under 2^-126, where float32 keeps fewer than 24 bits, so obj_exp hands the unrounded value out
//                           as a double: within 2^-22 relative of exp(t) on all of [-104, 0] (measured: DESIGN.md section 5).  t < -104
//                           (exp(t) < 2^-150) returns +0.
//   obj_exp_f32(t)          obj_exp(t) rounded once to float32 (two float32 factors when k < -100; no float64): the e of the rules below.
//   "logistic", D >= 1      targets float32 [n, D];  e = obj_exp_f32(-|p|);  s = p >= 0 ? 1 / (1 + e) : e / (1 + e) (correctly rounded division);
//                           g = fl32(s - y).  Row loss (device only, float64 from the float32 p): sum_d [max(p, 0) - y p + log1p(exp(-|p|))].
//   "softmax", D >= 2       targets int32 [n], labels in [0, D);  m = max_c p_c;  t_c = fl32(p_c - m), and 0 where p_c == m (a score of +inf is the
//                           maximum, not inf - inf);  e_c = obj_exp_f32(t_c);  S = float32 sum of e_c, c ascending;  q_c = e_c / S;
//                           g_c = fl32(q_c - [c == y]).  Row loss (device only, float64): log(sum_c exp((double)p_c - m)) + m - p_y.
//   "rmse"                  g = fl32(p - y): what fit_prepared has always done (predict_loss.h has its loss).
//
// g is dL/dp: trees fit g and predictions move by -lr * value, as with p - y.
//
//   row weights             weights float32 [n], every entry finite and in [0, kWeightMax], W = sum_r (double)w_r > 0 where a loss or a bias is taken.
//                           g_w = fl32(w * g) with g exactly as above: one float32 multiply behind the rule, so w == 1 changes no bit (obj_weighted).
//                           The loss is sum_r (double)w_r * L_r over W in place of sum_r L_r over the row count: L_r the float64 row loss as
//                           before, one float64 multiply per row (obj_weighted_loss) in front of the reduction, whose order is unchanged.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_OBJ_HD __host__ __device__
#else
#define GBRL_OBJ_HD
#endif

namespace gbrl {
namespace kern {

constexpr int kObjRmse = 0, kObjLogistic = 1, kObjSoftmax = 2;   // GBRL_HIP_OBJ_* (include/gbrl_hip.h)

GBRL_OBJ_HD inline float obj_bits_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
#endif
}

// correctly rounded float32 division on either side
GBRL_OBJ_HD inline float obj_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// exp(t) = p * 2^k for t in [-104, 0]: p in [0.70, 1.42] (float32 steps only), k in [-150, 0]
GBRL_OBJ_HD inline float obj_exp_parts(float t, int &k) {
#pragma clang fp contract(off)
    const float z = __builtin_fmaf(t, 0x1.715476p+0f, 12582912.0f);   // t * log2(e) + 1.5 * 2^23: the sum rounds to an integer, ties to even
    const float kf = z - 12582912.0f;                               // exact
    float r = __builtin_fmaf(kf, -0x1.62e4p-1f, t);                 // ln2 high part: 15 significant bits, k * hi is exact
    r = __builtin_fmaf(kf, -0x1.7f7d1cp-20f, r);
    float q = 0x1.a15318p-13f;
    q = __builtin_fmaf(q, r, 0x1.6d44b6p-10f);
    q = __builtin_fmaf(q, r, 0x1.1110c6p-7f);
    q = __builtin_fmaf(q, r, 0x1.5554e8p-5f);
    q = __builtin_fmaf(q, r, 0x1.555556p-3f);
    q = __builtin_fmaf(q, r, 0.5f);
    const float r2 = r * r;
    k = static_cast<int>(kf);
    return 1.0f + __builtin_fmaf(r2, q, r);
}

// obj_exp: the value itself, p * 2^k without a rounding -- a float32 significand under an exponent that float32 does not hold below 2^-126.
// Returned as a double (the scaling is an integer subtraction in its exponent field: exact).  t < -104 gives +0; a NaN stays a NaN.
GBRL_OBJ_HD inline double obj_exp(float t) {
    if (t < -104.0f) return 0.0;
    if (!(t <= 0.0f)) return static_cast<double>(t != t ? t : 1.0f);   // (never passed: a NaN, or t > 0 answered as exp(0))
    int k;
    const double p = static_cast<double>(obj_exp_parts(t, k));
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, p) - (static_cast<uint64_t>(-k) << 52));
}

// obj_exp_f32: obj_exp rounded ONCE to float32, nearest-even, into the subnormals below 2^-126 -- (float)obj_exp(t) bit for bit
// (tests/test_objective_host.py holds it to that), computed without float64: what the gradients use, on the host and in the kernels.
GBRL_OBJ_HD inline float obj_exp_f32(float t) {
#pragma clang fp contract(off)
    if (t < -104.0f) return 0.0f;                                   // (also -inf; a NaN falls through and stays a NaN)
    int k;
    const float p = obj_exp_parts(t, k);
    if (k >= -100) return p * obj_bits_float(static_cast<uint32_t>(127 + k) << 23);   // exact scaling
    return (p * obj_bits_float(static_cast<uint32_t>(227 + k) << 23)) * 0x1p-100f;    // one rounding, into the subnormals
}

// row weights: the largest weight, what is refused (a NaN, a negative, an infinite or a larger entry), the weighted gradient / hessian entry
// fl32(w * x) and the weighted row loss (double)w * L
constexpr float kWeightMax = 65536.0f;
GBRL_OBJ_HD inline bool obj_weight_bad(float w) { return !(w >= 0.0f && w <= kWeightMax); }
GBRL_OBJ_HD inline float obj_weighted(float w, float x) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(w, x);
#else
    return w * x;
#endif
}
GBRL_OBJ_HD inline double obj_weighted_loss(float w, double loss) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(static_cast<double>(w), loss);
#else
    return static_cast<double>(w) * loss;
#endif
}

// logistic: dL/dp of one output
GBRL_OBJ_HD inline float obj_logistic_grad(float p, float y) {
#pragma clang fp contract(off)
    const float e = obj_exp_f32(p >= 0.0f ? -p : p);   // -|p| (a -0.0 goes in as it is: exp gives 1 for either zero)
    const float den = 1.0f + e;
    const float s = p >= 0.0f ? obj_div(1.0f, den) : obj_div(e, den);
    return s - y;
}

// softmax: p[0 .. D) becomes the gradient row in place; label in [0, D) (checked by the caller)
template <typename Row>
GBRL_OBJ_HD inline void obj_softmax_grad_row(Row &p, int D, int label) {
#pragma clang fp contract(off)
    float m = p[0];
    for (int c = 1; c < D; ++c) m = p[c] > m ? p[c] : m;
    float S = 0.0f;
    for (int c = 0; c < D; ++c) {
        const float e = obj_exp_f32(p[c] == m ? 0.0f : p[c] - m);
        p[c] = e;
        S = S + e;
    }
    for (int c = 0; c < D; ++c) p[c] = obj_div(p[c], S) - (c == label ? 1.0f : 0.0f);
}

// the same on a register row of DMAX entries (every loop unrolled: no dynamic index, so the row stays in registers)
template <int DMAX>
GBRL_OBJ_HD inline void obj_softmax_grad_regs(float (&p)[DMAX], int D, int label) {
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
        if (c < D) p[c] = obj_div(p[c], S) - (c == label ? 1.0f : 0.0f);
}

}  // namespace kern
}  // namespace gbrl
