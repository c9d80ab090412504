// rank_core.h -- the ranking objectives of GBRL.rank_gradient ("pairwise", "lambdarank"): ONE definition of a row's position inside its query, of the
// discounts and gains, of the ideal DCG, of a pair's weight and of what a pair adds to its two rows, compiled by the host (Engine::rank_gradient_host)
// and by the device (rank.hip).  As in objective_core.h every operation is written out, contraction is off, every float64 product, sum and quotient
// is rounded on its own, and the only transcendental is obj_exp_f32 through the logistic rule (newton_core.h: obj_logistic_grad_hess).
//
//   inputs       s float32 [n] (a model of output_dim 1), labels int32 [n] in [0, kRankMaxLabel], group int32 [Q]: the sizes of consecutive row runs,
//                each in [1, kRankMaxQuery], summing to n.
//   pos(i)       #{j in the query of i : s_j > s_i, or s_j == s_i and j < i}: 0-based, the float compare (-0 == +0).  A score that is not finite is
//                refused (the kernels set kRankBadPred in their flag word).
//   disc[t]      1 / log2(t + 2), t in [0, kRankMaxQuery), float64: a table built once on the host (rank_discount_table) and an INPUT of the rule --
//                host and kernels read the same table.  With ndcg_at = K > 0, disc[t] counts as 0 for t >= K (rank_disc); K == 0: no truncation.
//   gain(l)      2^l - 1, exact.
//   maxDCG_q     the query's labels in descending order l_(0) >= l_(1) >= ..: sum_t gain(l_(t)) * disc[t], t ascending;  inv_q = maxDCG_q > 0 ?
//                1 / maxDCG_q : 0.  Labels do not change: once per call.
//   pairs        rows i, j of one query with l_i > l_j:  delta = fl32(s_i - s_j), rho = sig(-delta), eta = fl32(sig(delta) * sig(-delta)) -- the
//                logistic gradient at (p = -delta, y = 0) and the logistic hessian, from one exp.
//   omega        "pairwise": 1.  "lambdarank": (|gain(l_i) - gain(l_j)| * |disc[pos i] - disc[pos j]|) * inv_q, two products in that order; <= 1.
//   sums         lam = (double)rho * omega, kap = (double)eta * omega;  row i (the better): g -= lam, h += kap;  row j: g += lam, h += kap.  Every row
//                keeps its own two float64 sums from +0.0, partners in ascending row order, a partner with an equal label or a zero omega skipped;
//                g = (float)acc_g, h = (float)acc_h: one rounding.  No atomics: the bits do not depend on the launch geometry.
//   ndcg_q       DCG_q = sum over the query's rows, ascending, of gain(l) * disc[pos];  ndcg_q = maxDCG_q > 0 ? DCG_q * inv_q : 1.
//   loss         "lambdarank": 1 - (sum_q ndcg_q) / Q.  "pairwise" (device only, float64 libm): the mean over the P label-ordered pairs of the
//                logistic row loss at (p = delta, y = 1); 0 when P == 0.
//
// g is dL/dp as everywhere here.  Not LightGBM's lambdarank: no sigmoid parameter (it is 1), no lambdarank_norm, no position bias, no label_gain table.
#pragma once

#include <cmath>

#include "newton_core.h"

namespace gbrl {
namespace kern {

constexpr int kObjPairwise = 4, kObjLambdarank = 5;   // GBRL_HIP_OBJ_* (include/gbrl_hip.h)
constexpr int kRankMaxQuery = 1024, kRankMaxLabel = 30;
constexpr int kRankBadPred = kNewtonBadPred;          // bit of the kernels' flag word: a score that is not finite

inline bool rank_objective(int objective) { return objective == kObjPairwise || objective == kObjLambdarank; }

// the discount table (host only: one libm call per entry; everything else reads the table)
inline void rank_discount_table(double *disc) {
    for (int t = 0; t < kRankMaxQuery; ++t) disc[t] = 1.0 / std::log2(static_cast<double>(t) + 2.0);
}

// float64 steps, each rounded on its own on either side
GBRL_OBJ_HD inline double rank_mul(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
GBRL_OBJ_HD inline double rank_add(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
GBRL_OBJ_HD inline double rank_sub(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
GBRL_OBJ_HD inline double rank_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

GBRL_OBJ_HD inline bool rank_bad_label(int32_t l) { return l < 0 || l > kRankMaxLabel; }
GBRL_OBJ_HD inline double rank_gain(int32_t l) { return static_cast<double>((1ll << l) - 1); }
GBRL_OBJ_HD inline double rank_disc(const double *disc, int t, int ndcg_at) { return ndcg_at > 0 && t >= ndcg_at ? 0.0 : disc[t]; }
// row j stands before row i
GBRL_OBJ_HD inline bool rank_before(float sj, int j, float si, int i) { return sj > si || (sj == si && j < i); }
// one term of a DCG and one step of its sum
GBRL_OBJ_HD inline double rank_dcg_term(int32_t l, const double *disc, int t, int ndcg_at) { return rank_mul(rank_gain(l), rank_disc(disc, t, ndcg_at)); }
GBRL_OBJ_HD inline double rank_inverse(double max_dcg) { return max_dcg > 0.0 ? rank_div(1.0, max_dcg) : 0.0; }
GBRL_OBJ_HD inline double rank_ndcg(double dcg, double max_dcg, double inv) { return max_dcg > 0.0 ? rank_mul(dcg, inv) : 1.0; }

// a pair, `hi` the row of the larger label: rho and eta from the two scores
GBRL_OBJ_HD inline void rank_pair(float s_hi, float s_lo, float &rho, float &eta) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    const float delta = __fsub_rn(s_hi, s_lo);
#else
    const float delta = s_hi - s_lo;
#endif
    obj_logistic_grad_hess(-delta, 0.0f, rho, eta);
}

// lambdarank's pair weight from the two labels and positions
GBRL_OBJ_HD inline double rank_omega(int32_t l_a, int32_t l_b, int pos_a, int pos_b, const double *disc, int ndcg_at, double inv) {
    const double dg = rank_sub(rank_gain(l_a), rank_gain(l_b)), dd = rank_sub(rank_disc(disc, pos_a, ndcg_at), rank_disc(disc, pos_b, ndcg_at));
    return rank_mul(rank_mul(dg < 0.0 ? -dg : dg, dd < 0.0 ? -dd : dd), inv);
}

// what partner j adds to the sums of row i (the caller skips j == i and rows of other queries)
template <bool LAMBDARANK>
GBRL_OBJ_HD inline void rank_accumulate(float s_i, int32_t l_i, int pos_i, float s_j, int32_t l_j, int pos_j, const double *disc, int ndcg_at, double inv,
                                        double &acc_g, double &acc_h) {
    if (l_i == l_j) return;
    double omega = 1.0;
    if (LAMBDARANK) {
        omega = rank_omega(l_i, l_j, pos_i, pos_j, disc, ndcg_at, inv);
        if (!(omega > 0.0)) return;
    }
    const bool better = l_i > l_j;
    float rho, eta;
    rank_pair(better ? s_i : s_j, better ? s_j : s_i, rho, eta);
    const double lam = LAMBDARANK ? rank_mul(static_cast<double>(rho), omega) : static_cast<double>(rho);
    const double kap = LAMBDARANK ? rank_mul(static_cast<double>(eta), omega) : static_cast<double>(eta);
    acc_g = better ? rank_sub(acc_g, lam) : rank_add(acc_g, lam);
    acc_h = rank_add(acc_h, kap);
}

}  // namespace kern
}  // namespace gbrl
