// sample_core.h -- the row sampler of fit_prepared(subsample=) and PreparedDataset.sample_rows: ONE function of (seed, draw, row) that the host
// (Engine::sample_rows_host) and the device (sample_rows.hip) both call, so that a sample is the same list wherever it is drawn.
//
//   x   = (uint64(draw) << 32) | uint32(row)            draw: int32 >= 0; row: absolute row index in the data set
//   z   = x + (seed + 1) * 0x9E3779B97F4A7C15           seed: uint64; everything wraps
//   z  ^= z >> 30;  z *= 0xBF58476D1CE4E5B9             (the splitmix64 finaliser)
//   z  ^= z >> 27;  z *= 0x94D049BB133111EB
//   z  ^= z >> 31
//   u   = z >> 40                                       24 bits
//   thr = (uint32) floor(subsample * 2^24)              in double; subsample in [2^-24, 1] => thr in [1, 2^24]
//   the row is kept  <=>  u < thr                       (subsample == 1: u < 2^24 always -- no special case)
//
// The sample of a row range is the ascending list of its kept rows: without replacement, independent of how the range is cut into launches.
//
// The column rule of fit_prepared(colsample=) and PreparedDataset.sample_cols (host only: F is a few thousand at most).  For F columns, a
// fraction colsample in (0, 1] (not NaN), a seed and a draw:
//   k   = max(1, floor(colsample * F + 0.5))            in double; never above F
//   u_f = sample_u24(seed ^ 0x636F6C73616D706C, draw, f)   ("colsampl": a stream of its own beside the row sampler's)
//   the kept columns are the k smallest pairs (u_f, f), returned ascending in f
// Exactly k columns whatever the hash does (a Bernoulli rule varies too much at F = 16 and needs an empty-draw case); colsample == 1 keeps all.
//
// Gradient-based one-side sampling (GOSS; LightGBM's data_sample_strategy = "goss") of fit_prepared(goss=) and PreparedDataset.sample_goss.  For
// the rows [row0, row0 + n), their gradient rows G [n][D] (float32), fractions top_rate = a and other_rate = b, a seed and a draw:
//   score   s_r = 0; for d = 0 .. D-1: s_r = fl32(s_r + fl32(g_rd * g_rd))      float32, a separate multiply and add (never contracted): goss_score
//   key     bits(s_r) & 0x7FFFFFFF                                             non-negative floats order like their bits; an infinity or a NaN
//                                                                              ranks by its bits
//   top     k = floor(a * n) in double; tau = the k-th largest key.  A row is TOP iff its key is above tau, or equals tau and the row is among
//           the first k - #{key > tau} such rows in row order: exactly k top rows whatever the ties.  k == 0: no top row (tau is reported as
//           kGossNoTau, which is above every key).
//   other   a row that is not top is kept iff sample_u24(seed ^ 0x676F737372657374, draw, row) < min(2^24, floor(p * 2^24)), p = b / (1 - a) in
//           double ("gossrest": a stream of its own).  A Bernoulli draw like subsample's, NOT LightGBM's sequential draw of an exact count.
//   amp     fl32((1 - a) / b), the quotient in double.  A kept other row's gradient entries become obj_weighted(amp, g) (objective_core.h: one
//           float32 multiply); a top row's are copied, so no bit of them changes.
//   sample  the ascending list of the kept absolute rows, their factor (1 or amp) and their gathered gradient rows with the factor applied.
// Refused: a NaN rate, a outside [0, 1), b outside (0, 1], a + b > 1 (in double), p < 2^-24.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "objective_core.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_SAMPLE_HD __host__ __device__
#else
#define GBRL_SAMPLE_HD
#endif

namespace gbrl {
namespace kern {

GBRL_SAMPLE_HD inline uint32_t sample_u24(uint64_t seed, int32_t draw, uint32_t row) {
    uint64_t z = ((static_cast<uint64_t>(static_cast<uint32_t>(draw)) << 32) | row) + (seed + 1ull) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<uint32_t>(z >> 40);
}

GBRL_SAMPLE_HD inline bool sample_keeps(uint64_t seed, int32_t draw, uint32_t row, uint32_t thr) { return sample_u24(seed, draw, row) < thr; }

// a fraction the sampler takes: not NaN, in [2^-24, 1]
inline bool sample_fraction_ok(double subsample) { return subsample >= 1.0 / 16777216.0 && subsample <= 1.0; }
inline uint32_t sample_threshold(double subsample) { return static_cast<uint32_t>(subsample * 16777216.0); }   // (floor: the product is positive)


// the column rule (see the head of the file)
constexpr uint64_t kSampleColsStream = 0x636F6C73616D706Cull;
inline bool sample_cols_fraction_ok(double colsample) { return colsample > 0.0 && colsample <= 1.0; }   // (false for a NaN)
inline int sample_cols_count(int F, double colsample) {
    const double k = static_cast<double>(static_cast<long long>(colsample * static_cast<double>(F) + 0.5));   // (floor: the sum is positive)
    return static_cast<int>(std::min<double>(F, std::max(1.0, k)));
}
inline void sample_cols(int F, double colsample, uint64_t seed, int32_t draw, std::vector<int32_t> &out) {
    const int k = sample_cols_count(F, colsample);
    std::vector<std::pair<uint32_t, int32_t>> u(static_cast<size_t>(F));
    for (int f = 0; f < F; ++f) u[f] = {sample_u24(seed ^ kSampleColsStream, draw, static_cast<uint32_t>(f)), f};
    std::partial_sort(u.begin(), u.begin() + k, u.end());
    out.resize(static_cast<size_t>(k));
    for (int i = 0; i < k; ++i) out[i] = u[i].second;
    std::sort(out.begin(), out.end());
}


// one-side sampling (see the head of the file)
constexpr uint64_t kGossStream = 0x676F737372657374ull;
constexpr uint32_t kGossNoTau = 0x80000000u;   // k == 0: above every key
GBRL_SAMPLE_HD inline float goss_score_add(float s, float g) {   // fl32(s + fl32(g * g)): two roundings
    // (the operators themselves under the pragma, on the host and on the device: the _rn intrinsics are plain operators of a header that is
    // compiled with contraction allowed, and fuse once they are inlined)
#pragma clang fp contract(off)
    const float sq = g * g;
    return s + sq;
}
GBRL_SAMPLE_HD inline float goss_score(const float *g, int D) {
    float s = 0.0f;
    for (int d = 0; d < D; ++d) s = goss_score_add(s, g[d]);
    return s;
}
GBRL_SAMPLE_HD inline uint32_t goss_key(float score) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(score) & 0x7FFFFFFFu;
#else
    uint32_t u;
    std::memcpy(&u, &score, sizeof(u));
    return u & 0x7FFFFFFFu;
#endif
}
// top: a row with `key`, the tie_rank-th (from 0, in row order) of the rows whose key equals tau, of which the first `take` are top
GBRL_SAMPLE_HD inline bool goss_is_top(uint32_t key, uint32_t tau, uint32_t tie_rank, uint32_t take) { return key > tau || (key == tau && tie_rank < take); }

inline bool goss_rates_ok(double a, double b) {   // (false for a NaN in either)
    return a >= 0.0 && a < 1.0 && b > 0.0 && b <= 1.0 && a + b <= 1.0 && b / (1.0 - a) >= 1.0 / 16777216.0;
}
struct GossPlan { int k; uint32_t thr; float amp; };
inline GossPlan goss_plan(int n, double a, double b) {   // rates that goss_rates_ok accepts
    const double p = b / (1.0 - a);
    return GossPlan{static_cast<int>(a * static_cast<double>(n)), static_cast<uint32_t>(std::min(16777216.0, p * 16777216.0)), static_cast<float>((1.0 - a) / b)};
}
// the rule on the host: rows_out / factor_out [n] get the m kept rows and their factors, G_out (nullable, [n][D]) their gradient rows; returns m
inline int goss_rows(const float *G, int D, int row0, int n, double a, double b, uint64_t seed, int32_t draw, int32_t *rows_out, float *factor_out,
                     float *G_out, int *n_top, uint32_t *tau_bits) {
    const GossPlan plan = goss_plan(n, a, b);
    std::vector<uint32_t> key(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) key[i] = goss_key(goss_score(G + static_cast<size_t>(i) * D, D));
    uint32_t tau = kGossNoTau, take = 0;
    if (plan.k > 0) {
        std::vector<uint32_t> sorted(key);
        std::nth_element(sorted.begin(), sorted.begin() + (plan.k - 1), sorted.end(), [](uint32_t x, uint32_t y) { return x > y; });
        tau = sorted[plan.k - 1];
        take = static_cast<uint32_t>(plan.k);
        for (int i = 0; i < n; ++i) take -= key[i] > tau ? 1u : 0u;
    }
    int m = 0;
    uint32_t tie_rank = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t row = static_cast<uint32_t>(row0) + static_cast<uint32_t>(i);
        const bool top = goss_is_top(key[i], tau, tie_rank, take);
        tie_rank += key[i] == tau ? 1u : 0u;
        if (!top && !sample_keeps(seed ^ kGossStream, draw, row, plan.thr)) continue;
        rows_out[m] = static_cast<int32_t>(row);
        factor_out[m] = top ? 1.0f : plan.amp;
        if (G_out)
            for (int d = 0; d < D; ++d) {
                const float g = G[static_cast<size_t>(i) * D + d];
                G_out[static_cast<size_t>(m) * D + d] = top ? g : obj_weighted(plan.amp, g);
            }
        ++m;
    }
    if (n_top) *n_top = plan.k;
    if (tau_bits) *tau_bits = tau;
    return m;
}

}  // namespace kern
}  // namespace gbrl
