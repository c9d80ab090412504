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
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

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

}  // namespace kern
}  // namespace gbrl
