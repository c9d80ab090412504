// cv_core.h -- control variates (the gradient variance reduction of the GBRL paper; Fitter::control_variates in the reference) as a call of its own:
// ONE definition of the chain, of the order every sum is taken in and of the coefficient, compiled by the host (cv_host.cpp, tests/cxx/cv_core_check.cpp)
// and by the device (control_variates.hip).  Every float32 operation is written out and contraction is off, so NumPy float32 restates the rule bit for bit.
//
//   chain        per row and output j, over the trees t of [start, T) in order, leaf = the row walk's leaf (predict_rowwalk.h; -1 ends the walk):
//                m_j = fl32(fl32(beta * m_j) + fl32(c * values[leaf][j])), c = fl32(1 - beta): three roundings, no fused multiply-add, no learning rate,
//                no optimizer ownership.  m starts from the caller's held raw average, or from zero.
//   scale        scale = 1 / sqrtf(1 - powf(beta, (float)T)) in float32 on the host (0 for a model without trees); ms = fl32(m * scale).
//   sums         float64, in ONE order.  A SLOT is the sum of up to 64 per-lane values by the wave butterfly (lane i adds lane i ^ off, off = 32 .. 1; a
//                lane without a row holds 0.0).  Pass 1 writes one slot per 64 consecutive rows: sum g and sum ms.  The moments pass writes
//                cv_moment_slots(n) slots: slot q takes the 64-row tiles q, q + S, q + 2 S, ... -- lane i adds its row of each tile in turn -- of
//                (double)mc * (double)mc and (double)gc * (double)mc (exact products).  A FOLD of S slots is again a butterfly: lane i adds the slots
//                i, i + 64, ... in turn.  gbar = fl32(fold(g) / n), mbar = fl32(fold(ms) / n), gc = fl32(g - gbar), mc = fl32(ms - mbar),
//                var = fl32(fold(mc^2) / (n - 1)), cov = fl32(fold(gc mc) / (n - 1)).
//   coefficient  alpha = clamp(fl32(cov / fl32(var + 1e-8f)), -1, 1); a NaN stays a NaN (the call then fails).
//   result       g' = fl32(g - fl32(mc * alpha)).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "leaf_accum.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_CV_HD __host__ __device__
#else
#define GBRL_CV_HD
#endif

namespace gbrl {
namespace kern {

constexpr int kCvSlotRows = 64;        // rows of a pass-1 slot and of a tile of the moments pass: one wave
constexpr int kCvMomentSlots = 2048;   // the most slots the moments pass writes: every block of the apply pass folds them
constexpr int kCvWalkTrees = 16;       // trees a lane walks into leaf indices before it gathers their values
constexpr int kCvStreamMaxD = 64, kCvMaxD = 128;
constexpr int kCvStats = 5;            // rows of the statistics matrix [kCvStats][D]:
constexpr int kCvAlpha = 0, kCvMeanGrads = 1, kCvMeanMomentum = 2, kCvVar = 3, kCvCov = 4;

// One float32 operation, one rounding.  Written as plain operators under contract(off): the operations carry no permission to fuse, whatever the
// file's -ffp-contract says (the __fmul_rn / __fadd_rn intrinsics are plain operators of the HIP headers and DO fuse into an fma when inlined).
// The volatile on the host pins the rounding to float32 on every host compiler.
GBRL_CV_HD inline float cv_mul(float a, float b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return a * b;
#else
    volatile float r = a * b;
    return r;
#endif
}
GBRL_CV_HD inline float cv_add(float a, float b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return a + b;
#else
    volatile float r = a + b;
    return r;
#endif
}
GBRL_CV_HD inline float cv_sub(float a, float b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return a - b;
#else
    volatile float r = a - b;
    return r;
#endif
}
GBRL_CV_HD inline float cv_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    volatile float r = a / b;
    return r;
#endif
}

// one tree of the chain
GBRL_CV_HD inline float cv_chain(float m, float beta, float c, float v) { return cv_add(cv_mul(beta, m), cv_mul(c, v)); }
// the bias correction for an ensemble of T trees (host: powf's last bit is the platform's)
inline float cv_scale(float beta, int T) { return T > 0 ? 1.0f / sqrtf(1.0f - powf(beta, static_cast<float>(T))) : 0.0f; }
inline bool cv_beta_ok(float beta) { return beta > 0.0f && beta < 1.0f; }   // (false for a NaN)

GBRL_CV_HD inline float cv_mean(double sum, long long n) { return static_cast<float>(sum / static_cast<double>(n)); }
GBRL_CV_HD inline float cv_moment(double sum, long long n) { return static_cast<float>(sum / static_cast<double>(n - 1)); }
GBRL_CV_HD inline float cv_alpha(float cov, float var) {
    const float a = cv_div(cov, cv_add(var, 1e-8f));
    return a > 1.0f ? 1.0f : (a < -1.0f ? -1.0f : a);
}
GBRL_CV_HD inline float cv_corrected(float g, float mc, float alpha) { return cv_sub(g, cv_mul(mc, alpha)); }

// ------------------------------------------------------------------------------------------------------------ the launch plan (no device)
GBRL_CV_HD inline int cv_walk_slots(long long n) { return static_cast<int>((n + kCvSlotRows - 1) / kCvSlotRows); }
inline int cv_moment_slots(long long n) { return std::min(cv_walk_slots(n), kCvMomentSlots); }
// value rows in flight beside the D averages of a lane: 32 floats' worth, between 1 and 8 trees
constexpr int cv_value_group(int dmax) { return dmax <= 4 ? 8 : dmax <= 8 ? 4 : dmax <= 16 ? 2 : 1; }
constexpr int cv_stream_dmax(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }

struct CvPlan {
    int streaming;      // 1: the lane-per-row kernel on an LDS tile; 0: one thread per row, rows read in place
    int dmax;           // template width of the walk
    int walk_trees;     // leaves a lane holds before it gathers values (streaming)
    int value_trees;    // value rows gathered together (streaming)
    int walk_slots, moment_slots;
    int launches;       // of a call that walks: walk, fold, moments, apply
    size_t lds;         // dynamic LDS of a block of the walk
};
// width: the float row's features, or (codes) the data set's 16-column groups.  `streamable`: what leaves_streamable says of the model.
inline CvPlan cv_plan(long long n, int width, bool codes, int D, bool streamable = true) {
    CvPlan p{};
    const size_t tile = codes ? static_cast<size_t>(kCvSlotRows) * ((static_cast<size_t>(width) * 8) | 1) * sizeof(uint32_t)
                              : static_cast<size_t>(kCvSlotRows) * (static_cast<size_t>(width) | 1) * sizeof(float);
    p.streaming = streamable && D <= kCvStreamMaxD && tile <= kStreamLdsBudget;
    p.dmax = p.streaming ? cv_stream_dmax(D) : (D <= 8 ? 8 : D <= 32 ? 32 : 128);
    p.walk_trees = p.streaming ? kCvWalkTrees : 1;
    p.value_trees = p.streaming ? cv_value_group(p.dmax) : 1;
    p.walk_slots = cv_walk_slots(n);
    p.moment_slots = cv_moment_slots(n);
    p.launches = 4;
    p.lds = p.streaming ? tile : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------------------ the sums on the host
// the wave butterfly on 64 values: what every lane holds at the end
inline double cv_butterfly(double (&v)[kCvSlotRows]) {
    for (int off = kCvSlotRows / 2; off >= 1; off >>= 1) {
        double w[kCvSlotRows];
        for (int i = 0; i < kCvSlotRows; ++i) w[i] = v[i] + v[i ^ off];
        for (int i = 0; i < kCvSlotRows; ++i) v[i] = w[i];
    }
    return v[0];
}
// fold of S slots of column c (slots are rows of C doubles)
inline double cv_fold(const double *part, int S, int C, int c) {
    double lane[kCvSlotRows];
    for (int i = 0; i < kCvSlotRows; ++i) {
        double acc = 0.0;
        for (int s = i; s < S; s += kCvSlotRows) acc += part[static_cast<size_t>(s) * C + c];
        lane[i] = acc;
    }
    return cv_butterfly(lane);
}

// Everything behind the chain: from the gradients g and the raw averages m, both [n][D], the corrected gradients out [n][D] and the statistics
// stats [kCvStats][D].  ms [n][D] and part [cv_walk_slots(n)][2 D] are the caller's scratch.  n >= 2.
inline void cv_finish_host(const float *g, const float *m, long long n, int D, float scale, float *ms, double *part, float *out, float *stats) {
    const int S1 = cv_walk_slots(n), S2 = cv_moment_slots(n), C = 2 * D;
    for (long long i = 0; i < n * D; ++i) ms[i] = cv_mul(m[i], scale);
    for (int s = 0; s < S1; ++s)
        for (int j = 0; j < D; ++j) {
            double a[kCvSlotRows], b[kCvSlotRows];
            for (int i = 0; i < kCvSlotRows; ++i) {
                const long long r = static_cast<long long>(s) * kCvSlotRows + i;
                a[i] = r < n ? static_cast<double>(g[r * D + j]) : 0.0;
                b[i] = r < n ? static_cast<double>(ms[r * D + j]) : 0.0;
            }
            part[static_cast<size_t>(s) * C + j] = cv_butterfly(a);
            part[static_cast<size_t>(s) * C + D + j] = cv_butterfly(b);
        }
    for (int j = 0; j < D; ++j) {
        stats[kCvMeanGrads * D + j] = cv_mean(cv_fold(part, S1, C, j), n);
        stats[kCvMeanMomentum * D + j] = cv_mean(cv_fold(part, S1, C, D + j), n);
    }
    for (int q = 0; q < S2; ++q)   // (the walk's slots are folded: the array is reused, S2 <= S1)
        for (int j = 0; j < D; ++j) {
            const float gbar = stats[kCvMeanGrads * D + j], mbar = stats[kCvMeanMomentum * D + j];
            double a[kCvSlotRows], b[kCvSlotRows];
            for (int i = 0; i < kCvSlotRows; ++i) {
                a[i] = b[i] = 0.0;
                for (long long r = static_cast<long long>(q) * kCvSlotRows + i; r < n; r += static_cast<long long>(S2) * kCvSlotRows) {
                    const double mc = static_cast<double>(cv_sub(ms[r * D + j], mbar)), gc = static_cast<double>(cv_sub(g[r * D + j], gbar));
                    a[i] += mc * mc;
                    b[i] += gc * mc;
                }
            }
            part[static_cast<size_t>(q) * C + j] = cv_butterfly(a);
            part[static_cast<size_t>(q) * C + D + j] = cv_butterfly(b);
        }
    for (int j = 0; j < D; ++j) {
        const float var = cv_moment(cv_fold(part, S2, C, j), n), cov = cv_moment(cv_fold(part, S2, C, D + j), n);
        stats[kCvVar * D + j] = var;
        stats[kCvCov * D + j] = cov;
        stats[kCvAlpha * D + j] = cv_alpha(cov, var);
    }
    for (long long r = 0; r < n; ++r)
        for (int j = 0; j < D; ++j)
            out[r * D + j] = cv_corrected(g[r * D + j], cv_sub(ms[r * D + j], stats[kCvMeanMomentum * D + j]), stats[kCvAlpha * D + j]);
}

}  // namespace kern
}  // namespace gbrl
