// step_stats.hip -- gradient statistics of GBRL::step: column sums and maxima, the statistics chain (mean, standard deviation, fixed-point
// scales), quantisation, and the small element-wise helpers of the row-sharded statistics exchange.  Every kernel sits above its launcher.
#include "kernels.h"
#include "kernels_common.h"
#include "small_prep.h"

#include <algorithm>
#include <cmath>

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------
// A2  gradient statistics: out[d] = sum_i (g[i,d] - center[d])^2  (center != null)  or  sum_i g[i,d]
// Block size is a multiple of D so that every thread owns one column; per-block partials are combined by a single
// block in a fixed order => deterministic.
// FACTOR: the same loop and tree with a per-row factor, out[d] = sum_i (double)factor[i] * (double)g[i,d] (an exact product: a factor of 1 keeps
// every bit); g == nullptr stands for the one-hot matrix of `labels`.  The plain instantiation reads neither pointer.
// ------------------------------------------------------------------------------------------------------------
template <bool FACTOR>
__global__ void k_column_sums(const float *__restrict__ g, size_t n_el, int D, const float *__restrict__ center,
                              double *__restrict__ partials /*[blocks][2D]: sums then maxima*/, const float *__restrict__ factor,
                              const int32_t *__restrict__ labels) {
    extern __shared__ double sh[];  // [2*bs]
    const int bs = blockDim.x;
    const int col = threadIdx.x % D;
    const float c = center ? center[col] : 0.0f;
    double acc = 0.0;
    float mx = 0.0f;
    auto at = [&](size_t e) -> float {   // element e of the matrix
        if constexpr (FACTOR) {
            if (g == nullptr) return labels[e / D] == col ? 1.0f : 0.0f;
        }
        return g[e];
    };
    auto take = [&](float v, size_t e) {
        if constexpr (FACTOR) {
            acc += static_cast<double>(factor[e / D]) * static_cast<double>(v);
            mx = fmaxf(mx, fabsf(v));
        } else if (center) {
            const float dv = v - c;  // fp32 subtraction like the reference (math_ops.cpp:498)
            acc += static_cast<double>(dv) * static_cast<double>(dv);
            mx = fmaxf(mx, fabsf(dv));
        } else {
            acc += static_cast<double>(v);
            mx = fmaxf(mx, fabsf(v));
        }
    };
    // eight loads in flight per thread, accumulated in the order of the plain grid-stride loop (the sums keep their bits)
    const size_t stride = static_cast<size_t>(gridDim.x) * bs;
    size_t e = static_cast<size_t>(blockIdx.x) * bs + threadIdx.x;
    for (; e + 7 * stride < n_el; e += 8 * stride) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = at(e + u * stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) take(v[u], e + u * stride);
    }
    for (; e < n_el; e += stride) take(at(e), e);
    sh[threadIdx.x] = acc;
    sh[bs + threadIdx.x] = static_cast<double>(mx);
    __syncthreads();
    if (threadIdx.x < D) {
        double s = 0.0, m = 0.0;
        for (int t = threadIdx.x; t < bs; t += D) { s += sh[t]; m = fmax(m, sh[bs + t]); }
        partials[static_cast<size_t>(blockIdx.x) * 2 * D + threadIdx.x] = s;
        partials[static_cast<size_t>(blockIdx.x) * 2 * D + D + threadIdx.x] = m;
    }
}
__global__ __launch_bounds__(256) void k_column_sums_final(const double *__restrict__ partials, int n_blocks, int D,
                                                           double *__restrict__ out /*[2D]*/) {
    // one block per output (D sums, then D maxima); fixed-shape tree => deterministic
    __shared__ double sh[256];
    const int d = blockIdx.x;
    const bool is_max = d >= D;
    double s = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) {
        const double v = partials[static_cast<size_t>(b) * 2 * D + d];
        s = is_max ? fmax(s, v) : s + v;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] = is_max ? fmax(sh[threadIdx.x], sh[threadIdx.x + o]) : sh[threadIdx.x] + sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[d] = sh[0];
}
}  // namespace

int column_sums_blocks(int n, int D) { return grid_for(static_cast<size_t>(n) * D, 256 * 8, 1024); }

void column_sums(const float *g, int n, int D, const float *center, double *block_partials, int n_blocks, double *out,
                 hipStream_t s) {
    const int bs = D <= 256 ? (256 / D) * D : D;  // multiple of D so a thread owns one column
    hipLaunchKernelGGL(k_column_sums<false>, dim3(n_blocks), dim3(bs), 2 * bs * sizeof(double), s, g, static_cast<size_t>(n) * D, D,
                       center, block_partials, static_cast<const float *>(nullptr), static_cast<const int32_t *>(nullptr));
    hipLaunchKernelGGL(k_column_sums_final, dim3(2 * D), dim3(256), 0, s, block_partials, n_blocks, D, out);
}

void column_sums_weighted(const float *g, const int32_t *labels, const float *factor, int n, int D, double *block_partials, int n_blocks, double *out,
                          hipStream_t s) {
    const int bs = D <= 256 ? (256 / D) * D : D;  // column_sums' geometry
    hipLaunchKernelGGL(k_column_sums<true>, dim3(n_blocks), dim3(bs), 2 * bs * sizeof(double), s, g, static_cast<size_t>(n) * D, D,
                       static_cast<const float *>(nullptr), block_partials, factor, labels);
    hipLaunchKernelGGL(k_column_sums_final, dim3(2 * D), dim3(256), 0, s, block_partials, n_blocks, D, out);
}

namespace {

// Statistics chain on the device, operation for operation what the host path does (fitter.cpp:58-63, math_ops.cpp:464,510,94)
// with explicitly rounded fp32 intrinsics (no contraction).
__global__ __launch_bounds__(256) void k_stats_mean(const double *__restrict__ stat, long long n, int D, float *__restrict__ meanden) {
    for (int d = threadIdx.x; d < D; d += blockDim.x) meanden[d] = static_cast<float>(stat[d] / static_cast<double>(n));
}
__global__ __launch_bounds__(256) void k_stats_finish(const double *__restrict__ stat_raw, const double *__restrict__ stat_centred,
                                                      long long n, int D, int chunk_rows, float *__restrict__ meanden,
                                                      StepScales *__restrict__ sc) {
    __shared__ float m0[256], m1[256];
    float h0 = 0.0f, h1 = 0.0f;
    const float recip = __fdiv_rn(1.0f, __fsub_rn(static_cast<float>(n), 1.0f));
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        h1 = fmaxf(h1, static_cast<float>(stat_raw[D + d]));
        if (!(fabs(stat_raw[d]) < INFINITY)) h1 = INFINITY;            // a NaN / inf gradient poisons its column sum
        if (stat_centred && !(fabs(stat_centred[d]) < INFINITY)) h0 = INFINITY;
        if (stat_centred) {
            const float sd = __fsqrt_rn(__fmul_rn(static_cast<float>(stat_centred[d]), recip));
            const float den = __fadd_rn(sd, 1e-8f);
            meanden[D + d] = den;
            h0 = fmaxf(h0, __fmul_rn(__fdiv_rn(static_cast<float>(stat_centred[D + d]), den), 1.0001f));
        }
    }
    // NaN must survive the reduction (fmaxf drops it): carried as +inf, which the host rejects
    if (h0 != h0) h0 = INFINITY;
    if (h1 != h1) h1 = INFINITY;
    m0[threadIdx.x] = h0;
    m1[threadIdx.x] = h1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { m0[threadIdx.x] = fmaxf(m0[threadIdx.x], m0[threadIdx.x + o]); m1[threadIdx.x] = fmaxf(m1[threadIdx.x], m1[threadIdx.x + o]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float hraw = m1[0], hbuild = stat_centred ? m0[0] : m1[0];
        int sbits = 20;
        if (hbuild > 0.f && hbuild < INFINITY) sbits = min(100, ilog2_floor_dev(2147483647.0 / (static_cast<double>(chunk_rows) * hbuild)) - 1);
        const int lbits = leaf_sum_bits_dev(n, hraw);
        StepScales o{};
        o.sbits = sbits; o.lbits = lbits;
        o.scale = static_cast<float>(ldexp(1.0, sbits));
        o.inv_scale = ldexp(1.0, -sbits);
        o.leaf_scale = ldexp(1.0, lbits);
        o.hmax_build = hbuild; o.hmax_raw = hraw;
        *sc = o;
    }
}
}  // namespace

void stats_mean(const double *stat, long long n, int D, float *meanden, hipStream_t s) {
    hipLaunchKernelGGL(k_stats_mean, dim3(1), dim3(256), 0, s, stat, n, D, meanden);
}
void stats_finish(const double *stat_raw, const double *stat_centred, long long n, int D, int chunk_rows, float *meanden,
                  StepScales *sc, hipStream_t s) {
    hipLaunchKernelGGL(k_stats_finish, dim3(1), dim3(256), 0, s, stat_raw, stat_centred, n, D, chunk_rows, meanden, sc);
}

namespace {

// RL-sized batches (round 4): the whole statistics chain in ONE block -- small_prep.h, small_stats_body (shared with the fused
// preparation kernel of small_prep.hip).
__global__ __launch_bounds__(kSmallStatsThreads) void k_small_stats(const float *__restrict__ g, int n, int D, int n_blocks, int bs, int centred /*L2: standardise*/,
                                                                    int chunk_rows, double *__restrict__ stat /*[4D]*/, float *__restrict__ meanden /*[2D]*/,
                                                                    StepScales *__restrict__ sc, int32_t *__restrict__ qg) {
    extern __shared__ double sd[];                       // [V] sums, [V] maxima, then [n_blocks][2D] partials
    small_stats_body(g, n, D, n_blocks, bs, centred, chunk_rows, stat, meanden, sc, qg, sd);
}
}  // namespace

// RL-sized batches: statistics + quantisation in one launch (k_small_stats).  false: shape not covered, nothing was launched.
bool small_stats(const float *g, int n, int D, bool centred, int chunk_rows, double *stat, float *meanden, StepScales *sc, int32_t *qg, hipStream_t s) {
    const int n_blocks = column_sums_blocks(n, D);
    const int bs = D <= 256 ? (256 / D) * D : D;
    if (D > 16 || n_blocks * bs > kSmallStatsVirtual || n_blocks > 32 || n < 2) return false;
    const size_t lds = sizeof(double) * (2 * static_cast<size_t>(n_blocks) * bs + static_cast<size_t>(n_blocks) * 2 * D);
    if (lds > 156 * 1024) return false;
    // A device that refuses the LDS opt-in (or the launch) is remembered: every later call answers "nothing was launched" and the
    // caller runs the seven-kernel chain (the first version reported the failure on the first call only).
    static PerDeviceOnce attr;
    static uint64_t unsupported = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0;
    if (attr.first() && hipFuncSetAttribute(reinterpret_cast<const void *>(k_small_stats), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048) != hipSuccess) {
        (void)hipGetLastError();
        unsupported |= bit;
    }
    if (unsupported & bit) return false;
    hipLaunchKernelGGL(k_small_stats, dim3(1), dim3(kSmallStatsThreads), lds, s, g, n, D, n_blocks, bs, centred ? 1 : 0, chunk_rows, stat, meanden, sc, qg);
    if (hipGetLastError() != hipSuccess) { unsupported |= bit; return false; }
    return true;
}

namespace {

__device__ __forceinline__ float standardise(float v, const float *mean, const float *denom, int col) {
    // (g - mean) / (std + 1e-8f) evaluated in fp32 exactly like fitter.cpp:58-63 -> math_ops.cpp:498,94
    if (mean == nullptr) return v;
    return (v - mean[col]) / denom[col];
}

__global__ void k_quantize(const float *__restrict__ g, size_t n_el, int D, const float *__restrict__ mean,
                           const float *__restrict__ denom, const StepScales *__restrict__ sc, int32_t *__restrict__ qg) {
    const float scale = sc->scale;
    for (size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n_el;
         e += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const float v = standardise(g[e], mean, denom, static_cast<int>(e % D));
        qg[e] = __float2int_rn(v * scale);  // scale is a power of two: the product is exact, one rounding to integer
    }
}
}  // namespace

void quantize_grads(const float *g, size_t n_el, int D, const float *mean, const float *denom, const StepScales *sc, int32_t *qg,
                    hipStream_t s) {
    hipLaunchKernelGGL(k_quantize, dim3(grid_for(n_el, 256, 4096)), dim3(256), 0, s, g, n_el, D, mean, denom, sc, qg);
}

__global__ void k_sub_arrays(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out, size_t n) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x)
        out[i] = a[i] - b[i];
}
void sub_arrays(const float *a, const float *b, float *out, size_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_sub_arrays, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, a, b, out, n);
}
__global__ void k_gather_rows(const float *__restrict__ src, const int32_t *__restrict__ perm, float *__restrict__ dst, int n, int width) {
    const size_t total = static_cast<size_t>(n) * width;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const size_t r = i / width, c = i - r * width;
        dst[i] = src[static_cast<size_t>(perm[r]) * width + c];
    }
}
void gather_rows(const float *src, const int32_t *perm, float *dst, int n, int width, hipStream_t s) {
    const size_t total = static_cast<size_t>(n) * width;
    if (total == 0) return;
    hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(total, 256, 8192)), dim3(256), 0, s, src, perm, dst, n, width);
}
__global__ void k_f64_to_f32(const double *__restrict__ in, float *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = static_cast<float>(in[i]);
}
__global__ void k_f32_to_f64(const float *__restrict__ in, double *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = static_cast<double>(in[i]);
}
// Row-sharded statistics in ONE sum all-reduce: msg = [D column sums | P rows of D maxima, one per rank].  A rank writes its maxima
// into its own row and zeros into the others, so the SUM over ranks is a gather (x + 0 = x exactly; maxima are >= 0), and the maximum
// over the P rows is taken locally afterwards.  Replaces a sum all-reduce + a max all-reduce (and two conversion launches).
__global__ void k_stats_pack(const double *__restrict__ st /*[2D] sums | maxima*/, int D, int P, int rank, double *__restrict__ msg /*[D + P D + 1]*/, double extra) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) msg[D + P * D] = extra;     // one more summed word (the rank's row count in the first round)
    if (i < D) msg[i] = st[i];
    if (i < P * D) msg[D + i] = (i / D == rank) ? st[D + i % D] : 0.0;
}
__global__ void k_stats_unpack(const double *__restrict__ msg, int D, int P, double *__restrict__ st) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    st[d] = msg[d];
    double m = 0.0;
    for (int r = 0; r < P; ++r) m = fmax(m, msg[D + r * D + d]);
    st[D + d] = m;
}
void stats_pack(const double *st, int D, int P, int rank, double *msg, hipStream_t s, double extra) {
    hipLaunchKernelGGL(k_stats_pack, dim3((std::max(1, P) * D + D + 255) / 256), dim3(256), 0, s, st, D, P, rank, msg, extra);
}
void stats_unpack(const double *msg, int D, int P, double *st, hipStream_t s) {
    hipLaunchKernelGGL(k_stats_unpack, dim3((D + 255) / 256), dim3(256), 0, s, msg, D, P, st);
}
// -x for the first n floats (min over ranks = -max(-x): the column minima and maxima of uniform candidates travel in ONE max all-reduce)
__global__ void k_negate_f32(float *__restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = -p[i];
}
void negate_f32(float *p, int n, hipStream_t s) { hipLaunchKernelGGL(k_negate_f32, dim3((n + 255) / 256), dim3(256), 0, s, p, n); }
void f64_to_f32(const double *in, float *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_f64_to_f32, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void f32_to_f64(const float *in, double *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_f32_to_f64, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
}  // namespace kern
}  // namespace gbrl
