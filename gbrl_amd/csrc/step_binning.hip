// step_binning.hip -- uniform thresholds (column minima / maxima) and the bisection binning of GBRL::step: rows -> bin codes, and the exact
// 32-pass multi-rank selection of quantile candidates built on the same counting kernel.  (Radix selection: radix_select.hip, quantile.hip.)
#include "kernels.h"
#include "kernels_common.h"

#include <stdexcept>

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------
// A4  uniform candidates: per-column min / max (order independent => atomics are deterministic)
// ------------------------------------------------------------------------------------------------------------
// Column minima / maxima from the feature-major keys (the transpose has already run: every later pass streams columns).  One block
// per (row chunk, feature): 16-byte loads, eight in flight per thread, wave reduction, one atomic pair per wave.
__global__ __launch_bounds__(256) void k_column_minmax(const uint32_t *__restrict__ kt, int n, int rows_per_block, uint32_t *__restrict__ mn,
                                                       uint32_t *__restrict__ mx) {
    const int f = blockIdx.y;
    const uint32_t *col = kt + static_cast<size_t>(f) * n;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    uint32_t lo = 0xffffffffu, hi = 0u;
    constexpr uint32_t kMinFinite = 0x007fffffu;   // key of -inf; smaller keys are NaNs, which the reference's `<` / `>` scan never picks up
    auto upd = [&](uint32_t k) { if (k >= kMinFinite) { lo = min(lo, k); hi = max(hi, k); } };
    // the column start is 4-byte aligned only (n is arbitrary): peel to a 16-byte boundary, then vector loads
    int r = r0 + threadIdx.x;
    const uintptr_t mis = (reinterpret_cast<uintptr_t>(col + r0) >> 2) & 3;
    const int head = min(r1 - r0, static_cast<int>((4 - mis) & 3));
    if (threadIdx.x < head) upd(col[r]);
    const int v0 = r0 + head, nvec = (r1 - v0) / 4;
    const uint4 *vec = reinterpret_cast<const uint4 *>(col + v0);
    for (int i = threadIdx.x; i < nvec; i += 256 * 4) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = vec[min(i + u * 256, nvec - 1)];   // past the end: re-read the last vector (harmless for min / max)
#pragma unroll
        for (int u = 0; u < 4; ++u) { upd(q[u].x); upd(q[u].y); upd(q[u].z); upd(q[u].w); }
    }
    for (r = v0 + nvec * 4 + threadIdx.x; r < r1; r += 256) upd(col[r]);
    for (int o = kWave / 2; o > 0; o >>= 1) {
        lo = min(lo, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo), o, kWave)));
        hi = max(hi, static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi), o, kWave)));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMin(&mn[f], lo);
        atomicMax(&mx[f], hi);
    }
}
__global__ void k_uniform_thresholds(const uint32_t *__restrict__ mn, const uint32_t *__restrict__ mx, int F, int B,
                                     float *__restrict__ thr, uint32_t *__restrict__ thr_keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * B) return;
    const int f = i / B, b = i % B;
    const float lo = key_to_float(mn[f]), hi = key_to_float(mx[f]);
    const float step = (hi - lo) / static_cast<float>(B);
    // split_candidate_generator.cpp:67: min + b*step, contracted to ONE fma by the reference's release build (Q5)
    float t = fmaf(static_cast<float>(b), step, lo);
    // a column with infinite values gives inf - inf = NaN thresholds (in the reference too): a NaN threshold never passes `x > t`;
    // -inf is stored instead so that the key comparison of step() (NaN has no key above it) and predict()'s float comparison agree
    if (t != t) t = -INFINITY;
    thr[i] = t;
    if (thr_keys) thr_keys[i] = float_to_key(t);   // (what a k_floats_to_keys launch behind this one did)
}
}  // namespace

void column_minmax(const uint32_t *kt, int n, int F, uint32_t *mn, uint32_t *mx, hipStream_t s) {
    const int rows_per_block = 16384;
    dim3 grid((n + rows_per_block - 1) / rows_per_block, F);
    hipLaunchKernelGGL(k_column_minmax, grid, dim3(256), 0, s, kt, n, rows_per_block, mn, mx);
}

void uniform_thresholds(const uint32_t *mn, const uint32_t *mx, int F, int B, float *thr, hipStream_t s, uint32_t *thr_keys) {
    hipLaunchKernelGGL(k_uniform_thresholds, dim3((F * B + 255) / 256), dim3(256), 0, s, mn, mx, F, B, thr, thr_keys);
}

namespace {

// ------------------------------------------------------------------------------------------------------------
// A3  binning / counting:  j(row, f) = #{k : trial[f][k] (<|<=) key(obs[row,f])},  counts[f][j] += 1,
//     optionally codes[row][f] = j.  Used (a) by the exact quantile bisection (non-strict, counts only) and
//     (b) to turn observations into bin codes once thresholds are known (strict: code = #{k : t_k < x}).
// One block = FT features x (256/FT) rows per iteration; trial keys staged in LDS transposed ([k][f], f fastest)
// so that the lanes of a wave, which hold consecutive features, always hit distinct banks.
// ------------------------------------------------------------------------------------------------------------
constexpr int kBinThreads = 256;

// FT = features per block tile: 64 (256 B of each row) while the 2 B + 1 LDS rows of a feature fit, fewer features for more thresholds
template <bool STRICT, int FT>
__global__ __launch_bounds__(kBinThreads) void k_bin_rows(const float *__restrict__ obs, int n, int F,
                                                           const uint32_t *__restrict__ trial, int B,
                                                           unsigned long long *__restrict__ counts, uint16_t *__restrict__ codes,
                                                           int code_stride, int code_off) {
    extern __shared__ uint32_t lds[];
    uint32_t *t = lds;                    // [B][FT]
    uint32_t *cnt = lds + B * FT;     // [B+1][FT]
    const int f0 = blockIdx.y * FT;
    const int nf = min(FT, F - f0);
    for (int i = threadIdx.x; i < B * FT; i += kBinThreads) {
        const int k = i / FT, fl = i % FT;
        t[i] = fl < nf ? trial[static_cast<size_t>(f0 + fl) * B + k] : 0xffffffffu;
    }
    if (counts)
        for (int i = threadIdx.x; i < (B + 1) * FT; i += kBinThreads) cnt[i] = 0;
    __syncthreads();
    const int fl = threadIdx.x % FT;
    const int rsub = threadIdx.x / FT;
    constexpr int RPI = kBinThreads / FT;
    if (fl < nf) {
        for (int r = blockIdx.x * RPI + rsub; r < n; r += gridDim.x * RPI) {
            const uint32_t key = float_to_key(obs[static_cast<size_t>(r) * F + f0 + fl]);
            int lo = 0, hi = B;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const uint32_t tv = t[mid * FT + fl];
                const bool below = STRICT ? (tv < key) : (tv <= key);
                if (below) lo = mid + 1; else hi = mid;
            }
            if (counts) atomicAdd(&cnt[lo * FT + fl], 1u);
            if (codes) codes[static_cast<size_t>(r) * code_stride + code_off + f0 + fl] = static_cast<uint16_t>(lo);
        }
    }
    if (counts) {
        __syncthreads();
        for (int i = threadIdx.x; i < (B + 1) * FT; i += kBinThreads) {
            const int j = i / FT, f = i % FT;
            const uint32_t c = cnt[i];
            if (c != 0 && f < nf) atomicAdd(&counts[static_cast<size_t>(f0 + f) * (B + 1) + j], static_cast<unsigned long long>(c));
        }
    }
}
}  // namespace

template <bool STRICT, int FT>
static void launch_bin_rows(const float *obs, int n, int F, const uint32_t *trial_keys, int B, unsigned long long *counts, uint16_t *codes,
                            int code_stride, int code_off, hipStream_t s) {
    const int tiles = (F + FT - 1) / FT;
    const int rpi = kBinThreads / FT;
    dim3 grid(grid_for(static_cast<size_t>(n), rpi * 64, 1024), tiles);
    const size_t lds = (static_cast<size_t>(B) * FT + static_cast<size_t>(B + 1) * FT) * sizeof(uint32_t);
    static PerDeviceOnce attr_set;
    if (attr_set.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_bin_rows<STRICT, FT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    hipLaunchKernelGGL((k_bin_rows<STRICT, FT>), grid, dim3(kBinThreads), lds, s, obs, n, F, trial_keys, B, counts, codes, code_stride, code_off);
}

void bin_rows(const float *obs, int n, int F, const uint32_t *trial_keys, int B, bool strict, int64_t *counts_,
              uint16_t *codes, int code_stride, int code_off, hipStream_t s) {
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(counts_);
    // thresholds + class counters of one feature take (2 B + 1) LDS words: 64 features per tile up to 319 thresholds, 16 up to 1279, 4 up to 5119
    auto fits = [&](int ft) { return (static_cast<size_t>(2 * B + 1) * ft) * sizeof(uint32_t) <= 160 * 1024; };
#define GBRL_BIN_ROWS(FT) do { if (strict) launch_bin_rows<true, FT>(obs, n, F, trial_keys, B, counts, codes, code_stride, code_off, s); \
                                else launch_bin_rows<false, FT>(obs, n, F, trial_keys, B, counts, codes, code_stride, code_off, s); } while (0)
    if (fits(64)) GBRL_BIN_ROWS(64);
    else if (fits(16)) GBRL_BIN_ROWS(16);
    else if (fits(4)) GBRL_BIN_ROWS(4);
    else throw std::runtime_error("the 32-pass bisection selection of quantile candidates supports n_bins <= 5119");
#undef GBRL_BIN_ROWS
}

namespace {

// Exact multi-rank selection by bisection on the 32-bit ordered key (A3).  For every (feature, target k) we build the
// answer v_k = smallest key with #{keys <= v_k} >= cum_k from the most significant bit down: with prefix p_k (decided
// high bits, low bits zero) and trial t_k = p_k | bit, the bit is set iff #{keys < t_k} < cum_k.  Targets are sorted
// by rank, so prefixes and trials stay sorted per feature and one binary search per element serves all targets.
__global__ void k_qsel_init(uint32_t *__restrict__ prefix, uint32_t *__restrict__ trial, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    prefix[i] = 0u;
    trial[i] = 0x80000000u;
}
__global__ void k_qsel_update(uint32_t *__restrict__ prefix, uint32_t *__restrict__ trial,
                              const int64_t *__restrict__ counts, const int64_t *__restrict__ cum, int B, int bit,
                              int next_bit) {
    // one block per feature; thread k owns target k (loop if B > blockDim)
    extern __shared__ unsigned long long below[];  // [B+1] inclusive prefix of counts
    const int f = blockIdx.x;
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int j = 0; j <= B; ++j) {
            run += static_cast<unsigned long long>(counts[static_cast<size_t>(f) * (B + 1) + j]);
            below[j] = run;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < B; k += blockDim.x) {
        const size_t i = static_cast<size_t>(f) * B + k;
        uint32_t p = prefix[i];
        // #{keys < t_k} = sum_{j<=k'} counts[j] where k' = index of the LAST trial equal to t_k ... trials are sorted and
        // counts[j] holds rows with exactly j trials <= key, so rows with key < t_k are those with j <= (#trials < t_k).
        // With duplicated trials (equal targets) the rows sit in the bucket of the first duplicate; use that index.
        int first = k;
        const uint32_t tk = trial[i];
        while (first > 0 && trial[i - (k - first) - 1] == tk) --first;
        const long long c_below = static_cast<long long>(below[first]);
        if (c_below < cum[k]) p |= (1u << bit);
        prefix[i] = p;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < B; k += blockDim.x) {
        const size_t i = static_cast<size_t>(f) * B + k;
        trial[i] = next_bit >= 0 ? (prefix[i] | (1u << next_bit)) : prefix[i];
    }
}

// Threshold keys -> floats.  A selected key in the NaN range (a column with more NaNs than one quantile step) is raised to -inf's key,
// in place, so that the key comparison of step() and the float comparison of predict() keep agreeing: `x > -inf`.
__global__ void k_keys_to_floats(uint32_t *__restrict__ keys, float *__restrict__ out, size_t n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k = keys[i];
    if (k < 0x007fffffu) { k = 0x007fffffu; keys[i] = k; }
    out[i] = key_to_float(k);
}
__global__ void k_floats_to_keys(const float *__restrict__ in, uint32_t *__restrict__ keys, size_t n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = float_to_key(in[i]);
}
__global__ void k_iota(int32_t *__restrict__ rows, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rows[i] = i;
}
}  // namespace

void qsel_init(uint32_t *prefix, uint32_t *trial, int F, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_qsel_init, dim3((F * B + 255) / 256), dim3(256), 0, s, prefix, trial, F * B);
}
void qsel_update(uint32_t *prefix, uint32_t *trial, const int64_t *counts, const int64_t *cum, int F, int B, int bit,
                 int next_bit, hipStream_t s) {
    hipLaunchKernelGGL(k_qsel_update, dim3(F), dim3(256), (B + 1) * sizeof(unsigned long long), s, prefix, trial, counts,
                       cum, B, bit, next_bit);
}
void keys_to_floats(uint32_t *keys, float *out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_keys_to_floats, dim3((n + 255) / 256), dim3(256), 0, s, keys, out, n);
}
void floats_to_keys(const float *in, uint32_t *keys, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_floats_to_keys, dim3((n + 255) / 256), dim3(256), 0, s, in, keys, n);
}
void iota_rows(int32_t *rows, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, s, rows, n);
}

}  // namespace kern
}  // namespace gbrl
