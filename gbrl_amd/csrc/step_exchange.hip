// step_exchange.hip -- what a step moves between device, pinned host memory and the other ranks: publish / fetch / stage / fill launches,
// the packed winner exchange of feature-sharded levels and the localisation of row-sharded ones.
#include "kernels.h"
#include "kernels_common.h"

#include <algorithm>
#include <cmath>

namespace gbrl {
namespace kern {

namespace {

__global__ __launch_bounds__(256) void k_publish_block(uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int words, uint32_t *flag,
                                                       uint32_t seq, int zero_src) {
    for (int i = threadIdx.x; i < words; i += 256) {
        __builtin_nontemporal_store(src[i], &dst[i]);
        if (zero_src) src[i] = 0;      // accumulators handed back clean: the next tree needs no memset
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Two device arrays copied into pinned, device-mapped host memory by one launch (no flag: whoever reads them has polled a later
// publication of the same stream).
__global__ __launch_bounds__(256) void k_publish_pair(const uint32_t *__restrict__ a, uint32_t *__restrict__ ha, int a_words,
                                                      const uint32_t *__restrict__ b, uint32_t *__restrict__ hb, int b_words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a_words) __builtin_nontemporal_store(a[i], &ha[i]);
    if (i < b_words) __builtin_nontemporal_store(b[i], &hb[i]);
}
}  // namespace

void publish_block(void *d_src, void *h_dst_mapped, size_t bytes, uint32_t *flag_mapped, uint32_t seq, hipStream_t s, bool zero_src) {
    hipLaunchKernelGGL(k_publish_block, dim3(1), dim3(256), 0, s, static_cast<uint32_t *>(d_src), static_cast<uint32_t *>(h_dst_mapped),
                       static_cast<int>(bytes / 4), flag_mapped, seq, zero_src ? 1 : 0);
}
void publish_pair(const void *d_a, void *h_a_mapped, size_t a_bytes, const void *d_b, void *h_b_mapped, size_t b_bytes, hipStream_t s) {
    const int aw = static_cast<int>(a_bytes / 4), bw = static_cast<int>(b_bytes / 4);
    hipLaunchKernelGGL(k_publish_pair, dim3((std::max(aw, bw) + 255) / 256), dim3(256), 0, s, static_cast<const uint32_t *>(d_a),
                       static_cast<uint32_t *>(h_a_mapped), aw, static_cast<const uint32_t *>(d_b), static_cast<uint32_t *>(h_b_mapped), bw);
}

namespace {

__global__ __launch_bounds__(256) void k_fetch_segments(FetchSegments fs) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < fs.n && i < fs.words[k]) static_cast<uint32_t *>(fs.dst[k])[i] = static_cast<const uint32_t *>(fs.src[k])[i];
}
__global__ __launch_bounds__(256) void k_stage_copy(StageSegments ss, const char *__restrict__ stage) {
    const int k = blockIdx.y;
    if (k >= ss.n) return;
    char *dst = static_cast<char *>(ss.dst[k]);
    const char *src = stage + ss.src_off[k];
    const uint32_t n = ss.bytes[k];
    const uint32_t i0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 3u) == 0) {
        for (uint32_t i = i0; i < n / 4; i += stride) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
        for (uint32_t i = (n & ~3u) + i0; i < n; i += stride) dst[i] = src[i];
    } else {
        for (uint32_t i = i0; i < n; i += stride) dst[i] = src[i];
    }
}
__global__ __launch_bounds__(256) void k_fill_segments(FillSegments fs) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < fs.n && i < fs.words[k]) static_cast<uint32_t *>(fs.dst[k])[i] = fs.value[k];
}
__global__ void k_fill_f32(float *__restrict__ p, size_t n, float v) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
}  // namespace

void fetch_segments(const FetchSegments &fs, hipStream_t s) {
    uint32_t mx = 0;
    for (int k = 0; k < fs.n; ++k) mx = std::max(mx, fs.words[k]);
    if (mx) hipLaunchKernelGGL(k_fetch_segments, dim3((mx + 255) / 256), dim3(256), 0, s, fs);
}
void stage_copy(const StageSegments &ss, const void *stage_mapped, hipStream_t s) {
    uint32_t mx = 0;
    for (int k = 0; k < ss.n; ++k) mx = std::max(mx, ss.bytes[k]);
    if (!mx || ss.n <= 0) return;
    const unsigned bx = std::min<unsigned>(64, (mx / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(k_stage_copy, dim3(bx, ss.n), dim3(256), 0, s, ss, static_cast<const char *>(stage_mapped));
}
void fill_segments(const FillSegments &fs, hipStream_t s) {
    uint32_t mx = 0;
    for (int k = 0; k < fs.n; ++k) mx = std::max(mx, fs.words[k]);
    if (mx) hipLaunchKernelGGL(k_fill_segments, dim3((mx + 255) / 256), dim3(256), 0, s, fs);
}
void fill_f32(float *p, size_t n, float v, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_fill_f32, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

namespace {

// see kernels.h: winner_pack / winner_adopt
__global__ void k_winner_pack(const int32_t *__restrict__ best_idx, const float *__restrict__ best_score, const int64_t *__restrict__ counts4,
                              int max_front, int n_win, int n_act, int rank, int64_t *__restrict__ gather, int P) {
    // (the other ranks' rows are cleared here: the sum over ranks is a gather; round 5: no memset launch in front of this one)
    const size_t stride = static_cast<size_t>(n_win) + 2 * n_act;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < stride * P; i += static_cast<size_t>(gridDim.x) * blockDim.x)
        if (i / stride != static_cast<size_t>(rank)) gather[i] = 0;
    int64_t *row = gather + static_cast<size_t>(rank) * (n_win + 2 * n_act);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_win) {
        const uint64_t key = (static_cast<uint64_t>(float_to_key(best_score[t])) << 32) | (0xffffffffu - static_cast<uint32_t>(best_idx[t]));
        row[t] = static_cast<int64_t>(key);
    }
    if (t < n_act) {
        row[n_win + 2 * t] = counts4[t];                                           // total rows of node t (global histogram)
        row[n_win + 2 * t + 1] = counts4[static_cast<size_t>(max_front) + t];      // rows right of this rank's best candidate
    }
}
__global__ void k_winner_adopt(const int64_t *__restrict__ gather, int P, int n_win, int n_act, int oblivious,
                               const int32_t *__restrict__ ref_to_internal, const int32_t *__restrict__ cand_slot, const FeatureSlot *__restrict__ slots,
                               const int32_t *__restrict__ seg_start, const uint32_t *__restrict__ thr_keys, int B, int32_t *__restrict__ best_idx,
                               float *__restrict__ best_score, int64_t *__restrict__ counts4, int max_front, NodeSplit *__restrict__ out,
                               int32_t *__restrict__ cursors) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_act) return;
    const int w = oblivious ? 0 : k;
    const size_t stride = static_cast<size_t>(n_win) + 2 * n_act;
    uint64_t best_key = 0;
    int owner = 0;
    for (int r = 0; r < P; ++r) {
        const uint64_t key = static_cast<uint64_t>(gather[r * stride + w]);
        if (r == 0 || key > best_key) { best_key = key; owner = r; }
    }
    const float score = key_to_float(static_cast<uint32_t>(best_key >> 32));
    const int idx = static_cast<int>(0xffffffffu - static_cast<uint32_t>(best_key & 0xffffffffu));
    const long long tot = gather[owner * stride + n_win + 2 * k], right = gather[owner * stride + n_win + 2 * k + 1];
    if (k == w || !oblivious) { best_idx[w] = idx; best_score[w] = score; }
    counts4[k] = tot;
    counts4[static_cast<size_t>(max_front) + k] = right;
    counts4[2 * static_cast<size_t>(max_front) + k] = 0;   // this rank's rows going right: counted next (k_count_right adds into it)
    const int j = ref_to_internal[idx];
    const int fs = cand_slot[j];
    const FeatureSlot sl = slots[fs];
    NodeSplit q{};
    q.fslot = fs;
    q.bin = sl.is_cat ? (j - sl.cand_base + 1) : (j - sl.cand_base);
    q.is_cat = sl.is_cat;
    q.thr_key = (!sl.is_cat && thr_keys) ? thr_keys[static_cast<size_t>(fs) * B + q.bin] : 0u;
    q.do_split = oblivious ? (score != -INFINITY) : (score >= 0.0f);
    q.seg_start = seg_start[k];
    q.n_left = static_cast<int>(tot - right);   // global; k_localize_splits replaces it by this rank's
    cursors[2 * k] = 0;
    cursors[2 * k + 1] = 0;
    out[k] = q;
}
}  // namespace

void winner_pack(const int32_t *best_idx, const float *best_score, const int64_t *counts4, int max_front, int n_win, int n_act, int rank,
                 int64_t *gather, hipStream_t s, int P) {
    hipLaunchKernelGGL(k_winner_pack, dim3((n_act + 63) / 64), dim3(64), 0, s, best_idx, best_score, counts4, max_front, n_win, n_act, rank, gather, P);
}
void winner_adopt(const int64_t *gather, int P, int n_win, int n_act, bool oblivious, const int32_t *ref_to_internal, const int32_t *cand_slot,
                  const FeatureSlot *slots, const int32_t *seg_start, const uint32_t *thr_keys, int B, int32_t *best_idx, float *best_score,
                  int64_t *counts4, int max_front, NodeSplit *out, int32_t *cursors, hipStream_t s) {
    hipLaunchKernelGGL(k_winner_adopt, dim3((n_act + 63) / 64), dim3(64), 0, s, gather, P, n_win, n_act, oblivious ? 1 : 0, ref_to_internal, cand_slot,
                       slots, seg_start, thr_keys, B, best_idx, best_score, counts4, max_front, out, cursors);
}

// Row-sharded runs: k_resolve_splits wrote GLOBAL left sizes; the partition needs this rank's.
__global__ void k_localize_splits(NodeSplit *__restrict__ splits, const int32_t *__restrict__ n_local,
                                  const int64_t *__restrict__ right_local, int n_nodes) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_nodes) splits[k].n_left = n_local[k] - static_cast<int32_t>(right_local[k]);
}
void localize_splits(NodeSplit *splits, const int32_t *n_local, const int64_t *right_local, int n_nodes, hipStream_t s) {
    hipLaunchKernelGGL(k_localize_splits, dim3((n_nodes + 63) / 64), dim3(64), 0, s, splits, n_local, right_local, n_nodes);
}
// the two in one launch (row-sharded levels: global left sizes -> this rank's, then the level's result block goes to the host)
__global__ __launch_bounds__(256) void k_localize_publish(NodeSplit *__restrict__ splits, const int32_t *__restrict__ n_local, const int64_t *__restrict__ right_local,
                                                          int n_nodes, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int words, uint32_t *flag, uint32_t seq) {
    for (int k = threadIdx.x; k < n_nodes; k += 256) splits[k].n_left = n_local[k] - static_cast<int32_t>(right_local[k]);
    for (int i = threadIdx.x; i < words; i += 256) __builtin_nontemporal_store(src[i], &dst[i]);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void localize_publish(NodeSplit *splits, const int32_t *n_local, const int64_t *right_local, int n_nodes, void *d_src, void *h_dst_mapped, size_t bytes,
                      uint32_t *flag_mapped, uint32_t seq, hipStream_t s) {
    hipLaunchKernelGGL(k_localize_publish, dim3(1), dim3(256), 0, s, splits, n_local, right_local, n_nodes, static_cast<const uint32_t *>(d_src),
                       static_cast<uint32_t *>(h_dst_mapped), static_cast<int>(bytes / 4), flag_mapped, seq);
}

}  // namespace kern
}  // namespace gbrl
