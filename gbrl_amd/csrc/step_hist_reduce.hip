// step_hist_reduce.hip -- from the int32 chunk partials of step_hist_build.hip to the int64 node histograms: reduce, and the two copies that
// place received or contiguous histograms into their level slots.
#include "kernels.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

// Sum the int32 chunk partials of every slot (node) into int64, reordering to hist[slot][feature][class][D+1].
// kReduceLanes chunk lanes per element: with many chunks per node (few feature groups => up to 256 chunks) a node's chunks are summed
// by 4 threads with four loads in flight each and combined through LDS; with the usual <= 32 chunks one thread per element is faster.
template <int kReduceLanes>
__global__ __launch_bounds__(256 * kReduceLanes) void k_hist_reduce(const int32_t *__restrict__ partials,
                                                                     const int32_t *__restrict__ slot_chunk_begin,
                                                                     const int32_t *__restrict__ slot_map, int n_groups, int FG, int NB,
                                                                     int D, int Fp, int64_t *__restrict__ hist, int scatter_fs,
                                                                     const uint32_t *__restrict__ root_le, int root_F, int root_B, long long root_n) {
    __shared__ int64_t part[kReduceLanes > 1 ? kReduceLanes - 1 : 1][256];
    const int n_acc = NB * (D + 1) * FG;
    const int k = blockIdx.z, g = blockIdx.y;
    const int slot = slot_map ? slot_map[k] : k;
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.y;
    const int c0 = slot_chunk_begin[k], c1 = slot_chunk_begin[k + 1];
    int64_t s = 0;
    if (i < n_acc) {
        const int32_t *src = partials + static_cast<size_t>(g) * n_acc + i;
        const size_t stride = static_cast<size_t>(n_groups) * n_acc;
        int c = c0 + lane;
        for (; c + 7 * kReduceLanes < c1; c += 8 * kReduceLanes) {   // eight independent loads in flight (integer sums: any order)
            int32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[(c + u * kReduceLanes) * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; c + 3 * kReduceLanes < c1; c += 4 * kReduceLanes) {
            const int32_t a = src[c * stride], b = src[(c + kReduceLanes) * stride], e = src[(c + 2 * kReduceLanes) * stride],
                          f = src[(c + 3 * kReduceLanes) * stride];
            s += static_cast<int64_t>(a) + b + e + f;
        }
        for (; c < c1; c += kReduceLanes) s += src[c * stride];
    }
    if (kReduceLanes > 1) {
        if (lane > 0) part[lane - 1][threadIdx.x] = s;
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < kReduceLanes - 1; ++q) s += part[q][threadIdx.x];
        }
    }
    const bool writer = lane == 0;     // the other chunk lanes stay until the last barrier and store nothing
    // The partials have the feature as the fastest index (the LDS layout of k_hist_build), the histograms the (class, field) pair:
    // the block's 256 sums are 16 features x 16 consecutive (class, field) elements when FG == 16.  Through a small LDS tile every
    // 16 lanes write 128 consecutive bytes of one feature instead of 16 features x 8 bytes.
    if (FG == 16) {
        __shared__ int64_t tile[16][17];
        if (writer) tile[threadIdx.x & 15][threadIdx.x >> 4] = s;
        __syncthreads();
        if (!writer) return;
        const int fl = threadIdx.x >> 4, el = threadIdx.x & 15;
        const int e = blockIdx.x * 16 + el;                       // (class, field) element: cls * (D + 1) + d
        const int f = g * FG + fl;
        if (e >= NB * (D + 1)) return;
        int64_t v = tile[fl][el];
        if (root_le && f < root_F) {   // the root's class counts from the selection: #{keys <= thr[c]} - #{keys <= thr[c-1]} (k_hist_build<COUNT = false>)
            const int cls = e / (D + 1);
            if (e - cls * (D + 1) == D) {
                const uint32_t *le = root_le + static_cast<size_t>(f) * root_B;
                const long long hi = cls < root_B ? static_cast<long long>(le[cls]) : root_n;
                const long long lo = cls == 0 ? 0ll : (cls - 1 < root_B ? static_cast<long long>(le[cls - 1]) : root_n);
                v = cls <= root_B ? hi - lo : 0;
            }
        }
        if (scatter_fs > 0) {   // send layout of the feature reduce-scatter: [owner rank][node k][feature inside the slice][class][D+1]
            if (f < Fp) hist[((static_cast<size_t>(f / scatter_fs) * gridDim.z + k) * scatter_fs + f % scatter_fs) * NB * (D + 1) + e] = v;
            return;
        }
        hist[(static_cast<size_t>(slot) * Fp + f) * NB * (D + 1) + e] = v;
        return;
    }
    if (!writer || i >= n_acc) return;
    const int fl = i % FG, d = (i / FG) % (D + 1), cls = i / (FG * (D + 1));
    const int f = g * FG + fl;
    if (scatter_fs > 0) {   // send layout of the feature reduce-scatter: [owner rank][node k][feature inside the slice][class][D+1]
        if (f < Fp) hist[(((static_cast<size_t>(f / scatter_fs) * gridDim.z + k) * scatter_fs + f % scatter_fs) * NB + cls) * (D + 1) + d] = s;
        return;
    }
    hist[((static_cast<size_t>(slot) * Fp + f) * NB + cls) * (D + 1) + d] = s;
}
}  // namespace

void hist_reduce(const int32_t *partials, const int32_t *slot_chunk_begin, const int32_t *slot_map, int n_slots, int n_groups, int FG,
                 int NB, int D, int Fp, int64_t *hist, hipStream_t s, int chunks_per_slot, int scatter_fs, const uint32_t *root_le, int root_F,
                 int root_B, long long root_n) {
    const int n_acc = NB * (D + 1) * FG;
    dim3 grid((n_acc + 255) / 256, n_groups, n_slots);
    if (FG != 16) root_le = nullptr;   // (the override lives in the FG == 16 store path; callers check hist_countless_supported)
    if (chunks_per_slot >= 48)
        hipLaunchKernelGGL(k_hist_reduce<4>, grid, dim3(256, 4), 0, s, partials, slot_chunk_begin, slot_map, n_groups, FG, NB, D, Fp, hist, scatter_fs, root_le, root_F, root_B, root_n);
    else
        hipLaunchKernelGGL(k_hist_reduce<1>, grid, dim3(256, 1), 0, s, partials, slot_chunk_begin, slot_map, n_groups, FG, NB, D, Fp, hist, scatter_fs, root_le, root_F, root_B, root_n);
}

namespace {

__global__ void k_hist_place_slice(const int64_t *__restrict__ recv, int64_t *__restrict__ hist, const int32_t *__restrict__ slot_map, int fs,
                                   int lo, int Fp, size_t feat_elems) {
    const int k = blockIdx.z, f = blockIdx.y;
    if (lo + f >= Fp) return;
    const int64_t *src = recv + (static_cast<size_t>(k) * fs + f) * feat_elems;
    int64_t *dst = hist + (static_cast<size_t>(slot_map[k]) * Fp + lo + f) * feat_elems;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < feat_elems; i += static_cast<size_t>(gridDim.x) * blockDim.x) dst[i] = src[i];
}
}  // namespace

void hist_place_slice(const int64_t *recv, int64_t *hist, const int32_t *slot_map, int n, int fs, int lo, int Fp, size_t feat_elems, hipStream_t s) {
    if (n <= 0 || fs <= 0) return;
    hipLaunchKernelGGL(k_hist_place_slice, dim3(static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(8, (feat_elems + 255) / 256))), fs, n), dim3(256), 0, s, recv, hist,
                       slot_map, fs, lo, Fp, feat_elems);
}

// Copies `n` contiguous node histograms into their level slots (dst slot = slot_map[k]).
__global__ void k_hist_place(const int64_t *__restrict__ src, int64_t *__restrict__ dst, const int32_t *__restrict__ slot_map,
                             size_t node_elems) {
    const int32_t slot = slot_map[blockIdx.y];
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < node_elems;
         i += static_cast<size_t>(gridDim.x) * blockDim.x)
        dst[static_cast<size_t>(slot) * node_elems + i] = src[static_cast<size_t>(blockIdx.y) * node_elems + i];
}
void hist_place(const int64_t *src, int64_t *dst, const int32_t *slot_map, int n, size_t node_elems, hipStream_t s) {
    const int bx = static_cast<int>(std::min<size_t>(256, (node_elems + 255) / 256));
    hipLaunchKernelGGL(k_hist_place, dim3(bx, n), dim3(256), 0, s, src, dst, slot_map, node_elems);
}

}  // namespace kern
}  // namespace gbrl
