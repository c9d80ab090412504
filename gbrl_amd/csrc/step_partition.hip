// step_partition.hip -- the row side of a tree level: partition of every splitting node's rows into its children, the count of rows a split
// sends right (row-sharded levels), and the exact leaf sums of the raw gradients.
#include "kernels.h"
#include "kernels_common.h"

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------
// A9  partition: every splitting node's segment [seg_start, seg_start+n) of the row list is split into [left | right] in
// place of the same range of the output list.  Destination slots are handed
// out with one wave-aggregated atomic per side; the order inside a child is not the reference's stable order, which is
// harmless because everything computed downstream is an order-independent integer sum.
// ------------------------------------------------------------------------------------------------------------
constexpr int kPartThreads = 1024;
constexpr int kPartRows = 4096;  // rows per block: 4 per thread, all loads issued before the ballots
__global__ __launch_bounds__(kPartThreads) void k_partition(const int32_t *__restrict__ rows_in, int32_t *__restrict__ rows_out,
                                                            const uint16_t *__restrict__ codes, const uint32_t *__restrict__ kt, int n_rows,
                                                            const Chunk *__restrict__ chunks, const NodeSplit *__restrict__ splits,
                                                            int32_t *__restrict__ cursors) {
    const Chunk ck = chunks[blockIdx.x];
    if (ck.len <= 0) return;    // unused entry of a device-planned chunk table
    const NodeSplit sp = splits[ck.slot];
    if (!sp.do_split) return;   // the node became a leaf (its segment stays in the input list)
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int U = kPartRows / kPartThreads;
    int row[U];
    bool right[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int p = u * kPartThreads + threadIdx.x;
        row[u] = p < ck.len ? rows_in[ck.start + p] : -1;
    }
    if (!sp.is_cat && kt) {
        // numeric split: code > bin <=> key > threshold key (the thresholds are sorted); the keys are feature-major, so the rows
        // of a node cost 4 bytes each instead of a 32-byte code record
        const uint32_t *kcol = kt + static_cast<size_t>(sp.fslot) * n_rows;
#pragma unroll
        for (int u = 0; u < U; ++u) right[u] = row[u] >= 0 && kcol[row[u]] > sp.thr_key;
    } else {
        const uint16_t *cbase = codes + (static_cast<size_t>(sp.fslot >> 4) * n_rows) * kCodeGroup + (sp.fslot & (kCodeGroup - 1));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int code = row[u] >= 0 ? cbase[static_cast<size_t>(row[u]) * kCodeGroup] : 0;
            right[u] = sp.is_cat ? (code == sp.bin) : (code > sp.bin);
        }
    }
    // destination slots: ballots give the rank inside a wave; per-(wave,u) counts are scanned in LDS and the block reserves
    // its range with ONE global atomic per side (at level 0 every wave of the grid would otherwise hit the same two words).
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (kWave - lane));
    constexpr int W = kPartThreads / kWave;
    __shared__ int cnt[W * U][2];
    __shared__ int base[2];
    const int wave = threadIdx.x / kWave;
    unsigned long long mr[U], ml[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool active = row[u] >= 0;
        mr[u] = __ballot(active && right[u]);
        ml[u] = __ballot(active && !right[u]);
        if (lane == 0) { cnt[wave * U + u][1] = __popcll(mr[u]); cnt[wave * U + u][0] = __popcll(ml[u]); }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int side = threadIdx.x;
        int run = 0;
        for (int q = 0; q < W * U; ++q) { const int c = cnt[q][side]; cnt[q][side] = run; run += c; }
        base[side] = run ? atomicAdd(&cursors[ck.slot * 2 + side], run) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (row[u] < 0) continue;
        const int off = cnt[wave * U + u][right[u] ? 1 : 0];
        const int dst = right[u] ? (sp.seg_start + sp.n_left + base[1] + off + __popcll(mr[u] & below))
                                 : (sp.seg_start + base[0] + off + __popcll(ml[u] & below));
        rows_out[dst] = row[u];
    }
}
}  // namespace

void partition_rows(const int32_t *rows_in, int32_t *rows_out, const uint16_t *codes, const uint32_t *kt, int n_rows, const Chunk *chunks,
                    int n_chunks, const NodeSplit *splits, int32_t *cursors, hipStream_t s) {
    hipLaunchKernelGGL(k_partition, dim3(n_chunks), dim3(kPartThreads), 0, s, rows_in, rows_out, codes, kt, n_rows, chunks, splits,
                       cursors);
}

namespace {

__global__ __launch_bounds__(kPartThreads) void k_count_right(const int32_t *__restrict__ rows, const uint16_t *__restrict__ codes,
                                                              const uint32_t *__restrict__ kt, int n_rows, const Chunk *__restrict__ chunks,
                                                              const NodeSplit *__restrict__ splits, int64_t *__restrict__ n_right) {
    const Chunk ck = chunks[blockIdx.x];
    const NodeSplit sp = splits[ck.slot];
    const uint16_t *cbase = codes + (static_cast<size_t>(sp.fslot >> 4) * n_rows) * kCodeGroup + (sp.fslot & (kCodeGroup - 1));
    int c = 0;
    if (!sp.is_cat && kt) {
        const uint32_t *kcol = kt + static_cast<size_t>(sp.fslot) * n_rows;
        for (int p = threadIdx.x; p < ck.len; p += kPartThreads) c += kcol[rows[ck.start + p]] > sp.thr_key ? 1 : 0;
    } else {
        for (int p = threadIdx.x; p < ck.len; p += kPartThreads) {
            const int code = cbase[static_cast<size_t>(rows[ck.start + p]) * kCodeGroup];
            c += (sp.is_cat ? (code == sp.bin) : (code > sp.bin)) ? 1 : 0;
        }
    }
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    __shared__ int wsum[kPartThreads / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot = 0;
        for (int w = 0; w < kPartThreads / kWave; ++w) tot += wsum[w];
        if (tot) atomicAdd(reinterpret_cast<unsigned long long *>(&n_right[ck.slot]), static_cast<unsigned long long>(tot));
    }
}
}  // namespace

void count_right(const int32_t *rows, const uint16_t *codes, const uint32_t *kt, int n_rows, const Chunk *chunks, int n_chunks,
                 const NodeSplit *splits, int64_t *n_right, hipStream_t s) {
    hipLaunchKernelGGL(k_count_right, dim3(n_chunks), dim3(kPartThreads), 0, s, rows, codes, kt, n_rows, chunks, splits, n_right);
}

namespace {

// ------------------------------------------------------------------------------------------------------------
// A11  leaf sums of RAW gradients (fixed-point int64, exact) + counts.  acc[leaf][0..D) sums, acc[leaf][D] count.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_leaf_sums(const float *__restrict__ grads, int D, const int32_t *__restrict__ rows,
                                                   const Chunk *__restrict__ chunks, const StepScales *__restrict__ scp,
                                                   int64_t *__restrict__ acc) {
    extern __shared__ unsigned long long shl[];  // [D+1]
    const double scale = scp->leaf_scale;
    for (int i = threadIdx.x; i <= D; i += blockDim.x) shl[i] = 0ull;
    __syncthreads();
    const Chunk ck = chunks[blockIdx.x];
    // thread <-> (row, d): consecutive threads read consecutive d of one row
    const int per = blockDim.x / D > 0 ? blockDim.x / D : 1;
    const int d = threadIdx.x % D, sub = threadIdx.x / D;
    long long s = 0;
    if (sub < per) {
        // eight independent (row id -> gradient) load chains in flight per thread
        int p = sub;
        for (; p + 7 * per < ck.len; p += 8 * per) {
            int r[8];
            float g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = rows[ck.start + p + u * per];
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] = grads[static_cast<size_t>(r[u]) * D + d];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += __double2ll_rn(static_cast<double>(g[u]) * scale);
        }
        for (; p < ck.len; p += per) {
            const int row = rows[ck.start + p];
            s += __double2ll_rn(static_cast<double>(grads[static_cast<size_t>(row) * D + d]) * scale);
        }
        atomicAdd(&shl[d], static_cast<unsigned long long>(s));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += blockDim.x)
        atomicAdd(reinterpret_cast<unsigned long long *>(&acc[static_cast<size_t>(ck.slot) * (D + 1) + i]), shl[i]);
    if (threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(&acc[static_cast<size_t>(ck.slot) * (D + 1) + D]),
                  static_cast<unsigned long long>(ck.len));
}
}  // namespace

void leaf_sums(const float *grads, int D, const int32_t *rows, const Chunk *chunks, int n_chunks, const StepScales *sc, int64_t *acc,
               hipStream_t s) {
    const int bs = D <= 256 ? 256 : ((D + 63) / 64) * 64;
    hipLaunchKernelGGL(k_leaf_sums, dim3(n_chunks), dim3(bs), (D + 1) * sizeof(unsigned long long), s, grads, D, rows, chunks,
                       sc, acc);
}

}  // namespace kern
}  // namespace gbrl
