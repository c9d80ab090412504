// step_partition.hip -- the row side of a tree level: partition of every splitting node's rows into its children, the count of rows a split
// sends right (row-sharded levels), and the exact leaf sums of the raw gradients.
#include "kernels.h"
#include "kernels_common.h"
#include "../../include/gbrl_hip.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

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
    if (D > static_cast<int>(blockDim.x)) {
        // more fields than threads (257 .. 512 outputs): thread t owns fields t, t + 256, .. of every row of the chunk -- the kernel is bounded at
        // 256 threads, a block of D rounded up to a wave cannot be launched on it
        for (int dd = threadIdx.x; dd < D; dd += blockDim.x) {
            long long t = 0;
            for (int p = 0; p < ck.len; ++p) t += __double2ll_rn(static_cast<double>(grads[static_cast<size_t>(rows[ck.start + p]) * D + dd]) * scale);
            shl[dd] = static_cast<unsigned long long>(t);
        }
    } else if (sub < per) {
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
    hipLaunchKernelGGL(k_leaf_sums, dim3(n_chunks), dim3(256), (D + 1) * sizeof(unsigned long long), s, grads, D, rows, chunks,
                       sc, acc);
}

// ------------------------------------------------------------------------------------------------------------ diagnostics

// gbrl_hip_rows_probe: one partition_rows, count_right or leaf_sums on host arrays.  The outputs go to the device holding the caller's values and
// come back afterwards.  Every index a kernel will form is checked here first; for the partition that includes the destinations, so the host
// counts every splitting node's left rows itself.
int rows_selftest(::gbrl_hip_rows_probe_t &p, const char **why) {
    const auto refuse = [&](const char *text) { *why = text; return static_cast<int>(kHistProbeInvalid); };
    *why = "";
    if (p.op < 0 || p.op > 2) return refuse("rows_probe: op must be 0, 1 or 2");
    const bool split_op = p.op != 2;
    if (p.n_rows < 1 || p.n_rows > (1 << 26) || p.m < 1 || p.m > (1 << 24) || p.n_chunks < 1 || p.n_chunks > (1 << 16) || p.n_slots < 1 || p.n_slots > (1 << 16) ||
        (split_op && (p.n_feature_slots < 1 || p.n_feature_slots > 4096)) || (!split_op && (p.output_dim < 1 || p.output_dim > 512 || p.lbits < 0 || p.lbits > 40)))
        return refuse("rows_probe: a size is out of range");
    if (!p.rows || !p.chunks || (split_op && (!p.codes || !p.splits)) || (p.op == 0 && (!p.rows_out || !p.cursors)) || (p.op != 0 && !p.acc) || (p.op == 2 && !p.grads))
        return refuse("rows_probe: null array");
    const int D = p.output_dim, n_rows = p.n_rows;
    const size_t n_codes = split_op ? static_cast<size_t>((p.n_feature_slots + kCodeGroup - 1) / kCodeGroup) * n_rows * kCodeGroup : 0;
    if (n_codes > (size_t{1} << 28) || (p.kt && static_cast<size_t>(p.n_feature_slots) * n_rows > (size_t{1} << 28)) || (!split_op && static_cast<size_t>(n_rows) * D > (size_t{1} << 28)))
        return refuse("rows_probe: a size is out of range");
    for (int i = 0; i < p.m; ++i)
        if (p.rows[i] < 0 || p.rows[i] >= n_rows) return refuse("rows_probe: a row index is outside [0, n_rows)");
    for (int i = 0; i < p.n_chunks; ++i) {
        const int32_t slot = p.chunks[3 * i], start = p.chunks[3 * i + 1], len = p.chunks[3 * i + 2];
        if (slot < 0 || slot >= p.n_slots || start < 0 || len < 0 || start > p.m || len > p.m - start) return refuse("rows_probe: a chunk lies outside the row list or the slots");
        if (p.op == 0 && len > kPartRows) return refuse("rows_probe: a partition chunk holds more than 4096 rows");
    }
    const NodeSplit *sp = reinterpret_cast<const NodeSplit *>(p.splits);
    const auto goes_right = [&](const NodeSplit &q, int row) {
        if (!q.is_cat && p.kt) return p.kt[static_cast<size_t>(q.fslot) * n_rows + row] > q.thr_key;
        const int code = p.codes[(static_cast<size_t>(q.fslot >> 4) * n_rows + row) * kCodeGroup + (q.fslot & (kCodeGroup - 1))];
        return q.is_cat ? code == q.bin : code > q.bin;
    };
    if (split_op)
        for (int k = 0; k < p.n_slots; ++k)
            if (sp[k].fslot < 0 || sp[k].fslot >= p.n_feature_slots) return refuse("rows_probe: a split names a feature slot outside the codes");
    if (p.op == 0) {
        std::vector<long long> total(p.n_slots, 0), left(p.n_slots, 0);
        for (int i = 0; i < p.n_chunks; ++i) {
            const int32_t slot = p.chunks[3 * i], start = p.chunks[3 * i + 1], len = p.chunks[3 * i + 2];
            if (!sp[slot].do_split) continue;
            total[slot] += len;
            for (int q = 0; q < len; ++q) left[slot] += goes_right(sp[slot], p.rows[start + q]) ? 0 : 1;
        }
        std::vector<std::pair<long long, long long>> segs;
        for (int k = 0; k < p.n_slots; ++k) {
            if (!sp[k].do_split || total[k] == 0) continue;
            if (sp[k].seg_start < 0 || sp[k].seg_start > p.m || total[k] > p.m - sp[k].seg_start) return refuse("rows_probe: a segment lies outside the row list");
            if (sp[k].n_left != left[k]) return refuse("rows_probe: n_left is not the number of rows the split sends left");
            if (p.cursors[2 * k] != 0 || p.cursors[2 * k + 1] != 0) return refuse("rows_probe: the cursors of a splitting node must start at 0");
            segs.emplace_back(sp[k].seg_start, sp[k].seg_start + total[k]);
        }
        std::sort(segs.begin(), segs.end());
        for (size_t i = 1; i < segs.size(); ++i)
            if (segs[i].first < segs[i - 1].second) return refuse("rows_probe: the segments of two splitting nodes overlap");
    }

    // ---- device half
    struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } };
    const auto up = [](Dev &d, const void *src, size_t bytes) {
        if (hipMalloc(&d.p, std::max<size_t>(16, bytes)) != hipSuccess) { (void)hipGetLastError(); return false; }
        return bytes == 0 || hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    std::vector<Chunk> ck(p.n_chunks);
    for (int i = 0; i < p.n_chunks; ++i) ck[i] = Chunk{p.chunks[3 * i], p.chunks[3 * i + 1], p.chunks[3 * i + 2], 0};
    StepScales sc{};
    sc.inv_scale = 1.0; sc.leaf_scale = std::ldexp(1.0, p.lbits); sc.scale = 1.0f; sc.lbits = p.lbits;
    const size_t acc_bytes = p.op == 1 ? 8 * static_cast<size_t>(p.n_slots) : (p.op == 2 ? 8 * static_cast<size_t>(p.n_slots) * (D + 1) : 0);
    Dev drows, dck, dcodes, dkt, dsp, dgr, dout, dcur, dacc, dsc;
    bool ok = up(drows, p.rows, 4 * static_cast<size_t>(p.m)) && up(dck, ck.data(), sizeof(Chunk) * ck.size()) && up(dsc, &sc, sizeof(sc));
    if (ok && split_op) ok = up(dcodes, p.codes, 2 * n_codes) && up(dsp, p.splits, sizeof(NodeSplit) * p.n_slots) && (!p.kt || up(dkt, p.kt, 4 * static_cast<size_t>(p.n_feature_slots) * n_rows));
    if (ok && p.op == 0) ok = up(dout, p.rows_out, 4 * static_cast<size_t>(p.m)) && up(dcur, p.cursors, 8 * static_cast<size_t>(p.n_slots));
    if (ok && p.op != 0) ok = up(dacc, p.acc, acc_bytes);
    if (ok && p.op == 2) ok = up(dgr, p.grads, 4 * static_cast<size_t>(n_rows) * D);
    if (!ok) return kHistProbeDevice;
    if (p.op == 0)
        partition_rows(static_cast<const int32_t *>(drows.p), static_cast<int32_t *>(dout.p), static_cast<const uint16_t *>(dcodes.p), static_cast<const uint32_t *>(dkt.p), n_rows,
                       static_cast<const Chunk *>(dck.p), p.n_chunks, static_cast<const NodeSplit *>(dsp.p), static_cast<int32_t *>(dcur.p), nullptr);
    else if (p.op == 1)
        count_right(static_cast<const int32_t *>(drows.p), static_cast<const uint16_t *>(dcodes.p), static_cast<const uint32_t *>(dkt.p), n_rows, static_cast<const Chunk *>(dck.p), p.n_chunks,
                    static_cast<const NodeSplit *>(dsp.p), static_cast<int64_t *>(dacc.p), nullptr);
    else
        leaf_sums(static_cast<const float *>(dgr.p), D, static_cast<const int32_t *>(drows.p), static_cast<const Chunk *>(dck.p), p.n_chunks, static_cast<const StepScales *>(dsc.p),
                  static_cast<int64_t *>(dacc.p), nullptr);
    if (hipGetLastError() != hipSuccess /* a refused launch */ || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return kHistProbeDevice; }
    if (p.op == 0) ok = hipMemcpy(p.rows_out, dout.p, 4 * static_cast<size_t>(p.m), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(p.cursors, dcur.p, 8 * static_cast<size_t>(p.n_slots), hipMemcpyDeviceToHost) == hipSuccess;
    else ok = hipMemcpy(p.acc, dacc.p, acc_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? kHistProbeOk : kHistProbeDevice;
}

}  // namespace kern
}  // namespace gbrl
