// step_hist_build.hip -- the split-score histogram build of GBRL::step: the three LDS-atomic kernels (compile-time / run-time D at 16 features
// per block, "wide" at 8, "quad" at 4), the one rule that routes a shape to a kernel, the one launcher, and the diagnostics that show both to the
// tests (hist_plan, hist_selftest).  The stand-alone harnesses
// scripts/hist_bench.hip and scripts/hist_sorted_bench.hip include this file.  (The arithmetic policy of these integer sums: step_score.hip.)
#include "kernels.h"
#include "hooks.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------
// A6  split-score histogram build (THE hot kernel).
// For one chunk of one node's row list and one group of FG features, accumulate per (class, feature):
//   count and the D fixed-point gradient sums, in LDS, with ds_add_u32 atomics.
// LDS layout h[(class*(D+1) + d)*FG + f_local]: the feature index is the fastest dimension, and the 16 lanes that
// share a row hold 16 different features, so the bank of an access is decided by the lane, not by the (random)
// class: a wave-wide atomic touches each bank at most twice (two rows per 32-lane group) -- the 2-way case the LDS
// absorbs for free.  Integer adds wrap mod 2^32; the host picks the fixed-point scale so that every true partial
// sum fits in int32, which makes the wrapped result exact.
// ------------------------------------------------------------------------------------------------------------
constexpr int kHistThreads = 1024;


// Broadcast lane `SRC` of every 16-lane row to the whole row (v_mov_b32_dpp row_newbcast: a VALU move, no LDS traffic).
template <int SRC>
__device__ __forceinline__ int row_bcast(int v) {
    // every lane of the row receives lane SRC's value, so there is no "old" value to keep: mov_dpp leaves the destination
    // untied (update_dpp(0, ...) made the compiler zero 64 registers per loop iteration)
    return __builtin_amdgcn_mov_dpp(v, 0x150 + SRC, 0xf, 0xf, true);
}
template <int DT, int K>
struct RowAtomics {   // adds q[K..DT) of this lane's row into dst, one LDS atomic per output dim
    static __device__ __forceinline__ void run(int32_t *dst, int FG, int myq) {
        atomicAdd(dst + K * FG, row_bcast<K>(myq));
        RowAtomics<DT, K + 1>::run(dst, FG, myq);
    }
};
template <int DT>
struct RowAtomics<DT, DT> {
    static __device__ __forceinline__ void run(int32_t *, int, int) {}
};

// k_hist_build<DT, U>.  DT = compile-time output_dim (1..16) for the FG == 16 layout, or 0 = generic (run-time D, any FG).
// Fast path: the 16 lanes that share a row are one DPP row.  Lane fl < DT loads ONE dword, q[fl], of the row's quantised
// gradients (32 contiguous bytes per row for D = 8) and the D values are handed to all 16 lanes with row_newbcast moves,
// instead of every lane loading all D values (which made the vector-memory path, not the LDS atomics, the bottleneck).
// Every row-slot keeps U rows in flight: all loads of the U rows are issued before the first atomic.
// `Ld`: how a lane fetches its row's class code and gradient word (the product's loads below; the stand-alone harness
// scripts/hist_bench.hip instantiates the kernel with experiment loaders of its own).
struct HistLoads {
    static __device__ __forceinline__ int code(const char *cgroup, uint32_t row, uint32_t coff) {
        return *reinterpret_cast<const uint16_t *>(cgroup + (row * (kCodeGroup * 2u) + coff));
    }
    template <int DT>
    static __device__ __forceinline__ int grad(const char *qbase, uint32_t row, uint32_t qoff) {
        return *reinterpret_cast<const int32_t *>(qbase + (row * static_cast<uint32_t>(DT * 4) + qoff));
    }
};
// COUNT = false (root level, one GPU, radix-selected quantile candidates): the row count of a class is not accumulated -- eight LDS atomics
// per (row, feature) instead of nine at D = 8; kern::hist_reduce fills the count field from the selection's ranks (root_le).
template <int DT, int U, bool PIPE, class Ld = HistLoads, bool COUNT = true>
__global__ __launch_bounds__(kHistThreads) void k_hist_build(const uint16_t *__restrict__ codes, int n_rows,
                                                              const int32_t *__restrict__ qg, int D_rt,
                                                              const int32_t *__restrict__ rows,
                                                              const Chunk *__restrict__ chunks, int n_chunks, int n_groups,
                                                              int FG, int fg_shift, int NB, int32_t *__restrict__ partials,
                                                              HistDirect direct = HistDirect{}) {
    extern __shared__ int32_t h[];
    const int D = DT ? DT : D_rt;
    if (DT) { FG = 16; fg_shift = 4; }
    // XCD-aware block -> (chunk, group) map: the blocks that share a chunk (one per feature group) re-read the same rows'
    // gradients and row ids.  Block b runs on XCD b % 8 (observed; used for speed only), so all groups of a chunk are
    // given ids that are congruent mod 8 and adjacent in launch order: the re-reads are served by that XCD's L2.
    const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
    const int g = jj % n_groups;
    const int chunk_id = (jj / n_groups) * 8 + xcd;
    if (chunk_id >= n_chunks) return;
    const Chunk ck = chunks[chunk_id];
    if (ck.len <= 0 && !direct.hist) return;   // block-uniform: an unused entry of a device-planned chunk table (direct: an empty node's zeros)
    const int n_acc = NB * (D + 1) * FG;
    if ((n_acc & 3) == 0) {   // 16-byte LDS writes (FG = 16: always)
        int4 *h4 = reinterpret_cast<int4 *>(h);
        for (int i = threadIdx.x; i < n_acc / 4; i += kHistThreads) h4[i] = make_int4(0, 0, 0, 0);
    } else {
        for (int i = threadIdx.x; i < n_acc; i += kHistThreads) h[i] = 0;
    }
    __syncthreads();
    const int fl = threadIdx.x & (FG - 1);
    const int slot = threadIdx.x >> fg_shift;
    const int n_slots = kHistThreads >> fg_shift;
    const int row_stride = (D + 1) * FG;
    const int fslot = g * FG + fl;
    const uint16_t *cbase = codes + (static_cast<size_t>(fslot >> 4) * n_rows) * kCodeGroup + (fslot & (kCodeGroup - 1));
    const int32_t *rlist = rows + ck.start;
    const int qlane = fl < (DT ? DT : 1) ? fl : (DT ? DT - 1 : 0);   // lanes >= D re-load the last value (never used)
    // DT path: block-uniform base pointers (SGPR pair) + 32-bit per-lane byte offsets, so that every load carries ONE address
    // VGPR to the memory pipeline instead of two (`global_load v, v_off, s[base]`).  The VGPR -> LDS / TA transfer path is shared
    // with the LDS atomics' address + data (2 clk per source dword per wave-instruction): with 64-bit VGPR addresses the two
    // gathered loads per row cost 8 clk of that path per wave-iteration on top of the 40 clk of the 9 atomics (52.5 measured);
    // the launcher takes this kernel only when n_rows * 64 fits 32 bits.
    const char *cgroup = reinterpret_cast<const char *>(codes + static_cast<size_t>(g) * n_rows * kCodeGroup);   // FG == 16: group g
    const char *qbase = reinterpret_cast<const char *>(qg);
    const uint32_t coff = static_cast<uint32_t>(fl) * 2u, qoff = static_cast<uint32_t>(qlane) * 4u;
    auto ld_code = [&](int row) -> int { return Ld::code(cgroup, static_cast<uint32_t>(row), coff); };
    auto ld_q = [&](int row) -> int { return Ld::template grad<DT>(qbase, static_cast<uint32_t>(row), qoff); };
    int p0 = slot;
    if (DT && PIPE && ck.len > 0) {
        // Software-pipelined main loop (three stages, U rows per slot and stage): while the 9U atomics of iteration i occupy the
        // LDS atomic unit, the codes / gradients of iteration i+1 (their row ids were loaded one iteration earlier) and the row
        // ids of iteration i+2 are already in flight.  Without it every wave of the block (one block per CU) waits for the two
        // dependent global-memory round trips at the same time and the atomic unit idles for a third of the kernel.
        // Prefetch positions beyond the chunk are clamped to its last row (loaded, never accumulated).
        const int last = ck.len - 1, step = n_slots * U;
        int rowB[U], codeA[U], qA[U];
        {
            int rowA[U];
#pragma unroll
            for (int u = 0; u < U; ++u) rowA[u] = rlist[min(p0 + u * n_slots, last)];
#pragma unroll
            for (int u = 0; u < U; ++u) rowB[u] = rlist[min(p0 + step + u * n_slots, last)];
#pragma unroll
            for (int u = 0; u < U; ++u) codeA[u] = ld_code(rowA[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) qA[u] = ld_q(rowA[u]);
        }
        for (; p0 + (U - 1) * n_slots < ck.len; p0 += step) {
            int codeB[U], qB[U], rowC[U];
#pragma unroll
            for (int u = 0; u < U; ++u) codeB[u] = ld_code(rowB[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) qB[u] = ld_q(rowB[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) rowC[u] = rlist[min(p0 + 2 * step + u * n_slots, last)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int32_t *dst = h + codeA[u] * row_stride + fl;
                RowAtomics<DT, 0>::run(dst, 16, qA[u]);
                if (COUNT) atomicAdd(dst + DT * 16, 1);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { codeA[u] = codeB[u]; qA[u] = qB[u]; rowB[u] = rowC[u]; }
        }
    }
    // main loop: U rows per slot, no bounds checks inside => straight-line code: 3U independent loads, then 9U atomics
    for (; p0 + (U - 1) * n_slots < ck.len; p0 += n_slots * U) {
        int row[U], code[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = rlist[p0 + u * n_slots];
        if (DT) {
#pragma unroll
            for (int u = 0; u < U; ++u) code[u] = ld_code(row[u]);
            int myq[U];
#pragma unroll
            for (int u = 0; u < U; ++u) myq[u] = ld_q(row[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int32_t *dst = h + code[u] * row_stride + fl;
                RowAtomics<DT, 0>::run(dst, 16, myq[u]);
                if (COUNT) atomicAdd(dst + DT * 16, 1);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) code[u] = cbase[static_cast<size_t>(row[u]) * kCodeGroup];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t *q = qg + static_cast<size_t>(row[u]) * D;
                int32_t *dst = h + code[u] * row_stride + fl;
                for (int d = 0; d < D; ++d) atomicAdd(dst + d * FG, q[d]);
                atomicAdd(dst + D * FG, 1);
            }
        }
    }
    // tail: one row per slot (p0 is uniform across the 16 lanes of a DPP row, so whole rows take the branch)
    for (; p0 < ck.len; p0 += n_slots) {
        const int row = rlist[p0];
        if (DT) {
            int32_t *dst = h + ld_code(row) * row_stride + fl;
            const int myq = ld_q(row);
            RowAtomics<DT, 0>::run(dst, 16, myq);
            if (COUNT) atomicAdd(dst + DT * 16, 1);
        } else {
            const int code = cbase[static_cast<size_t>(row) * kCodeGroup];
            int32_t *dst = h + code * row_stride + fl;
            const int32_t *q = qg + static_cast<size_t>(row) * D;
            for (int d = 0; d < D; ++d) atomicAdd(dst + d * FG, q[d]);
            atomicAdd(dst + D * FG, 1);
        }
    }
    __syncthreads();
    if (direct.hist) {
        // the node's only chunk: the tile is the node's histogram of this feature group (LDS index = element * FG + feature).
        // FG == 16: 256 threads take 16 elements x 16 features with the ELEMENT as the lane-fastest index, so every 16 lanes store
        // 128 consecutive bytes of one feature (a 4-way LDS bank conflict on the read side, which is the cheaper side).
        const int hslot = direct.slot_map ? direct.slot_map[ck.slot] : ck.slot;
        int64_t *dst = direct.hist + (static_cast<size_t>(hslot) * direct.Fp + static_cast<size_t>(g) * FG) * NB * (D + 1);
        const size_t fstride = static_cast<size_t>(NB) * (D + 1);
        if (FG == 16) {
            const int n_el = NB * (D + 1);
            for (int i = threadIdx.x; i < ((n_el + 15) & ~15) * 16; i += kHistThreads) {
                const int e = (i >> 8) * 16 + (i & 15), f = (i >> 4) & 15;
                if (e < n_el) dst[f * fstride + e] = h[e * 16 + f];
            }
        } else {
            for (int i = threadIdx.x; i < n_acc; i += kHistThreads) dst[(i & (FG - 1)) * fstride + (i >> fg_shift)] = h[i];
        }
        return;
    }
    int32_t *out = partials + (static_cast<size_t>(chunk_id) * n_groups + g) * n_acc;
    if ((n_acc & 3) == 0) {   // the block's 148 KB of partial sums leave in 16-byte pieces
        const int4 *h4 = reinterpret_cast<const int4 *>(h);
        int4 *o4 = reinterpret_cast<int4 *>(out);
        for (int i = threadIdx.x; i < n_acc / 4; i += kHistThreads) o4[i] = h4[i];
    } else {
        for (int i = threadIdx.x; i < n_acc; i += kHistThreads) out[i] = h[i];
    }
}

// k_hist_build_wide<P, H, U>: output dimensions beyond 16, or class counts that leave room for only 8 or 4 features per block
// (FG = 16 / P).  A 16-lane DPP row still works on ONE data row, but on FG features x P parts of the D + 1 fields: lane
// (part p, feature f) adds the fields p*H .. p*H + H - 1 (H = ceil((D + 1) / P) <= 16) of feature f.  Lane l of the row loads the
// P values (field p*H + l, p = 0..P-1; the count's constant 1 sits at field D) once, and step k hands every part ITS lane-k value
// with one row_newbcast move per part, written under that part's bank mask (a DPP bank = 4 lanes) -- P moves per atomic instead of
// D + 1 loads per lane, which is what made the run-time-D path vector-memory bound (3.1 ms per tree at D = 18 against 1.5 ms of
// atomic-unit time).  Same LDS layout [class][field][FG] and the same partials as the generic path.
template <int P, int H, int K, int SRC>
struct WideValue {   // value of step K for this lane's part, assembled from the row's lane K
    static __device__ __forceinline__ int get(const int (&r)[P]) {
        constexpr int bank_mask = P == 2 ? (SRC == 0 ? 0x3 : 0xC) : (1 << SRC);
        const int lower = WideValue<P, H, K, SRC - 1>::get(r);
        return __builtin_amdgcn_update_dpp(lower, r[SRC], 0x150 + K, 0xf, bank_mask, false);
    }
};
template <int P, int H, int K>
struct WideValue<P, H, K, 0> {
    static __device__ __forceinline__ int get(const int (&r)[P]) { return __builtin_amdgcn_mov_dpp(r[0], 0x150 + K, 0xf, 0xf, true); }
};
template <int P, int H, int K>
struct WideAtomics {
    // n_last (uniform): fields owned by the LAST part; every other part owns H.  Steps below n_last need no per-lane test.
    static __device__ __forceinline__ void run(int32_t *dst, int FG, const int (&r)[P], int n_last, bool last_part) {
        const int v = WideValue<P, H, K, P - 1>::get(r);
        if (K < n_last) atomicAdd(dst + K * FG, v);
        else if (!last_part) atomicAdd(dst + K * FG, v);
        WideAtomics<P, H, K + 1>::run(dst, FG, r, n_last, last_part);
    }
};
template <int P, int H>
struct WideAtomics<P, H, H> {
    static __device__ __forceinline__ void run(int32_t *, int, const int (&)[P], int, bool) {}
};

template <int P, int H, int U>
__global__ __launch_bounds__(kHistThreads) void k_hist_build_wide(const uint16_t *__restrict__ codes, int n_rows,
                                                                   const int32_t *__restrict__ qg, int D,
                                                                   const int32_t *__restrict__ rows, const Chunk *__restrict__ chunks,
                                                                   int n_chunks, int n_groups, int NB, int32_t *__restrict__ partials) {
    extern __shared__ int32_t h[];
    constexpr int FG = 16 / P;
    const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
    const int g = jj % n_groups;
    const int chunk_id = (jj / n_groups) * 8 + xcd;
    if (chunk_id >= n_chunks) return;
    const Chunk ck = chunks[chunk_id];
    if (ck.len <= 0) return;   // unused entry of a device-planned chunk table
    const int n_acc = NB * (D + 1) * FG;
    for (int i = threadIdx.x; i < n_acc; i += kHistThreads) h[i] = 0;
    __syncthreads();
    const int fl = threadIdx.x & 15;
    const int part = fl / FG, f = fl & (FG - 1);
    const int slot = threadIdx.x >> 4;
    constexpr int n_slots = kHistThreads >> 4;
    const int row_stride = (D + 1) * FG;
    const int fslot = g * FG + f;
    const uint16_t *cbase = codes + (static_cast<size_t>(fslot >> 4) * n_rows) * kCodeGroup + (fslot & (kCodeGroup - 1));
    const int32_t *rlist = rows + ck.start;
    const int n_last = D + 1 - (P - 1) * H;          // fields the last part owns (1..H); the others own H
    const bool last_part = part == P - 1;
    const int dst_off = f + part * H * FG;
    // what this lane contributes as a SOURCE: field p*H + fl of the row, for every part p
    auto load_fields = [&](int row, int (&r)[P]) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int e = p * H + fl;
            r[p] = (fl < H && e < D) ? qg[static_cast<size_t>(row) * D + e] : (e == D ? 1 : 0);
        }
    };
    int p0 = slot;
    for (; p0 + (U - 1) * n_slots < ck.len; p0 += n_slots * U) {
        int row[U], code[U], r[U][P];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = rlist[p0 + u * n_slots];
#pragma unroll
        for (int u = 0; u < U; ++u) code[u] = cbase[static_cast<size_t>(row[u]) * kCodeGroup];
#pragma unroll
        for (int u = 0; u < U; ++u) load_fields(row[u], r[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) WideAtomics<P, H, 0>::run(h + code[u] * row_stride + dst_off, FG, r[u], n_last, last_part);
    }
    for (; p0 < ck.len; p0 += n_slots) {
        const int row = rlist[p0];
        const int code = cbase[static_cast<size_t>(row) * kCodeGroup];
        int r[P];
        load_fields(row, r);
        WideAtomics<P, H, 0>::run(h + code * row_stride + dst_off, FG, r, n_last, last_part);
    }
    __syncthreads();
    int32_t *out = partials + (static_cast<size_t>(chunk_id) * n_groups + g) * n_acc;
    for (int i = threadIdx.x; i < n_acc; i += kHistThreads) out[i] = h[i];
}

// k_hist_build_quad<R, U>: 4 features per block (FG = 4: many outputs or many classes).  A DPP quad (4 lanes) works on ONE data row:
// lane j owns feature j and loads the fields j, j + 4, j + 8, ... (R = ceil((D + 1) / 4) registers, 16 contiguous bytes per quad and
// register); field e is then handed to the quad from lane e % 4, register e / 4, with ONE quad_perm broadcast per atomic.  (Splitting the
// fields over a 16-lane row as k_hist_build_wide does would need four DPP moves per atomic here, which makes the kernel VALU-bound.)
template <int R, int E>
struct QuadAtomics {   // fields E .. 4R-1
    static __device__ __forceinline__ void run(int32_t *dst, const int (&reg)[R], int D) {
        if (E <= D) {   // uniform
            constexpr int j = E & 3;
            const int v = __builtin_amdgcn_mov_dpp(reg[E >> 2], j * 0x55, 0xf, 0xf, true);   // quad_perm:[j,j,j,j]
            atomicAdd(dst + E * 4, v);
        }
        QuadAtomics<R, E + 1>::run(dst, reg, D);
    }
};
template <int R>
struct QuadAtomics<R, 4 * R> {
    static __device__ __forceinline__ void run(int32_t *, const int (&)[R], int) {}
};

template <int R, int U>
__global__ __launch_bounds__(kHistThreads) void k_hist_build_quad(const uint16_t *__restrict__ codes, int n_rows,
                                                                   const int32_t *__restrict__ qg, int D,
                                                                   const int32_t *__restrict__ rows, const Chunk *__restrict__ chunks,
                                                                   int n_chunks, int n_groups, int NB, int32_t *__restrict__ partials) {
    extern __shared__ int32_t h[];
    const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
    const int g = jj % n_groups;
    const int chunk_id = (jj / n_groups) * 8 + xcd;
    if (chunk_id >= n_chunks) return;
    const Chunk ck = chunks[chunk_id];
    if (ck.len <= 0) return;   // unused entry of a device-planned chunk table
    const int n_acc = NB * (D + 1) * 4;
    for (int i = threadIdx.x; i < n_acc; i += kHistThreads) h[i] = 0;
    __syncthreads();
    const int f = threadIdx.x & 3;
    const int slot = threadIdx.x >> 2;
    constexpr int n_slots = kHistThreads >> 2;
    const int row_stride = (D + 1) * 4;
    const int fslot = g * 4 + f;
    const uint16_t *cbase = codes + (static_cast<size_t>(fslot >> 4) * n_rows) * kCodeGroup + (fslot & (kCodeGroup - 1));
    const int32_t *rlist = rows + ck.start;
    auto load_fields = [&](int row, int (&reg)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = r * 4 + f;
            reg[r] = e < D ? qg[static_cast<size_t>(row) * D + e] : (e == D ? 1 : 0);
        }
    };
    int p0 = slot;
    for (; p0 + (U - 1) * n_slots < ck.len; p0 += n_slots * U) {
        int row[U], code[U], reg[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = rlist[p0 + u * n_slots];
#pragma unroll
        for (int u = 0; u < U; ++u) code[u] = cbase[static_cast<size_t>(row[u]) * kCodeGroup];
#pragma unroll
        for (int u = 0; u < U; ++u) load_fields(row[u], reg[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) QuadAtomics<R, 0>::run(h + code[u] * row_stride + f, reg[u], D);
    }
    for (; p0 < ck.len; p0 += n_slots) {
        const int row = rlist[p0];
        const int code = cbase[static_cast<size_t>(row) * kCodeGroup];
        int reg[R];
        load_fields(row, reg);
        QuadAtomics<R, 0>::run(h + code * row_stride + f, reg, D);
    }
    __syncthreads();
    int32_t *out = partials + (static_cast<size_t>(chunk_id) * n_groups + g) * n_acc;
    for (int i = threadIdx.x; i < n_acc; i += kHistThreads) out[i] = h[i];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ route and launch

size_t hist_lds_bytes(int NB, int D, int FG) { return static_cast<size_t>(NB) * (D + 1) * FG * sizeof(int32_t); }

namespace {

#ifndef GBRL_HIST_U
#define GBRL_HIST_U 8
#endif

// Which kernel a (D, FG, n_rows) shape gets, and what that kernel can do.  hist_build, hist_direct_supported and hist_countless_supported all
// answer from this one function, so the engine's questions and the launch cannot disagree.
struct HistRoute {
    enum Kind { GENERIC, FIXED_D, WIDE, QUAD } kind;
    int param;           // FIXED_D: D (1..16);  WIDE: H = ceil((D + 1) / 2) (1..16);  QUAD: R = ceil((D + 1) / 4) (1..16)
    bool pipe;           // FIXED_D only: the software-pipelined main loop (measurement hook GBRL_HIP_HIST_PIPE=0 takes it out)
    bool direct_ok;      // the tile can leave as the node's histogram (HistDirect).  By FG alone, whatever the kernel: FG 8 / 4 MAY go to the
                         // wide / quad kernels, which only write partials -- and skip empty chunks
    bool countless_ok;   // a COUNT = false variant exists: the compile-time-D kernels with the software pipeline
};
HistRoute hist_route(int D, int FG, int n_rows) {
    const bool generic_only = hooks::on(hooks::HIST_GENERIC);   // test hook
    const char *e = hooks::raw(hooks::HIST_PIPE);
    const bool pipe = !(e && e[0] == '0');
    HistRoute r{HistRoute::GENERIC, 0, false, FG != 8 && FG != 4, false};
    // the compile-time-D kernels address codes and gradients with 32-bit byte offsets from block-uniform bases (64 bytes per row at D = 16)
    if (generic_only || n_rows > (1 << 26)) return r;
    if (FG == 16 && D >= 1 && D <= 16) {
        r.kind = HistRoute::FIXED_D; r.param = D; r.pipe = pipe; r.countless_ok = pipe;
    } else if (FG == 8 && D + 1 <= 32) {   // the fields of a row are split over the two halves of the 16-lane DPP row (k_hist_build_wide<2, H>)
        r.kind = HistRoute::WIDE; r.param = (D + 2) / 2;
    } else if (FG == 4 && D + 1 <= 64) {   // one DPP quad per data row (k_hist_build_quad)
        r.kind = HistRoute::QUAD; r.param = (D + 4) / 4;
    }
    return r;
}

// One launch's arguments, built once in hist_build: everything a build kernel takes.  codes .. n_groups are the first eight parameters of every
// build kernel, in order; k_hist_build takes (FG, fg_shift, NB, partials, direct) behind them, the wide and quad kernels (NB, partials).
struct HistArgs {
    const uint16_t *codes; int n_rows; const int32_t *qg; int D; const int32_t *rows; const Chunk *chunks; int n_chunks, n_groups, FG, fg_shift, NB;
    int32_t *partials; HistDirect direct; size_t lds; hipStream_t s;
    hipEvent_t ev_start, ev_stop;   // (nullable) the dispatch's own begin / end timestamps -- no extra packets in the stream, unlike hipEventRecord around the launch
};
template <auto Kernel>
void launch_hist(const HistArgs &a) {
    static PerDeviceOnce attr_set;   // one per kernel instantiation
    if (attr_set.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const dim3 grid(8 * a.n_groups * ((a.n_chunks + 7) / 8)), block(kHistThreads);
    if constexpr (std::is_invocable_v<decltype(Kernel), const uint16_t *, int, const int32_t *, int, const int32_t *, const Chunk *, int, int, int, int, int,
                                      int32_t *, HistDirect>)   // k_hist_build
        hipExtLaunchKernelGGL(Kernel, grid, block, a.lds, a.s, a.ev_start, a.ev_stop, 0, a.codes, a.n_rows, a.qg, a.D, a.rows, a.chunks, a.n_chunks, a.n_groups,
                              a.FG, a.fg_shift, a.NB, a.partials, a.direct);
    else
        hipExtLaunchKernelGGL(Kernel, grid, block, a.lds, a.s, a.ev_start, a.ev_stop, 0, a.codes, a.n_rows, a.qg, a.D, a.rows, a.chunks, a.n_chunks, a.n_groups,
                              a.NB, a.partials);
}

// f(std::integral_constant<int, v>{}) for a run-time v in [Lo, Hi]; false, and no call, outside it
template <int Lo, class F, int... I>
bool dispatch_int(int v, F &&f, std::integer_sequence<int, I...>) {
    return ((v == Lo + I ? (f(std::integral_constant<int, Lo + I>{}), true) : false) || ...);
}
template <int Lo, int Hi, class F>
bool dispatch_int(int v, F &&f) { return dispatch_int<Lo>(v, f, std::make_integer_sequence<int, Hi - Lo + 1>{}); }

}  // namespace

bool hist_direct_supported(int FG) { return hist_route(1, FG, 1).direct_ok; }   // (by FG alone)
bool hist_countless_supported(int D, int FG, int n_rows) { return hist_route(D, FG, n_rows).countless_ok; }

int hist_feature_group(int NB, int D) {
    int FG = 16;
    while (FG > 1 && hist_lds_bytes(NB, D, FG) > kHistLdsLimit) FG >>= 1;
    // more than 16 outputs: k_hist_build_wide spreads the D + 1 fields of a row over the 16 / FG parts of a 16-lane row (<= 16 each)
    while (D > 16 && FG > 4 && (16 / FG) * 16 < D + 1) FG >>= 1;
    return FG;
}

HistPlan hist_plan(int D, int FG, int n_rows) {
    const HistRoute r = hist_route(D, FG, n_rows);
    return HistPlan{static_cast<int>(r.kind), r.param, r.pipe, r.direct_ok, r.countless_ok};
}

namespace {

// What launch_route launched: the route of the kernel that ran (the one asked for, unless its parameter lies outside the instantiations) with
// `pipe` = the PIPE form ran, and whether the kernel accumulates the count field (COUNT).
struct HistLaunched { HistRoute route; bool counted; };
HistLaunched launch_route(const HistArgs &a, const HistRoute &r, bool count_rows) {
    switch (r.kind) {
    case HistRoute::FIXED_D: {
        bool pipe = false, counted = true;
        if (dispatch_int<1, 16>(r.param, [&](auto c) {
                constexpr int DD = decltype(c)::value;
                if (r.pipe && !count_rows) { launch_hist<k_hist_build<DD, GBRL_HIST_U, true, HistLoads, false>>(a); pipe = true; counted = false; }
                else if (r.pipe) { launch_hist<k_hist_build<DD, GBRL_HIST_U, true>>(a); pipe = true; }
                else launch_hist<k_hist_build<DD, GBRL_HIST_U, false>>(a);
            })) {
            HistRoute ran = r;
            ran.pipe = pipe;
            return {ran, counted};
        }
        break;
    }
    case HistRoute::WIDE:
        if (dispatch_int<1, 16>(r.param, [&](auto c) { launch_hist<k_hist_build_wide<2, decltype(c)::value, 4>>(a); })) return {r, true};
        break;
    case HistRoute::QUAD:
        if (dispatch_int<1, 16>(r.param, [&](auto c) {
                constexpr int R = decltype(c)::value;
                launch_hist<k_hist_build_quad<R, (R <= 8 ? 4 : 2)>>(a);
            })) return {r, true};
        break;
    case HistRoute::GENERIC:
        break;
    }
    // the run-time-D kernel: the generic route, and the way out should a route's parameter ever lie outside its kernel's instantiations
    launch_hist<k_hist_build<0, 4, false>>(a);
    return {HistRoute{HistRoute::GENERIC, 0, false, r.direct_ok, false}, true};
}

HistLaunched hist_build_routed(const uint16_t *codes, int n_rows, const int32_t *qg, int D, const int32_t *rows, const Chunk *chunks,
                            int n_chunks, int n_groups, int FG, int NB, int32_t *partials, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop,
                            const HistDirect *direct, bool count_rows, bool *direct_out) {
    int shift = 0;
    while ((1 << shift) < FG) ++shift;
    const HistArgs a{codes, n_rows, qg, D, rows, chunks, n_chunks, n_groups, FG, shift, NB, partials, direct ? *direct : HistDirect{}, hist_lds_bytes(NB, D, FG),
                     s, ev_start, ev_stop};
    const HistLaunched ran = launch_route(a, hist_route(D, FG, n_rows), count_rows);
    // k_hist_build answers a HistDirect; the wide and quad kernels only write partials
    *direct_out = a.direct.hist != nullptr && (ran.route.kind == HistRoute::FIXED_D || ran.route.kind == HistRoute::GENERIC);
    return ran;
}

}  // namespace

bool hist_build(const uint16_t *codes, int n_rows, const int32_t *qg, int D, const int32_t *rows, const Chunk *chunks,
                int n_chunks, int n_groups, int FG, int NB, int32_t *partials, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop,
                const HistDirect *direct, bool count_rows) {
    bool direct_out = false;
    (void)hist_build_routed(codes, n_rows, qg, D, rows, chunks, n_chunks, n_groups, FG, NB, partials, s, ev_start, ev_stop, direct, count_rows, &direct_out);
    return direct_out;
}

// ------------------------------------------------------------------------------------------------------------ diagnostics

// gbrl_hip_hist_probe: host arrays in, the int64 histograms out -- one hist_build, and hist_reduce behind it unless the build stored the histograms
// itself.  The caller's `hist` goes to the device first and comes back afterwards, so a cell no kernel stored keeps the caller's value; the partials
// start from a non-zero pattern, so a partial that the reduce reads and no block wrote shows.  Every index a kernel will form is checked here first.
int hist_selftest(HistProbe &p, const char **why) {
    const auto refuse = [&](const char *text) { *why = text; return static_cast<int>(kHistProbeInvalid); };
    *why = "";
    if (!p.codes || !p.qg || !p.hist || (p.m > 0 && !p.rows) || (p.n_chunks > 0 && !p.chunks)) return refuse("hist_probe: null array");
    if (p.n_rows < 1 || p.n_rows > (1 << 26) || p.D < 1 || p.D > 512 || p.m < 0 || p.m > (1 << 24) || p.n_chunks < 0 || p.n_chunks > (1 << 16) || p.n_nodes < 1 ||
        p.n_nodes > 65535 /* hist_reduce: one grid z per node */ || p.n_fslots < 1 || p.n_fslots > 4096 || p.NB < 1 || p.NB > 65535 || p.chunks_per_slot < 1 || p.scatter_fs < 0)
        return refuse("hist_probe: a size is out of range");
    const int FG = p.FG, NB = p.NB, D = p.D;
    if (FG != 1 && FG != 2 && FG != 4 && FG != 8 && FG != 16) return refuse("hist_probe: FG must be 1, 2, 4, 8 or 16");
    if (hist_lds_bytes(NB, D, FG) > kHistLdsLimit) return refuse("hist_probe: (classes per feature) x (output_dim + 1) x FG does not fit the LDS");
    if (p.mode != 0 && p.mode != 1) return refuse("hist_probe: mode must be 0 or 1");
    const HistRoute route = hist_route(D, FG, p.n_rows);
    const int Fp = ((p.n_fslots + FG - 1) / FG) * FG, n_groups = Fp / FG;
    const size_t feat = static_cast<size_t>(NB) * (D + 1), n_acc = feat * FG;
    const size_t n_codes = static_cast<size_t>((Fp + kCodeGroup - 1) / kCodeGroup) * p.n_rows * kCodeGroup;
    if (n_codes > (size_t{1} << 28) || static_cast<size_t>(p.n_rows) * D > (size_t{1} << 28)) return refuse("hist_probe: a size is out of range");
    for (size_t i = 0; i < n_codes; ++i)
        if (p.codes[i] >= NB) return refuse("hist_probe: a class code is not below n_classes");
    for (int i = 0; i < p.m; ++i)
        if (p.rows[i] < 0 || p.rows[i] >= p.n_rows) return refuse("hist_probe: a row index is outside [0, n_rows)");
    // chunk table: the entries with rows first, slots ascending; behind them only len = 0 entries (what the device planner leaves)
    int n_real = 0;
    for (int i = 0; i < p.n_chunks; ++i) {
        const int32_t slot = p.chunks[3 * i], start = p.chunks[3 * i + 1], len = p.chunks[3 * i + 2];
        if (slot < 0 || slot >= p.n_nodes || start < 0 || len < 0 || start > p.m || len > p.m - start) return refuse("hist_probe: a chunk lies outside the row list or the nodes");
        if (len > 0) n_real = i + 1;
    }
    for (int i = 1; i < n_real; ++i)
        if (p.chunks[3 * i] < p.chunks[3 * (i - 1)]) return refuse("hist_probe: chunk slots must ascend");
    if (p.mode == 1) {
        if (!route.direct_ok) return refuse("hist_probe: this FG has no direct store");
        if (p.n_chunks != p.n_nodes) return refuse("hist_probe: the direct store needs every node to be one chunk");
        for (int i = 0; i < p.n_chunks; ++i)
            if (p.chunks[3 * i] != i) return refuse("hist_probe: the direct store needs every node to be one chunk");
        if (p.scatter_fs > 0 || p.root_le || !p.count_rows) return refuse("hist_probe: the direct store has no scatter layout and no root counts");
    } else {
        for (int i = 0; i < n_real; ++i)
            if (p.chunks[3 * i + 2] == 0) return refuse("hist_probe: an empty chunk in front of a chunk with rows (a node without rows has no chunk)");
    }
    if ((!p.count_rows || p.root_le) && !route.countless_ok) return refuse("hist_probe: this shape has no count-less build");
    if (p.root_le && (p.root_F < 0 || p.root_F > Fp || p.root_B < 1 || p.root_B > 65534 || p.root_n < 0)) return refuse("hist_probe: root_le sizes out of range");
    // the histogram buffer: node slots [n_hist_slots][Fp][class][D+1], or the scatter layout [ceil(Fp / fs)][n_nodes][fs][class][D+1]
    if (p.hist_elems < 1) return refuse("hist_probe: hist_elems does not match the layout");
    if (p.scatter_fs > 0) {
        const size_t want = static_cast<size_t>((Fp + p.scatter_fs - 1) / p.scatter_fs) * p.n_nodes * p.scatter_fs * feat;
        if (static_cast<size_t>(p.hist_elems) != want) return refuse("hist_probe: hist_elems does not match the layout");
    } else if (static_cast<size_t>(p.hist_elems) % (Fp * feat) != 0) {
        return refuse("hist_probe: hist_elems does not match the layout");
    }
    const size_t n_hist_slots = p.scatter_fs > 0 ? static_cast<size_t>(p.n_nodes) : static_cast<size_t>(p.hist_elems) / (Fp * feat);
    if (p.slot_map) {
        std::vector<char> seen(n_hist_slots, 0);
        for (int k = 0; k < p.n_nodes; ++k) {
            const int32_t t = p.slot_map[k];
            if (t < 0 || static_cast<size_t>(t) >= n_hist_slots || seen[t]) return refuse("hist_probe: slot_map must name distinct histogram slots");
            seen[t] = 1;
        }
    } else if (n_hist_slots < static_cast<size_t>(p.n_nodes)) {
        return refuse("hist_probe: hist_elems does not match the layout");
    }
    const size_t n_part = static_cast<size_t>(std::max(1, p.n_chunks)) * n_groups * n_acc;
    if (n_part > (size_t{1} << 29) || static_cast<size_t>(p.hist_elems) > (size_t{1} << 28)) return refuse("hist_probe: a size is out of range");

    // ---- device half
    std::vector<Chunk> ck(std::max(1, p.n_chunks), Chunk{0, 0, 0, 0});
    for (int i = 0; i < p.n_chunks; ++i) ck[i] = Chunk{p.chunks[3 * i], p.chunks[3 * i + 1], p.chunks[3 * i + 2], 0};
    std::vector<int32_t> begin(p.n_nodes + 1, 0);   // begin[k] = entries with rows whose slot is below k
    for (int i = 0; i < n_real; ++i) ++begin[ck[i].slot + 1];
    for (int k = 0; k < p.n_nodes; ++k) begin[k + 1] += begin[k];
    struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } };
    Dev dcodes, dqg, drows, dck, dbegin, dle, dmap, dhist, dpart;
    const auto up = [](Dev &d, const void *src, size_t bytes) {
        if (hipMalloc(&d.p, std::max<size_t>(16, bytes)) != hipSuccess) { (void)hipGetLastError(); return false; }
        return bytes == 0 || hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(dcodes, p.codes, n_codes * sizeof(uint16_t)) || !up(dqg, p.qg, sizeof(int32_t) * p.n_rows * D) || !up(drows, p.rows, sizeof(int32_t) * p.m) ||
        !up(dck, ck.data(), sizeof(Chunk) * ck.size()) || !up(dbegin, begin.data(), sizeof(int32_t) * begin.size()) ||
        !up(dhist, p.hist, sizeof(int64_t) * p.hist_elems) || (p.root_le && !up(dle, p.root_le, sizeof(uint32_t) * p.root_F * p.root_B)) ||
        (p.slot_map && !up(dmap, p.slot_map, sizeof(int32_t) * p.n_nodes)))
        return kHistProbeDevice;
    if (hipMalloc(&dpart.p, n_part * sizeof(int32_t)) != hipSuccess || hipMemset(dpart.p, 0x5b, n_part * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return kHistProbeDevice; }
    HistDirect hd;
    hd.hist = static_cast<int64_t *>(dhist.p); hd.slot_map = static_cast<const int32_t *>(dmap.p); hd.Fp = Fp;
    bool wrote = false;
    HistLaunched ran{route, p.count_rows != 0 || !route.pipe};   // (no chunk, no launch: what a launch would take)
    if (p.n_chunks > 0)
        ran = hist_build_routed(static_cast<const uint16_t *>(dcodes.p), p.n_rows, static_cast<const int32_t *>(dqg.p), D, static_cast<const int32_t *>(drows.p),
                                static_cast<const Chunk *>(dck.p), p.n_chunks, n_groups, FG, NB, static_cast<int32_t *>(dpart.p), nullptr, nullptr, nullptr,
                                p.mode == 1 ? &hd : nullptr, p.count_rows != 0, &wrote);
    if (hipGetLastError() != hipSuccess /* a refused launch */ || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return kHistProbeDevice; }
    if (!wrote) {
        hist_reduce(static_cast<const int32_t *>(dpart.p), static_cast<const int32_t *>(dbegin.p), static_cast<const int32_t *>(dmap.p), p.n_nodes, n_groups, FG, NB, D, Fp,
                    static_cast<int64_t *>(dhist.p), nullptr, p.chunks_per_slot, p.scatter_fs, static_cast<const uint32_t *>(dle.p), p.root_F, p.root_B, p.root_n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return kHistProbeDevice; }
    }
    if (hipMemcpy(p.hist, dhist.p, sizeof(int64_t) * p.hist_elems, hipMemcpyDeviceToHost) != hipSuccess) return kHistProbeDevice;
    p.kind = static_cast<int>(ran.route.kind); p.param = ran.route.param; p.pipe = ran.route.pipe ? 1 : 0; p.counted = ran.counted ? 1 : 0; p.direct = wrote ? 1 : 0;
    return kHistProbeOk;
}

}  // namespace kern
}  // namespace gbrl
