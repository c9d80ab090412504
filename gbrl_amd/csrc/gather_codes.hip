// gather_codes.hip -- gfx950 kernels behind the row subsets of a prepared data set (Engine::step_prepared with `rows`, gbrl_hip_dataset_codes).
//
// The class codes of a batch are group-major: [group][row][16] u16 (kern::kCodeGroup), so the 16 codes of one (group, row) pair are ONE
// 32-byte record.  A subset of the rows is a gather of whole records:
//   k_gather_code_records   dst[g][j][0..16) = src[g][rows[j]][0..16).  A record is two lanes, each moving 16 bytes with one
//                           global_load_dwordx4 and one global_store_dwordx4.  The grid is (ceil(2 m / 256), G): blockIdx.y is the group, so
//                           no thread divides by m.  Stores are fully coalesced (lane i writes bytes [16 i, 16 i + 16) of the block's 4 KiB
//                           segment); loads come in aligned 32-byte pairs wherever rows[] points, and in whole 1 KiB runs when rows[] is
//                           ascending (rows = arange(n)).  The index is read once per lane (two lanes share one: the same 4-byte word,
//                           one request).  The kernel moves 64 G m bytes of codes + 4 G m of indices and does nothing else.
//   k_rows_minmax           smallest and largest entry of a DEVICE index vector (wave reduction, then two atomicMin per wave: min v and min ~v), read
//                           back by the host BEFORE anything reads through the vector: an entry outside [0, n) is an argument error, not a fault.
#include "kernels.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

constexpr int kGatherThreads = 256;   // 128 records per block

__global__ __launch_bounds__(kGatherThreads) void k_gather_code_records(const uint4 *__restrict__ src, const int32_t *__restrict__ rows, uint4 *__restrict__ dst,
                                                                        int n, int m) {
    const size_t t = static_cast<size_t>(blockIdx.x) * kGatherThreads + threadIdx.x;   // half-record of this group
    const size_t j = t >> 1;
    if (j >= static_cast<size_t>(m)) return;
    const unsigned half = static_cast<unsigned>(t & 1u);
    const size_t g = blockIdx.y;
    const size_t r = static_cast<size_t>(rows[j]);   // checked against [0, n) by the caller
    const uint4 v = src[((g * static_cast<size_t>(n) + r) << 1) + half];
    dst[((g * static_cast<size_t>(m) + j) << 1) + half] = v;
}

__global__ __launch_bounds__(256) void k_rows_minmax(const int32_t *__restrict__ rows, int m, int32_t *__restrict__ mm /*[2]: min v, min ~v*/) {
    int lo = 0x7fffffff, hi = static_cast<int>(0x80000000u);   // mm holds min(v) and min(~v): both start from one byte pattern (a memset)
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < static_cast<size_t>(m); i += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const int v = rows[i];
        lo = min(lo, v);
        hi = max(hi, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], lo);
        atomicMin(&mm[1], ~hi);
    }
}

}  // namespace

void gather_code_records(const uint16_t *codes, int n, int n_groups, const int32_t *rows, int m, uint16_t *out, hipStream_t s) {
    if (m <= 0 || n_groups <= 0) return;
    const unsigned bx = static_cast<unsigned>((2 * static_cast<size_t>(m) + kGatherThreads - 1) / kGatherThreads);
    // (grid.y <= 65535: more than 2^20 numeric features never reach this point -- the code groups of a data set are F / 16)
    hipLaunchKernelGGL(k_gather_code_records, dim3(bx, static_cast<unsigned>(n_groups)), dim3(kGatherThreads), 0, s, reinterpret_cast<const uint4 *>(codes), rows,
                       reinterpret_cast<uint4 *>(out), n, m);
}

void rows_minmax(const int32_t *rows, int m, int32_t *mm, hipStream_t s) {
    (void)hipMemsetAsync(mm, 0x7f, 2 * sizeof(int32_t), s);   // 0x7f7f7f7f: non-negative, so a negative entry always lowers mm[0]; above ~v of every v, so mm[1] is exact
    const int blocks = std::max(1, std::min(1024, (m + 255) / 256));
    hipLaunchKernelGGL(k_rows_minmax, dim3(blocks), dim3(256), 0, s, rows, m, mm);
}

}  // namespace kern
}  // namespace gbrl
