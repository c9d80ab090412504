// cat_rank.hip -- the ranking statistics of a batch with more distinct categorical cells than candidates are kept (A5, overflow case).
//
// The reference then keeps the Fc * n_bins categories with the largest MEAN gradient norm (split_candidate_generator.cpp:117-163):
//     unique_cats[cat].total_grad_norm += grad_norms[sample_idx];   unique_cats[cat].cat_count += 1;
// i.e. per distinct (feature, cell) pair q a count and a float32 total summed in ascending row order from 0.0f.  The ranking compares the
// float32 means total / float(count), and which of several equal means survives depends on std::sort seeing exactly these values, so the
// totals here equal that serial loop BIT FOR BIT:
//   (a) k_rank_norms   : norm[i] = fma chain over the raw gradients of row i (calculate_squared_norm, math_ops.cpp:726-749, contracted)
//   (b) k_rank_keys    : list index q of every cell through the scan's own hash tables (categorical.hip) + count[q]
//   (c) radix_sort_pass: stable LSD radix sort (8-bit digits, radix_sort.hip) of the cells by q.  The cells start in (row, feature) order and one q belongs
//                        to one feature, so after a STABLE sort the rows of a category are contiguous and ascending
//   (d) k_rank_short   : one thread per category adds its rows' norms one by one; categories with more than kRankLong rows go through
//                        kern::seq_sums (seqsum.hip), which evaluates a sequential float32 sum in parallel, bit for bit
// Nothing here reads a value the host has to provide beyond sizes: the whole sequence is enqueued in one go.
#include "kernels.h"
#include "kernels_common.h"
#include "cat_hash.h"

#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace gbrl {
namespace kern {

namespace {

constexpr int kRankLong = 1024;           // rows of one category above which its chain goes through seq_sums
constexpr int kRadixTile = kRadixSortTile;   // (radix_sort.hip: the elements one block of a sort pass owns)
constexpr int kRankMaxProbes = 512;       // (kCatMaxProbes of categorical.hip: the probe that inserted a cell finds it again)

__device__ __forceinline__ uint64_t rank_cell_hash(const char *cell) {
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(cell);
    uint64_t w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) { const ulonglong2 v = src[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
    return cat_cell_hash_raw(w);
}

__global__ __launch_bounds__(256) void k_rank_norms(const float *__restrict__ g, int n, int D, float *__restrict__ norm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = g + static_cast<size_t>(i) * D;
    float acc = 0.0f;
    for (int d = 0; d < D; ++d) { const float v = r[d]; acc = fmaf(v, v, acc); }
    norm[i] = acc;
}

// list index of every live table slot (k_cat_publish writes the same values, but only for the records it publishes)
__global__ __launch_bounds__(256) void k_rank_slotq(const int32_t *__restrict__ meta, const int32_t *__restrict__ list_slot, int n_q,
                                                    int32_t *__restrict__ slot_q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < min(meta[2], n_q)) slot_q[list_slot[i]] = i;
}

__global__ __launch_bounds__(256) void k_rank_keys(const char *__restrict__ cells, uint32_t n_cells, int Fc,
                                                   const unsigned long long *__restrict__ keys, const int32_t *__restrict__ slot_q, int log2_cap,
                                                   int n_q, uint32_t *__restrict__ qkey, uint32_t *__restrict__ rowv, int32_t *__restrict__ count,
                                                   int32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cells) return;
    const int f = static_cast<int>(i % Fc);
    const uint64_t h = rank_cell_hash(cells + static_cast<size_t>(i) * 128);
    const uint32_t mask = (1u << log2_cap) - 1u;
    uint32_t slot = static_cast<uint32_t>(h >> 20) & mask;
    const size_t base = static_cast<size_t>(f) << log2_cap;
    int q = -1;
    for (int p = 0; p < kRankMaxProbes; ++p) {
        const unsigned long long k = keys[base + slot];
        if (k == h) { q = slot_q[base + slot]; break; }
        if (k == 0ull) break;
        slot = (slot + 1) & mask;
    }
    if (q < 0 || q >= n_q) { flags[0] = 1; q = 0; }   // (cannot happen after a scan without overflow: reported like one)
    else atomicAdd(&count[q], 1);
    qkey[i] = static_cast<uint32_t>(q);
    rowv[i] = i / static_cast<uint32_t>(Fc);
}

// the sorted cells: first position of every category, the norms in sorted order, and the categories whose chain is long.  A long
// category covers more than kRankLong positions, so no two of them start in the same kRankLong-slot: long_slot is an ordered list
// with holes, without atomics
__global__ __launch_bounds__(256) void k_rank_bounds(const uint32_t *__restrict__ qs, const uint32_t *__restrict__ rows, uint32_t n,
                                                     const float *__restrict__ norm, const int32_t *__restrict__ count, int n_q,
                                                     uint32_t *__restrict__ seg_start, float *__restrict__ xs, int32_t *__restrict__ long_slot) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t q = qs[j];
    xs[j] = norm[rows[j]];
    if (q < static_cast<uint32_t>(n_q) && (j == 0 || qs[j - 1] != q)) {
        seg_start[q] = j;
        if (count[q] > kRankLong) long_slot[j / kRankLong] = static_cast<int32_t>(q);
    }
}
// (d) short chains: exactly the reference's loop, one category per thread
__global__ __launch_bounds__(256) void k_rank_short(int n_q, const int32_t *__restrict__ count, const uint32_t *__restrict__ seg_start, uint32_t n,
                                                    const float *__restrict__ xs, float *__restrict__ total) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const int c = count[q];
    if (c > kRankLong) return;
    float s = 0.0f;
    if (c > 0) {
        const uint32_t b = seg_start[q];
        if (b + static_cast<uint32_t>(c) <= n)
            for (int j = 0; j < c; ++j) s = s + xs[b + j];
    }
    total[q] = s;
}
// long chains: the slots with a category, compacted in order into the SeqChain table of seq_sums (one block).  blk0 = start / 256 + the
// chain's ordinal is ascending and leaves every chain its ceil(len / 256) blocks; the unused tail of the table gets empty chains behind
// every block.
__global__ __launch_bounds__(256) void k_rank_chains(const int32_t *__restrict__ long_slot, int n_slots, const int32_t *__restrict__ count,
                                                     const uint32_t *__restrict__ seg_start, const float *__restrict__ xs, SeqChain *__restrict__ chains,
                                                     int32_t *__restrict__ chain_q) {
    __shared__ int sc[256];
    const int tid = threadIdx.x;
    int base = 0;
    for (int k0 = 0; k0 < n_slots; k0 += 256) {
        const int k = k0 + tid;
        const int q = k < n_slots ? long_slot[k] : -1;
        const int flag = q >= 0 ? 1 : 0;
        sc[tid] = flag;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        if (flag) {
            const int ord = base + sc[tid] - 1;
            const uint32_t b = seg_start[q];
            SeqChain c;
            c.x = xs + b; c.len = static_cast<uint32_t>(count[q]); c.blk0 = b / 256u + static_cast<uint32_t>(ord); c.start = 0.0f;
            chains[ord] = c;
            chain_q[ord] = q;
        }
        base += sc[255];
        __syncthreads();
    }
    for (int i = base + tid; i < n_slots; i += 256) {
        SeqChain c;
        c.x = xs; c.len = 0; c.blk0 = 0xffffffffu; c.start = 0.0f;
        chains[i] = c;
        chain_q[i] = -1;
    }
}
__global__ __launch_bounds__(256) void k_rank_long_store(const int32_t *__restrict__ chain_q, const float *__restrict__ sums, int n,
                                                         float *__restrict__ total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && chain_q[i] >= 0) total[chain_q[i]] = sums[i];
}

inline size_t up256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
struct RankLayout {
    size_t norm, qa, qb, ra, rb, xs, seg, lslot, chains, chain_q, chain_out, hist, seq, bytes;
    uint32_t n_tiles, seq_blocks;
    int n_slots;
};
RankLayout rank_layout(int N, size_t n_cells, int n_q) {
    RankLayout L{};
    L.n_tiles = radix_sort_tiles(n_cells);
    L.n_slots = static_cast<int>((n_cells + kRankLong - 1) / kRankLong);
    L.seq_blocks = static_cast<uint32_t>(n_cells / 256 + static_cast<size_t>(L.n_slots) + 2);
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += up256(b); return at; };
    L.norm = take(sizeof(float) * static_cast<size_t>(N));
    L.qa = take(4 * n_cells); L.qb = take(4 * n_cells); L.ra = take(4 * n_cells); L.rb = take(4 * n_cells);
    L.xs = take(4 * n_cells + 64);
    L.seg = take(4 * static_cast<size_t>(std::max(1, n_q)));
    L.lslot = take(4 * static_cast<size_t>(L.n_slots));
    L.chains = take(sizeof(SeqChain) * static_cast<size_t>(L.n_slots));
    L.chain_q = take(4 * static_cast<size_t>(L.n_slots));
    L.chain_out = take(4 * static_cast<size_t>(L.n_slots));
    L.hist = take(4 * 256 * static_cast<size_t>(L.n_tiles));
    L.seq = take(seq_sums_scratch_bytes(L.seq_blocks));
    L.bytes = o;
    return L;
}

}  // namespace

bool cat_rank_fits(int N, int Fc) { return N > 0 && Fc > 0 && static_cast<size_t>(N) * Fc < (size_t(1) << 31) - kRadixTile; }

size_t cat_rank_scratch_bytes(int N, int Fc, int n_q) { return rank_layout(N, static_cast<size_t>(N) * Fc, n_q).bytes; }

void cat_rank(const char *cells, int N, int Fc, const float *grads, int D, const uint64_t *keys, int log2_cap, int32_t *meta,
              const int32_t *list_slot, int n_q, int32_t *slot_q, void *scratch, int32_t *count, float *total, hipStream_t s) {
    const size_t n_cells_sz = static_cast<size_t>(N) * Fc;
    if (n_cells_sz == 0 || n_q <= 0) return;
    const uint32_t n_cells = static_cast<uint32_t>(n_cells_sz);
    const RankLayout L = rank_layout(N, n_cells_sz, n_q);
    char *base = static_cast<char *>(scratch);
    float *norm = reinterpret_cast<float *>(base + L.norm);
    uint32_t *qa = reinterpret_cast<uint32_t *>(base + L.qa), *qb = reinterpret_cast<uint32_t *>(base + L.qb);
    uint32_t *ra = reinterpret_cast<uint32_t *>(base + L.ra), *rb = reinterpret_cast<uint32_t *>(base + L.rb);
    float *xs = reinterpret_cast<float *>(base + L.xs);
    uint32_t *seg = reinterpret_cast<uint32_t *>(base + L.seg);
    int32_t *lslot = reinterpret_cast<int32_t *>(base + L.lslot);
    SeqChain *chains = reinterpret_cast<SeqChain *>(base + L.chains);
    int32_t *chain_q = reinterpret_cast<int32_t *>(base + L.chain_q);
    float *chain_out = reinterpret_cast<float *>(base + L.chain_out);
    uint32_t *hist = reinterpret_cast<uint32_t *>(base + L.hist);
    const unsigned cell_blocks = (n_cells + 255u) / 256u;

    (void)hipMemsetAsync(count, 0, sizeof(int32_t) * static_cast<size_t>(n_q), s);
    (void)hipMemsetAsync(seg, 0, sizeof(uint32_t) * static_cast<size_t>(n_q), s);
    (void)hipMemsetAsync(lslot, 0xff, sizeof(int32_t) * static_cast<size_t>(L.n_slots), s);
    hipLaunchKernelGGL(k_rank_norms, dim3((N + 255) / 256), dim3(256), 0, s, grads, N, D, norm);
    hipLaunchKernelGGL(k_rank_slotq, dim3((n_q + 255) / 256), dim3(256), 0, s, meta, list_slot, n_q, slot_q);
    hipLaunchKernelGGL(k_rank_keys, dim3(cell_blocks), dim3(256), 0, s, cells, n_cells, Fc, reinterpret_cast<const unsigned long long *>(keys), slot_q,
                       log2_cap, n_q, qa, ra, count, meta);
    int bits = 1;
    while (bits < 32 && (static_cast<uint32_t>(n_q - 1) >> bits)) ++bits;
    for (int shift = 0; shift < bits; shift += 8) {
        radix_sort_pass(qa, ra, n_cells, 1, shift, hist, qb, rb, s);
        std::swap(qa, qb);
        std::swap(ra, rb);
    }
    hipLaunchKernelGGL(k_rank_bounds, dim3(cell_blocks), dim3(256), 0, s, qa, ra, n_cells, norm, count, n_q, seg, xs, lslot);
    hipLaunchKernelGGL(k_rank_short, dim3((n_q + 255) / 256), dim3(256), 0, s, n_q, count, seg, n_cells, xs, total);
    if (n_cells > static_cast<uint32_t>(kRankLong)) {
        // The addends are squared norms: non-negative.  The power-of-two edge case reported for seq_apply (a running sum that sits exactly on
        // 2^e and is pulled below it) needs an element of the opposite sign and cannot occur in these chains.
        hipLaunchKernelGGL(k_rank_chains, dim3(1), dim3(256), 0, s, lslot, L.n_slots, count, seg, xs, chains, chain_q);
        seq_sums(chains, L.n_slots, L.seq_blocks, base + L.seq, chain_out, nullptr, s);
        hipLaunchKernelGGL(k_rank_long_store, dim3((L.n_slots + 255) / 256), dim3(256), 0, s, chain_q, chain_out, L.n_slots, total);
    }
}

// diagnostics (gbrl_hip_cat_rank_stats): host arrays in; per distinct (feature, cell) pair its feature, first row, count and total out
int cat_rank_selftest(const char *cells, int n, int Fc, const float *grads, int D, int cap, int32_t *feat, int32_t *first_row, int32_t *count,
                      float *total) {
    if (!cat_rank_fits(n, Fc) || D < 1) return -1;
    const size_t n_cells = static_cast<size_t>(n) * Fc;
    const int list_cap = static_cast<int>(std::min<size_t>(n_cells, size_t(1) << 21));
    int log2_cap = 8;
    while ((1ll << log2_cap) < 4ll * n && log2_cap < 20) ++log2_cap;
    const size_t slots = static_cast<size_t>(Fc) << log2_cap;
    if (slots >= (size_t(1) << 31)) return -1;
    struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } };
    Dev dcells, dgrads, dkeys, dfirst, dmeta, dlslot, dslotq, dscr, dcnt, dtot;
    auto alloc = [](Dev &d, size_t b) { return hipMalloc(&d.p, std::max<size_t>(256, b)) == hipSuccess; };
    if (!alloc(dcells, n_cells * 128) || !alloc(dgrads, sizeof(float) * static_cast<size_t>(n) * D) || !alloc(dkeys, 8 * slots) || !alloc(dfirst, 4 * slots) ||
        !alloc(dmeta, 16) || !alloc(dlslot, 4 * static_cast<size_t>(list_cap)) || !alloc(dslotq, 4 * slots) ||
        !alloc(dscr, cat_rank_scratch_bytes(n, Fc, list_cap)) || !alloc(dcnt, 4 * static_cast<size_t>(list_cap)) || !alloc(dtot, 4 * static_cast<size_t>(list_cap))) {
        (void)hipGetLastError();
        return -1;
    }
    if (hipMemcpy(dcells.p, cells, n_cells * 128, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (hipMemcpy(dgrads.p, grads, sizeof(float) * static_cast<size_t>(n) * D, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (hipMemset(dkeys.p, 0, 8 * slots) != hipSuccess || hipMemset(dfirst.p, 0x7f, 4 * slots) != hipSuccess || hipMemset(dmeta.p, 0, 16) != hipSuccess) return -1;
    int32_t *meta = static_cast<int32_t *>(dmeta.p);
    cat_distinct_insert(static_cast<const char *>(dcells.p), n, Fc, static_cast<uint64_t *>(dkeys.p), static_cast<int32_t *>(dfirst.p), log2_cap, meta,
                        static_cast<int32_t *>(dlslot.p), meta + 2, list_cap, nullptr);
    cat_distinct_verify(static_cast<const char *>(dcells.p), n, Fc, static_cast<const uint64_t *>(dkeys.p), static_cast<const int32_t *>(dfirst.p), log2_cap, meta, nullptr);
    int32_t hm[4] = {0, 0, 0, 0};
    if (hipMemcpy(hm, meta, 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hm[0] != 0 || hm[1] != 0 || hm[2] > list_cap) return -1;
    const int n_q = hm[2];
    if (n_q > cap) return -2;
    cat_rank(static_cast<const char *>(dcells.p), n, Fc, static_cast<const float *>(dgrads.p), D, static_cast<const uint64_t *>(dkeys.p), log2_cap, meta,
             static_cast<const int32_t *>(dlslot.p), n_q, static_cast<int32_t *>(dslotq.p), dscr.p, static_cast<int32_t *>(dcnt.p), static_cast<float *>(dtot.p), nullptr);
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (hipMemcpy(hm, meta, 16, hipMemcpyDeviceToHost) != hipSuccess || hm[0] != 0) return -1;
    std::vector<int32_t> ls(n_q), fr(slots);
    if (hipMemcpy(ls.data(), dlslot.p, 4 * static_cast<size_t>(n_q), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(fr.data(), dfirst.p, 4 * slots, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int q = 0; q < n_q; ++q) { feat[q] = ls[q] >> log2_cap; first_row[q] = fr[ls[q]]; }
    if (hipMemcpy(count, dcnt.p, 4 * static_cast<size_t>(n_q), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(total, dtot.p, 4 * static_cast<size_t>(n_q), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n_q;
}

}  // namespace kern
}  // namespace gbrl
