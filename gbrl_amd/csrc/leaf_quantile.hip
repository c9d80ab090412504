// leaf_quantile.hip -- gfx950 kernels behind GBRL::quantile_leaves_prepared and fit_prepared(leaf_update="quantile"): per (leaf, output) of one tree the
// k-th largest residual x = fl32(p - y) among the rows the tree routes to the leaf, k from the leaf's row count and the output's level.
// quantile_core.h has the rule; the result is one of the inputs, bit for bit, so two different algorithms must (and do) return the same bytes.
//
//   k_lq_route          one thread per row: the code walk (predict_rowwalk.h: general_leaf on the bin codes), the local leaf index per row (-1 when the
//                       search leaves the tree), the keys quantile_key(x) column-major [D][m] so that every later pass coalesces, the rows per leaf
//                       (integer LDS counters for the select path's trees, one global add per non-zero counter and block; wave-aggregated global adds
//                       for the larger trees of the general path) and the flag word (a p, y or x that is not finite).  rows= and abs_index as in newton.hip.
//   select path         per-(leaf, output) MSD radix select, 8 bits a pass, no sort and no data movement.  A leaf has exactly one live prefix at any
//     k_lq_count        time, so the slot is the leaf: one block = one output column x chunks of kRowsPerChunk rows (grid-stride over the chunks), LDS
//     k_lq_target       holds prefix[leaf] and uint32 counters [leaf][256]; a key counts in pass q iff its upper digits equal its leaf's prefix; the block
//                       stores its counters as a partial (no global atomics, nothing to zero).  The target pass (one block per (leaf, output), thread =
//                       digit: the partials are read coalesced) sums the partials, finds the digit that holds the remaining rank counted from the
//                       largest key, and updates prefix and rank; pass 0 takes k from the leaf's count by quantile_rank on the device.  After the last
//                       digit the prefix is the key.  Ties stay in one counter to the last digit; where a whole wave meets one counter it adds once
//                       (goss.hip's ballot shortcut).  Trees of up to kMaxSelectLeaves leaves whose counters the LDS opt-in covers.
//   general path        more leaves, a refused opt-in, GBRL_HIP_CONTINUE_GENERIC=1: every key column sorted by radix_sort.hip (the columns are the
//     k_lq_offsets      segments, the leaf id rides along), then sorted stably by leaf id, one 8-bit pass per byte of the id (rows outside the tree carry
//     k_lq_pick         the id n_leaves and end up last); the leaf offsets from the counts; element off[leaf] + m_leaf - k is the answer.
//
//   k_lq_bias_keys      a fresh model's bias: the keys of fl32(0 - y) with every row in leaf 0, then the select path's passes with one leaf.
//
//   The result block res (uint32 words, ZEROED by the caller on `s`): keys [n_leaves][D], ranks [n_leaves][D], counts [n_leaves], flag -- one read-back.
#include "kernels.h"
#include "kernels_common.h"
#include "leaf_accum.h"
#include "predict_rowwalk.h"
#include "quantile_core.h"

#include <algorithm>

namespace gbrl {
namespace kern {

namespace {

constexpr int kMaxSelectLeaves = 64;    // 64 leaves x 256 digits x 4 B = 64 KiB of counters (+ the prefixes): a depth-6 tree
constexpr int kRowsPerChunk = 2048;     // rows one block of the count pass takes at a time: 256 threads x 8
constexpr int kMaxCountBlocks = 32;     // chunk blocks per output column: the partials stay small (blocks x D x leaves KiB per pass)
constexpr int kRouteLdsLeaves = kMaxSelectLeaves;   // leaf counters of the route pass kept in LDS: the select path's trees

__device__ __forceinline__ uint32_t lq_leaf_id(int l, int n_leaves) { return l < 0 ? static_cast<uint32_t>(n_leaves) : static_cast<uint32_t>(l); }

// ------------------------------------------------------------------------------------------------------------ route and key pass
__global__ __launch_bounds__(256) void k_lq_route(LeavesModel cm, TreeSpan tr, CodeRows cr, int m, int D, const float *__restrict__ pred,
                                                  const float *__restrict__ targets, int abs_index, int32_t *__restrict__ leaf_out,
                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ id_cols, uint32_t *__restrict__ counts,
                                                  uint32_t *__restrict__ flag_out) {
#pragma clang fp contract(off)
    __shared__ uint32_t lcnt[kRouteLdsLeaves];
    const bool in_lds = tr.n_leaves <= kRouteLdsLeaves;   // (uniform)
    if (in_lds) {
        leaf_acc_zero(lcnt, tr.n_leaves, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = j < static_cast<size_t>(m);   // (dead lanes stay for the ballots and the barriers)
    const size_t jj = live ? j : 0;
    const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + jj] : cr.row0 + static_cast<int>(jj));
    const GeneralCodeRow r{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    const int lane = threadIdx.x & (kWave - 1);
    int l = -1;
    if (live) {
        l = local_leaf(general_leaf(cm, r, tr.t), tr.leaf0, tr.n_leaves);
        leaf_out[j] = l;
    }
    const size_t pr = abs_index ? src : jj;
    const float *p = pred + pr * D;
    const float *y = targets + pr * D;
    const uint32_t id = lq_leaf_id(l, tr.n_leaves);
    unsigned flag = 0;
    if (live) {
#pragma unroll 1
        for (int d = 0; d < D; ++d) {
            const float pd = p[d], yd = y[d];
            const float x = quantile_residual(pd, yd);
            if (quantile_not_finite(pd)) flag |= kQuantileBadPred;
            if (quantile_not_finite(yd)) flag |= kQuantileBadTarget;
            if (quantile_not_finite(x)) flag |= kQuantileBadResidual;
            keys[static_cast<size_t>(d) * m + j] = quantile_key(x);
            if (id_cols != nullptr) id_cols[static_cast<size_t>(d) * m + j] = id;
        }
    }
    if (in_lds) {
        if (l >= 0) atomicAdd(&lcnt[l], 1u);
        __syncthreads();
        leaf_acc_flush(lcnt, counts, tr.n_leaves, threadIdx.x, blockDim.x);
    } else {   // one add per distinct leaf of the wave
        for_each_wave_leaf(l, lane, [&](int k, bool, unsigned long long same, bool leader) {
            if (leader) atomicAdd(&counts[k], static_cast<uint32_t>(__popcll(same)));
        });
    }
    if (flag) atomicOr(flag_out, flag);
}

// the bias of a fresh model: one leaf of every row at p = 0 -- the keys of fl32(0 - y), the leaf 0 for every row, its count n
__global__ __launch_bounds__(256) void k_lq_bias_keys(const float *__restrict__ targets, int n, int D, int32_t *__restrict__ leaf_out, uint32_t *__restrict__ keys,
                                                      uint32_t *__restrict__ counts, uint32_t *__restrict__ flag_out) {
#pragma clang fp contract(off)
    const size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j == 0) counts[0] = static_cast<uint32_t>(n);
    if (j >= static_cast<size_t>(n)) return;
    leaf_out[j] = 0;
    const float *y = targets + j * D;
    unsigned flag = 0;
#pragma unroll 1
    for (int d = 0; d < D; ++d) {
        const float yd = y[d];
        if (quantile_not_finite(yd)) flag |= kQuantileBadTarget;
        keys[static_cast<size_t>(d) * n + j] = quantile_key(quantile_residual(0.0f, yd));
    }
    if (flag) atomicOr(flag_out, flag);
}

// ------------------------------------------------------------------------------------------------------------ select path
// pass q of 4: digit (key >> (24 - 8 q)) & 255 of every key whose upper q digits are its leaf's prefix; part [D][blocks][n_leaves][256]
__global__ __launch_bounds__(256) void k_lq_count(const uint32_t *__restrict__ keys, const int32_t *__restrict__ leaf, int m, int n_leaves, int pass,
                                                  const uint32_t *__restrict__ prefix /*[D][n_leaves]*/, uint32_t *__restrict__ part) {
    extern __shared__ __align__(16) uint32_t lq_lds[];   // [n_leaves][256] counters, then [n_leaves] prefixes
    uint32_t *cnt = lq_lds;
    uint32_t *pfx = lq_lds + static_cast<size_t>(n_leaves) * 256;
    const int d = blockIdx.y;
    const int n_cnt = n_leaves * 256;
    for (int i = threadIdx.x; i < n_cnt; i += blockDim.x) cnt[i] = 0u;
    if (pass > 0)
        for (int i = threadIdx.x; i < n_leaves; i += blockDim.x) pfx[i] = prefix[static_cast<size_t>(d) * n_leaves + i];
    __syncthreads();
    const uint32_t *col = keys + static_cast<size_t>(d) * m;
    const int shift = 24 - 8 * pass;
    const int lane = threadIdx.x & (kWave - 1);
    const int n_chunks = (m + kRowsPerChunk - 1) / kRowsPerChunk;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {   // (uniform over the block)
        const int r0 = c * kRowsPerChunk;
#pragma unroll 1
        for (int i = 0; i < kRowsPerChunk / 256; ++i) {   // (whole waves stay for the ballots)
            const int j = r0 + i * 256 + static_cast<int>(threadIdx.x);
            bool in = j < m;
            uint32_t slot = 0;
            if (in) {
                const int l = leaf[j];
                const uint32_t key = col[j];
                in = l >= 0 && (pass == 0 || (key >> (shift + 8)) == pfx[l]);
                slot = static_cast<uint32_t>(l >= 0 ? l : 0) * 256u + ((key >> shift) & 255u);
            }
            const unsigned long long act = __ballot(in);
            if (act == 0ull) continue;   // (wave-uniform)
            const int first = __ffsll(static_cast<long long>(act)) - 1;
            const uint32_t s0 = __shfl(slot, first, kWave);
            const unsigned long long same = __ballot(in && slot == s0);
            if (same == act) {   // the wave meets one counter: one add
                if (lane == first) atomicAdd(&cnt[s0], static_cast<uint32_t>(__popcll(act)));
            } else if (in) {
                atomicAdd(&cnt[slot], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t *out = part + (static_cast<size_t>(d) * gridDim.x + blockIdx.x) * n_cnt;
    for (int i = threadIdx.x; i < n_cnt; i += blockDim.x) out[i] = cnt[i];
}

// one block per (leaf, output), thread = digit: the digit that holds the remaining rank counted from the largest key
__global__ __launch_bounds__(256) void k_lq_target(const uint32_t *__restrict__ part, int n_blocks, int n_leaves, int D, int pass, const float *__restrict__ alpha,
                                                   const uint32_t *__restrict__ counts, uint32_t *__restrict__ prefix, uint32_t *__restrict__ rem,
                                                   uint32_t *__restrict__ keys_out, uint32_t *__restrict__ ranks_out) {
    __shared__ uint32_t scan[2][256];
    const int l = blockIdx.x, d = blockIdx.y, dg = threadIdx.x;
    const size_t n_cnt = static_cast<size_t>(n_leaves) * 256;
    uint32_t mine = 0;
    for (int b = 0; b < n_blocks; ++b) mine += part[(static_cast<size_t>(d) * n_blocks + b) * n_cnt + static_cast<size_t>(l) * 256 + dg];
    // keys at or above this digit: an inclusive scan from digit 255 down (Hillis-Steele over the mirrored index, integers: order-free)
    const int r = 255 - dg;
    int cur = 0;
    scan[0][r] = mine;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t v = scan[cur][r] + (r >= off ? scan[cur][r - off] : 0u);
        scan[cur ^ 1][r] = v;
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t at_or_above = scan[cur][r], above = at_or_above - mine;
    const size_t at = static_cast<size_t>(d) * n_leaves + l;
    const uint32_t rows = counts[l];
    const uint32_t k = pass == 0 ? static_cast<uint32_t>(quantile_rank(static_cast<long long>(rows), alpha[d])) : rem[at];
    const uint32_t pf = pass == 0 ? 0u : prefix[at];
    if (rows == 0u) {   // an empty leaf: prefix 0, rank 0
        if (dg == 0) {
            prefix[at] = 0u;
            rem[at] = 0u;
            if (pass == 0) ranks_out[static_cast<size_t>(l) * D + d] = 0u;
            if (pass == 3) keys_out[static_cast<size_t>(l) * D + d] = 0u;
        }
        return;
    }
    __syncthreads();   // every thread has read prefix[at] and rem[at]: the one below may write them
    if (above < k && k <= at_or_above) {   // exactly one digit holds the rank (1 <= k <= the keys that counted)
        const uint32_t next = (pf << 8) | static_cast<uint32_t>(dg);
        prefix[at] = next;
        rem[at] = k - above;
        if (pass == 0) ranks_out[static_cast<size_t>(l) * D + d] = k;
        if (pass == 3) keys_out[static_cast<size_t>(l) * D + d] = next;
    }
}

// ------------------------------------------------------------------------------------------------------------ general path
__global__ void k_lq_offsets(const uint32_t *__restrict__ counts, int n_leaves, uint32_t *__restrict__ off) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t run = 0;
    for (int l = 0; l < n_leaves; ++l) {
        off[l] = run;
        run += counts[l];
    }
}

// sorted [D][m]: by leaf id, and within a leaf by key ascending -- the k-th largest of leaf l is element off[l] + rows - k of its column
__global__ __launch_bounds__(256) void k_lq_pick(const uint32_t *__restrict__ sorted, int m, int n_leaves, int D, const float *__restrict__ alpha,
                                                 const uint32_t *__restrict__ counts, const uint32_t *__restrict__ off, uint32_t *__restrict__ keys_out,
                                                 uint32_t *__restrict__ ranks_out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= static_cast<size_t>(n_leaves) * D) return;
    const int l = static_cast<int>(i / D), d = static_cast<int>(i % D);
    const uint32_t rows = counts[l];
    const uint32_t k = static_cast<uint32_t>(quantile_rank(static_cast<long long>(rows), alpha[d]));
    ranks_out[i] = k;
    keys_out[i] = rows == 0u ? 0u : sorted[static_cast<size_t>(d) * m + off[l] + rows - k];
}

size_t lq_select_lds(int n_leaves) { return static_cast<size_t>(n_leaves) * 257 * sizeof(uint32_t); }
int lq_count_blocks(int m) { return std::min((m + kRowsPerChunk - 1) / kRowsPerChunk, kMaxCountBlocks); }
int lq_id_passes(int n_leaves) {   // bytes of the largest id, n_leaves itself
    int passes = 1;
    for (uint32_t v = static_cast<uint32_t>(n_leaves) >> 8; v != 0; v >>= 8) ++passes;
    return passes;
}
size_t lq_align(size_t words) { return (words + 63) & ~static_cast<size_t>(63); }   // 256-byte steps

bool lq_select_ok(int n_leaves, bool generic) {
    if (generic || n_leaves > kMaxSelectLeaves) return false;
    static StreamLdsOptIn optin;
    return optin.ok(k_lq_count, lq_select_lds(n_leaves));
}

// the four count / target passes over keys [D][m] and leaf [m]
void lq_select_passes(const uint32_t *keys, const int32_t *leaf, int m, int n_leaves, int D, const float *alpha, const uint32_t *counts, uint32_t *prefix,
                      uint32_t *rem, uint32_t *part, uint32_t *keys_out, uint32_t *ranks_out, hipStream_t s) {
    const int blocks = lq_count_blocks(m);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(k_lq_count, dim3(blocks, D), dim3(256), lq_select_lds(n_leaves), s, keys, leaf, m, n_leaves, pass, prefix, part);
        hipLaunchKernelGGL(k_lq_target, dim3(n_leaves, D), dim3(256), 0, s, part, blocks, n_leaves, D, pass, alpha, counts, prefix, rem, keys_out, ranks_out);
    }
}

// *flag |= kQuantileBadTarget when any entry of a target matrix is not finite (fit_prepared refuses it before anything changes)
__global__ __launch_bounds__(256) void k_lq_check_targets(const float *__restrict__ targets, size_t n_el, uint32_t *__restrict__ flag) {
    bool bad = false;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el; i += static_cast<size_t>(gridDim.x) * blockDim.x)
        bad = bad || quantile_not_finite(targets[i]);
    if (bad) atomicOr(flag, static_cast<uint32_t>(kQuantileBadTarget));
}

}  // namespace

void leaf_quantile_check_targets(const float *targets, size_t n_el, uint32_t *flag, hipStream_t s) {
    if (n_el == 0) return;
    hipLaunchKernelGGL(k_lq_check_targets, dim3(static_cast<unsigned>(std::min<size_t>((n_el + 255) / 256, 4096))), dim3(256), 0, s, targets, n_el, flag);
}

void leaf_quantile_geometry(int *max_select_leaves, int *rows_per_chunk) {
    if (max_select_leaves) *max_select_leaves = kMaxSelectLeaves;
    if (rows_per_chunk) *rows_per_chunk = kRowsPerChunk;
}

bool leaf_quantile_fits(int m, int D) { return static_cast<size_t>(m) * D < (static_cast<size_t>(1) << 31) - kRadixSortTile; }

LeafQuantilePlan leaf_quantile_plan(int m, int D, int n_leaves, bool generic) {
    LeafQuantilePlan plan;
    plan.select = lq_select_ok(n_leaves, generic);
    const size_t cells = static_cast<size_t>(m) * D;
    size_t words = lq_align(static_cast<size_t>(m)) + lq_align(cells);   // the leaf per row, the keys
    if (plan.select) {
        words += 2 * lq_align(static_cast<size_t>(D) * n_leaves);                                     // prefix, remaining rank
        words += lq_align(static_cast<size_t>(lq_count_blocks(m)) * D * n_leaves * 256);             // the partials
    } else {
        words += 3 * lq_align(cells);                                                                 // the ids, and the sort's second pair
        words += lq_align(static_cast<size_t>(D) * 256 * radix_sort_tiles(static_cast<size_t>(m)));   // its histograms
        words += lq_align(static_cast<size_t>(n_leaves));                                             // the leaf offsets
    }
    plan.scratch_bytes = words * sizeof(uint32_t);
    return plan;
}

void leaf_quantile(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int tree, int leaf0, int n_leaves, const float *pred,
                   const float *targets, bool abs_index, const float *alpha, const LeafQuantilePlan &plan, void *scratch, uint32_t *res, hipStream_t s) {
    if (m <= 0 || n_leaves <= 0) return;
    const int D = pm.D;
    LeavesModel cm = leaves_model(pm);   // the routing view of the float walk with the threshold words replaced by bins
    cm.cond_pack = ct.cond_pack;
    cm.grd_nodes = ct.grd_nodes;
    cm.feature_bins = ct.bins;
    const size_t cells = static_cast<size_t>(m) * D, nld = static_cast<size_t>(n_leaves) * D;
    uint32_t *keys_out = res, *ranks_out = res + nld, *counts = res + 2 * nld, *flag = counts + n_leaves;
    uint32_t *w = static_cast<uint32_t *>(scratch);
    int32_t *leaf = reinterpret_cast<int32_t *>(w); w += lq_align(static_cast<size_t>(m));
    uint32_t *keys = w; w += lq_align(cells);
    const TreeSpan tr{tree, leaf0, n_leaves};
    if (plan.select) {
        uint32_t *prefix = w; w += lq_align(nld);
        uint32_t *rem = w; w += lq_align(nld);
        uint32_t *part = w;
        hipLaunchKernelGGL(k_lq_route, dim3((m + 255) / 256), dim3(256), 0, s, cm, tr, cr, m, D, pred, targets, abs_index ? 1 : 0, leaf, keys,
                           static_cast<uint32_t *>(nullptr), counts, flag);
        lq_select_passes(keys, leaf, m, n_leaves, D, alpha, counts, prefix, rem, part, keys_out, ranks_out, s);
        return;
    }
    uint32_t *ids = w; w += lq_align(cells);
    uint32_t *keys_b = w; w += lq_align(cells);
    uint32_t *ids_b = w; w += lq_align(cells);
    uint32_t *hist = w; w += lq_align(static_cast<size_t>(D) * 256 * radix_sort_tiles(static_cast<size_t>(m)));
    uint32_t *off = w;
    hipLaunchKernelGGL(k_lq_route, dim3((m + 255) / 256), dim3(256), 0, s, cm, tr, cr, m, D, pred, targets, abs_index ? 1 : 0, leaf, keys, ids, counts, flag);
    uint32_t *ka = keys, *va = ids, *kb = keys_b, *vb = ids_b;
    const uint32_t um = static_cast<uint32_t>(m);
    for (int shift = 0; shift < 32; shift += 8) {   // every column by key, the leaf id riding along
        radix_sort_pass(ka, va, um, D, shift, hist, kb, vb, s);
        std::swap(ka, kb); std::swap(va, vb);
    }
    for (int b = 0; b < lq_id_passes(n_leaves); ++b) {   // then stably by leaf id: the id is the key now
        radix_sort_pass(va, ka, um, D, 8 * b, hist, vb, kb, s);
        std::swap(ka, kb); std::swap(va, vb);
    }
    hipLaunchKernelGGL(k_lq_offsets, dim3(1), dim3(1), 0, s, counts, n_leaves, off);
    hipLaunchKernelGGL(k_lq_pick, dim3(static_cast<unsigned>((nld + 255) / 256)), dim3(256), 0, s, ka, m, n_leaves, D, alpha, counts, off, keys_out, ranks_out);
}

size_t leaf_quantile_bias_scratch_bytes(int n, int D) { return leaf_quantile_plan(n, D, 1, false).scratch_bytes; }

void leaf_quantile_bias(const float *targets, int n, int D, const float *alpha, void *scratch, uint32_t *res, hipStream_t s) {
    if (n <= 0) return;
    (void)lq_select_ok(1, false);   // (one leaf: 1 KiB of counters, no opt-in is needed)
    const size_t cells = static_cast<size_t>(n) * D;
    uint32_t *keys_out = res, *ranks_out = res + D, *counts = res + 2 * D, *flag = counts + 1;
    uint32_t *w = static_cast<uint32_t *>(scratch);
    int32_t *leaf = reinterpret_cast<int32_t *>(w); w += lq_align(static_cast<size_t>(n));
    uint32_t *keys = w; w += lq_align(cells);
    uint32_t *prefix = w; w += lq_align(static_cast<size_t>(D));
    uint32_t *rem = w; w += lq_align(static_cast<size_t>(D));
    uint32_t *part = w;
    hipLaunchKernelGGL(k_lq_bias_keys, dim3((n + 255) / 256), dim3(256), 0, s, targets, n, D, leaf, keys, counts, flag);
    lq_select_passes(keys, leaf, n, 1, D, alpha, counts, prefix, rem, part, keys_out, ranks_out, s);
}

}  // namespace kern
}  // namespace gbrl
