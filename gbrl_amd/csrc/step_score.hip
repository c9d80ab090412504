// step_score.hip -- split scores and selection of GBRL::step: candidate scores from the exact histograms, the two-stage arg-max, and the
// resolution of every node's winner into a split descriptor with its child sizes.
//
// Arithmetic policy (DESIGN.md "exact sums"): every sum that feeds a split decision or a leaf value is an INTEGER
// sum of fixed-point values, so results do not depend on the order in which waves, blocks or GPUs add them
// (deterministic, and bit-identical for 1/2/4/8 row shards).  Scores are evaluated in fp64 from those exact sums and
// rounded to fp32 once, then compared the way the reference compares them (fitter.cpp:332-341, 435-444).
#include "kernels.h"
#include "kernels_common.h"
#include "score_common.h"
#include "../../include/gbrl_hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace gbrl {
namespace kern {

namespace {

// ------------------------------------------------------------------------------------------------------------
// A6/A7  candidate scores from the exact histograms.  One block per (node, feature slot).
//   numeric candidate k : right = classes > k (suffix sum), left = total - right
//   categorical cand. j : right = class j+1,                left = total - right
//   L2     : |S_L|^2/n_L + |S_R|^2/n_R            (== n_L|mean_L|^2 + n_R|mean_R|^2, node.cpp:360-373)
//   Cosine : sqrt of the same quantity, 0 if it is 0 (== cosine_score, math_ops.h:538-575, since
//            sum_{i in S} g_i . mean_S = |sum_S g|^2 / n_S)
// evaluated in fp64 from integer sums and rounded once to fp32.  -inf when the candidate repeats a condition of the
// node's path (node.cpp:154-166) or a side has fewer than min_data_in_leaf rows (node.cpp:354).
// Block (slot 0) also emits the node's parent score for greedy growth (split_candidate_generator.cpp:262-320).
// ------------------------------------------------------------------------------------------------------------
constexpr int kScoreLoads = 10;
__global__ __launch_bounds__(256, 5) void k_score(int64_t *__restrict__ hist, const int64_t *__restrict__ hist_prev,
                                               const int32_t *__restrict__ sub_par, const int32_t *__restrict__ sub_sib, int Fp, int NB, int D,
                                               const FeatureSlot *__restrict__ slots, const float *__restrict__ thr,
                                               int B, int n_cand, int min_data, int cosine, const StepScales *__restrict__ scp,
                                               const int32_t *__restrict__ path_len, const int32_t *__restrict__ path_slot,
                                               const float *__restrict__ path_val, const int32_t *__restrict__ path_bin,
                                               float *__restrict__ scores, float *__restrict__ parent,
                                               const float *__restrict__ cand_w, const int32_t *__restrict__ cand_ref,
                                               const int32_t *__restrict__ is_root, float *__restrict__ part_v, int32_t *__restrict__ part_i, int slot0,
                                               int keep_derived, float *__restrict__ part_s /*nullable: second-best DISTINCT gain per block (near-tie detection)*/,
                                               int32_t *__restrict__ part_n /*with part_s: rows the block's best sends right*/,
                                               int32_t *__restrict__ cand_nr /*nullable, scores mode: [n_nodes][n_cand] rows every candidate sends right*/) {
    extern __shared__ int64_t sh64[];  // [NB][D+1] suffix sums (numeric) or raw classes (categorical)
    const double inv_scale = scp->inv_scale;
    const int node = blockIdx.y, fs = slot0 + blockIdx.x;
    const FeatureSlot sl = slots[fs];
    const int W = D + 1;
    // classes this slot really has (numeric: n_bins thresholds + 1; categorical: its candidates + "none of them"): the slices are NB
    // classes apart, but the classes beyond NBe hold nothing -- not loaded, not scanned, not written back (a 33-class categorical
    // slot beside 257-class numeric ones moved 8x the bytes it needed; k_resolve_splits applies the same bound)
    const int NBe = min(NB, sl.n_cand + 1);
    int64_t *src = hist + (static_cast<size_t>(node) * Fp + fs) * NB * W;
    // the node's path conditions on THIS feature slot, staged once per block (a candidate that repeats one of them is rejected,
    // node.cpp:154-166); reading the path arrays from global memory inside the candidate loop costs a memory round trip per
    // path entry and thread at the deep levels.  The first wave reads one path entry per lane (kMaxPath <= 64) and the four loads
    // are issued HERE, unconditionally (the arrays hold kMaxPath entries per node), so that they are in flight with the histogram
    // loads below instead of three dependent round trips after the scan; they are consumed just before the loads' barrier.
    __shared__ float s_pval[kMaxPath];
    __shared__ int s_pbin[kMaxPath];
    __shared__ int s_np;
    static_assert(kMaxPath <= kWave, "one lane per path entry");
    int q_len = 0, q_slot = -1, q_bin = 0;
    float q_val = 0.0f;
    if (threadIdx.x < kMaxPath) {
        q_len = path_len[node];
        q_slot = path_slot[node * kMaxPath + threadIdx.x];
        q_val = path_val[node * kMaxPath + threadIdx.x];
        q_bin = path_bin[node * kMaxPath + threadIdx.x];
    }
    const int par = sub_par ? sub_par[node] : -1;
    if (par >= 0) {
        // sibling subtraction fused here: this node was not accumulated from the data; its histogram is parent - sibling (exact
        // integers).  The slice is written back because the next level subtracts from it and k_resolve_splits reads it -- except at
        // the LAST level (keep_derived == 0): nothing subtracts from it any more, and k_resolve_splits derives the winner's class
        // counts from the same two slices (one third of this kernel's traffic at the deepest, most expensive level).
        const int sib = sub_sib[node];
        const int64_t *pp = hist_prev + (static_cast<size_t>(par) * Fp + fs) * NB * W;
        const int64_t *ss = sib >= 0 ? hist + (static_cast<size_t>(sib) * Fp + fs) * NB * W : nullptr;
        // kScoreLoads elements per thread in flight: the whole slice of a 257-class, 9-field slot (2313 words / 256 threads) in ONE batch --
        // a block is a chain of dependent phases and every extra batch is a memory round trip on it
        const int tot = NBe * W, step = static_cast<int>(blockDim.x);
        for (int i0 = threadIdx.x; i0 < tot; i0 += kScoreLoads * step) {
            int64_t a[kScoreLoads], b[kScoreLoads];
#pragma unroll
            for (int u = 0; u < kScoreLoads; ++u) {
                const int i = i0 + u * step;
                a[u] = i < tot ? pp[i] : 0;
                b[u] = (ss && i < tot) ? ss[i] : 0;
            }
#pragma unroll
            for (int u = 0; u < kScoreLoads; ++u) {
                const int i = i0 + u * step;
                if (i < tot) { const int64_t v = a[u] - b[u]; sh64[i] = v; if (keep_derived) src[i] = v; }
            }
        }
    } else {
        const int tot = NBe * W, step = static_cast<int>(blockDim.x);
        for (int i0 = threadIdx.x; i0 < tot; i0 += kScoreLoads * step) {
            int64_t a[kScoreLoads];
#pragma unroll
            for (int u = 0; u < kScoreLoads; ++u) { const int i = i0 + u * step; a[u] = i < tot ? src[i] : 0; }
#pragma unroll
            for (int u = 0; u < kScoreLoads; ++u) { const int i = i0 + u * step; if (i < tot) sh64[i] = a[u]; }
        }
    }
    if (threadIdx.x < kWave) {
        const int p = threadIdx.x;
        const bool hit = p < kMaxPath && p < q_len && q_slot == fs;
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const int pos = __popcll(m & ((1ull << p) - 1));
            s_pval[pos] = q_val;
            s_pbin[pos] = q_bin;
        }
        if (p == 0) s_np = __popcll(m);
    }
    __syncthreads();
    // totals = sum over all classes; also turn numeric features into suffix sums in place.  Block-wide scan: thread t of a
    // 256-class tile owns class NB-1-(tile*256+t), so an inclusive prefix over t is the suffix sum over classes.  Up to 9
    // fields are scanned together so that their cross-lane shuffles overlap.
    int64_t *total = sh64 + static_cast<size_t>(NB) * W;  // [D+1]
    double *total_f = reinterpret_cast<double *>(total + W);   // [D+1] the same totals as doubles
    constexpr int WCH = 9;
    __shared__ long long wsum[4][WCH];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int w0 = 0; w0 < W; w0 += WCH) {
        long long run_base[WCH];
#pragma unroll
        for (int j = 0; j < WCH; ++j) run_base[j] = 0;
        // (a last tile of at most 4 classes -- 257 classes = 256 + 1 is the usual shape -- is added serially below instead of
        // paying a block-wide scan and two barriers for it)
        const int n_tiles = (NBe + 255) / 256 - ((NBe % 256) != 0 && (NBe % 256) <= 4 && NBe > 256 ? 1 : 0);
        for (int tile = 0; tile < n_tiles; ++tile) {
            const int c = NBe - 1 - (tile * 256 + static_cast<int>(threadIdx.x));
            long long v[WCH];
#pragma unroll
            for (int j = 0; j < WCH; ++j) v[j] = (c >= 0 && w0 + j < W) ? sh64[c * W + w0 + j] : 0;
            static_assert(WCH == 9, "wave_scan9");
            wave_scan9(v);   // within rows of 16 lanes (row_shr 1, 2, 4, 8), then across the rows (row_bcast 15, 31)
            if (lane == kWave - 1) {
#pragma unroll
                for (int j = 0; j < WCH; ++j) wsum[wave][j] = v[j];
            }
            __syncthreads();
            {   // wave by wave (not all 36 partial sums at once: they would be the kernel's register peak and cost a wave of occupancy)
                long long below[WCH], all[WCH];
#pragma unroll
                for (int j = 0; j < WCH; ++j) { below[j] = 0; all[j] = 0; }
#pragma unroll 1
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j = 0; j < WCH; ++j) { const long long x = wsum[i][j]; if (i < wave) below[j] += x; all[j] += x; }
                }
#pragma unroll
                for (int j = 0; j < WCH; ++j) {
                    if (c >= 0 && !sl.is_cat && w0 + j < W) sh64[c * W + w0 + j] = v[j] + run_base[j] + below[j];
                    run_base[j] += all[j];
                }
            }
            __syncthreads();
        }
        const int rem = NBe - n_tiles * 256;       // classes 0 .. rem-1 not covered by a tile (0 or 1..4): suffix sums by one thread per field
        if (static_cast<int>(threadIdx.x) < WCH && w0 + static_cast<int>(threadIdx.x) < W) {
            const int j = threadIdx.x;
            long long run = 0;
#pragma unroll
            for (int jj = 0; jj < WCH; ++jj) if (jj == j) run = run_base[jj];
            for (int c = rem - 1; c >= 0; --c) {
                run += sh64[c * W + w0 + j];
                if (!sl.is_cat) sh64[c * W + w0 + j] = run;
            }
            total[w0 + j] = run;
            total_f[w0 + j] = static_cast<double>(run);   // exact (|sums| < 2^53): the left side below is total_f - (double)right, no int64 subtraction + second conversion
        }
    }
    __syncthreads();
    const int64_t n_tot = total[D];
    // parent score of the node (greedy growth): the totals are the same integers for every feature of the node, so every block
    // derives the identical float
    float par_score = 0.0f;
    if (blockIdx.x == 0 || part_v) {   // oblivious growth needs it from one block only
        const double x = side_term(total, D, n_tot, inv_scale);
        par_score = static_cast<float>(cosine ? sqrt(x) : x);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) parent[node] = par_score;
    // greedy growth (part_v != null): the block also reduces its candidates to one best (gain, reference index) -- stage 1 of the
    // arg-max, fused here so that a greedy level needs no separate arg-max launch (fitter.cpp:318-354: gain = fma(score, w, -parent),
    // root parent = 0, lowest reference index among maxima)
    const float par_sub = (part_v && is_root[node]) ? 0.0f : par_score;
    Best mine{-INFINITY, 0x7fffffff};
    float second = -INFINITY;     // the best gain of a candidate of another class (score_common.h second_merge)
    int mine_nr = -1;             // rows the block's best sends right
    const int np = s_np;
    for (int k = threadIdx.x; k < sl.n_cand; k += blockDim.x) {
        const int64_t *R = sh64 + (k + 1) * W;
        const int64_t n_r = R[D], n_l = n_tot - n_r;
        bool reject = (n_l < min_data) || (n_r < min_data);
        if (np > 0) {
            const float tk = sl.is_cat ? 0.0f : thr[static_cast<size_t>(fs) * B + k];
            for (int p = 0; p < np; ++p) {
                if (sl.is_cat) reject |= (s_pbin[p] == k + 1);
                else reject |= (s_pval[p] == tk);
            }
        }
        float out;
        if (reject) {
            out = -INFINITY;
        } else {
            // (score_common.h: the fused RL-sized growth kernel evaluates the same expression.)  k_score is bound by its VALU instruction
            // count and this loop was 170 of them per candidate (now ~115).
            out = candidate_score([&](int d) { return static_cast<double>(R[d]); }, total_f, D, n_l, n_r, cosine, inv_scale);
        }
        if (part_v) {
            const int j = sl.cand_base + k;
            const float gain = fmaf(out, cand_w[j], -par_sub);
            const Best cb{gain, cand_ref[j]};
            const int cls = part_n ? near_class(n_r, n_tot) : 0;     // (part_n == nullptr: batches of <= 8192 rows, classes by the gain alone)
            second = second_merge(mine.v, mine_nr, second, gain, cls, -INFINITY);
            if (better_takes_second(mine, cb)) { mine = cb; mine_nr = cls; }
        } else {
            scores[static_cast<size_t>(node) * n_cand + sl.cand_base + k] = out;
            if (cand_nr) cand_nr[static_cast<size_t>(node) * n_cand + sl.cand_base + k] = near_class(n_r, n_tot);
        }
    }
    if (part_v) {
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const Best other{__shfl_xor(mine.v, o, kWave), __shfl_xor(mine.i, o, kWave)};
            if (part_s) {
                const int onr = __shfl_xor(mine_nr, o, kWave);
                second = second_merge(mine.v, mine_nr, second, other.v, onr, __shfl_xor(second, o, kWave));
                if (better_takes_second(mine, other)) mine_nr = onr;
            }
            mine = better(mine, other);
        }
        __shared__ float bv[4], b2[4];
        __shared__ int bi[4], bn[4];
        if (lane == 0) { bv[wave] = mine.v; bi[wave] = mine.i; b2[wave] = second; bn[wave] = mine_nr; }
        __syncthreads();
        if (threadIdx.x == 0) {
            Best b{bv[0], bi[0]};
            float s2 = b2[0];
            int nr = bn[0];
            for (int q = 1; q < 4; ++q) {
                const Best o{bv[q], bi[q]};
                s2 = second_merge(b.v, nr, s2, o.v, bn[q], b2[q]);
                if (better_takes_second(b, o)) { b = o; nr = bn[q]; }
            }
            part_v[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = b.v;
            part_i[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = b.i;
            if (part_s) part_s[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = s2;
            if (part_n) part_n[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = nr;
        }
    }
}
}  // namespace

void score_candidates(int64_t *hist, const int64_t *hist_prev, const int32_t *sub_par, const int32_t *sub_sib, int n_nodes, int Fp, int NB,
                      int D, const FeatureSlot *slots, int n_slots,
                      const float *thr, int B, int n_cand, int min_data, int cosine, const StepScales *sc,
                      const int32_t *path_len, const int32_t *path_slot, const float *path_val, const int32_t *path_bin,
                      float *scores, float *parent, const float *cand_w, const int32_t *cand_ref, const int32_t *is_root, float *part_v,
                      int32_t *part_i, hipStream_t s, int slot0, bool keep_derived, float *part_s, int32_t *part_n, int32_t *cand_nr) {
    const size_t lds = static_cast<size_t>(NB + 2) * (D + 1) * sizeof(int64_t);   // class sums, the totals, the totals as doubles
    static PerDeviceOnce attr_set;
    if (attr_set.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_score), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    }
    hipLaunchKernelGGL(k_score, dim3(n_slots, n_nodes), dim3(256), lds, s, hist, hist_prev, sub_par, sub_sib, Fp, NB, D, slots, thr, B, n_cand, min_data,
                       cosine, sc, path_len, path_slot, path_val, path_bin, scores, parent, cand_w, cand_ref, is_root, part_v, part_i, slot0,
                       keep_derived ? 1 : 0, part_s, part_n, cand_nr);
}

namespace {

// Two stages: stage 1 (many blocks) reduces a slice of the candidates; the per-block bests are reduced by k_resolve_splits.
constexpr int kArgmaxThreads = 256;
__global__ __launch_bounds__(kArgmaxThreads) void k_argmax_stage1(const float *__restrict__ scores, int n_nodes, int n_cand,
                                                                  const float *__restrict__ w, const int32_t *__restrict__ ref,
                                                                  const float *__restrict__ parent, const int32_t *__restrict__ is_root,
                                                                  int oblivious, float *__restrict__ part_v, int32_t *__restrict__ part_i,
                                                                  float *__restrict__ part_s /*nullable: second-best distinct score per block*/) {
    const int j = blockIdx.x * kArgmaxThreads + threadIdx.x;
    const int node = blockIdx.y;
    Best mine{-INFINITY, 0x7fffffff};
    if (j < n_cand) {
        float sc;
        if (oblivious) {   // sum over nodes in node order, fp32, then * w (fitter.cpp:426-435)
            sc = 0.0f;
            int nd = 0;
            for (; nd + 8 <= n_nodes; nd += 8) {      // eight loads in flight, added in node order
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = scores[static_cast<size_t>(nd + u) * n_cand + j];
#pragma unroll
                for (int u = 0; u < 8; ++u) sc += v[u];
            }
            for (; nd < n_nodes; ++nd) sc += scores[static_cast<size_t>(nd) * n_cand + j];
            sc = sc * w[j];
        } else {           // fma(score, w, -parent): the reference's "score*w - parent" is contracted (fitter.cpp:332)
            const float par = is_root[node] ? 0.0f : parent[node];
            sc = fmaf(scores[static_cast<size_t>(node) * n_cand + j], w[j], -par);
        }
        mine = better(mine, Best{sc, ref[j]});
    }
    __shared__ float sv[kArgmaxThreads], s2[kArgmaxThreads];
    __shared__ int si[kArgmaxThreads];
    sv[threadIdx.x] = mine.v;
    si[threadIdx.x] = mine.i;
    s2[threadIdx.x] = -INFINITY;
    __syncthreads();
    for (int o = kArgmaxThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            Best a2{sv[threadIdx.x], si[threadIdx.x]}, b2{sv[threadIdx.x + o], si[threadIdx.x + o]};
            s2[threadIdx.x] = second_distinct(a2.v, s2[threadIdx.x], b2.v, s2[threadIdx.x + o]);
            a2 = better(a2, b2);
            sv[threadIdx.x] = a2.v;
            si[threadIdx.x] = a2.i;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part_v[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = sv[0];
        part_i[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = si[0];
        if (part_s) part_s[static_cast<size_t>(node) * gridDim.x + blockIdx.x] = s2[0];
    }
}
}  // namespace

int argmax_parts(int n_cand) { return (n_cand + kArgmaxThreads - 1) / kArgmaxThreads; }
void argmax(const float *scores, int n_nodes, int n_cand, const float *w, const int32_t *ref, const float *parent,
            const int32_t *is_root, bool oblivious, float *part_v, int32_t *part_i, int32_t *best_idx, float *best_score,
            hipStream_t s, float *part_s) {
    const int parts = argmax_parts(n_cand);
    const int out_nodes = oblivious ? 1 : n_nodes;
    hipLaunchKernelGGL(k_argmax_stage1, dim3(parts, out_nodes), dim3(kArgmaxThreads), 0, s, scores, n_nodes, n_cand, w, ref, parent,
                       is_root, oblivious ? 1 : 0, part_v, part_i, part_s);
    (void)best_idx; (void)best_score;   // published by k_resolve_splits, which runs the last reduction stage itself
}

namespace {

// Child sizes of the selected split of every active node, straight from the histograms (one wave per node), so that the
// host learns the winner AND the sizes of its children with a single read-back.  counts4 = [total_local | right_local |
// total_global | right_global], each max_front wide.
__global__ __launch_bounds__(64) void k_resolve_splits(const float *__restrict__ part_v, const int32_t *__restrict__ part_i, int n_parts,
                                                       int32_t *__restrict__ best_idx, float *__restrict__ best_score, int oblivious,
                                                       const int32_t *__restrict__ ref_to_internal, const int32_t *__restrict__ cand_slot,
                                                       const FeatureSlot *__restrict__ slots, const int64_t *__restrict__ hist_local,
                                                       const int64_t *__restrict__ hist_global, int Fp, int NB, int D,
                                                       NodeSplit *__restrict__ out, int64_t *__restrict__ counts4, int max_front,
                                                       const int32_t *__restrict__ seg_start /*nullable*/, int32_t *__restrict__ cursors,
                                                       const uint32_t *__restrict__ thr_keys, int B, char *pub, uint32_t *pub_flag,
                                                       uint32_t pub_seq, unsigned *pub_done, const int64_t *__restrict__ hist_prev,
                                                       const int32_t *__restrict__ sub_par, const int32_t *__restrict__ sub_sib,
                                                       const float *__restrict__ part_s, const int32_t *__restrict__ part_n /*nullable: oblivious levels*/, float near_rel, const float *__restrict__ parent,
                                                       const int32_t *__restrict__ is_root, int cosine_score, long long near_rows) {
    const int node = blockIdx.x;
    // pub != nullptr: the result block [best_idx | best_score | counts4] is mirrored into pinned, device-mapped host memory of the same
    // layout and the LAST block to finish stores pub_seq to pub_flag (system scope) -- the host polls it (no publishing launch)
    int32_t *pub_idx = reinterpret_cast<int32_t *>(pub);
    float *pub_score = reinterpret_cast<float *>(pub + 4 * static_cast<size_t>(max_front));
    int64_t *pub_counts = reinterpret_cast<int64_t *>(pub + 8 * static_cast<size_t>(max_front));
    // final stage of the argmax (same total order as stage 1: higher score, then lower reference index): every block
    // reduces the per-block bests of its node (oblivious: of the level); the owner block publishes them for the host
    const int src_node = oblivious ? 0 : node;
    Best mine{-INFINITY, 0x7fffffff};
    float second = -INFINITY;
    int mine_nr = 0;          // (oblivious levels carry no child sizes: every candidate's is 0 and only the gains tell classes apart)
    for (int q = threadIdx.x; q < n_parts; q += kWave) {
        const Best other{part_v[static_cast<size_t>(src_node) * n_parts + q], part_i[static_cast<size_t>(src_node) * n_parts + q]};
        if (part_s) {
            const int onr = part_n ? part_n[static_cast<size_t>(src_node) * n_parts + q] : 0;
            second = second_merge(mine.v, mine_nr, second, other.v, onr, part_s[static_cast<size_t>(src_node) * n_parts + q]);
            if (better_takes_second(mine, other)) mine_nr = onr;
        }
        mine = better(mine, other);
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const Best other{__shfl_xor(mine.v, o, kWave), __shfl_xor(mine.i, o, kWave)};
        if (part_s) {
            const int onr = __shfl_xor(mine_nr, o, kWave);
            second = second_merge(mine.v, mine_nr, second, other.v, onr, __shfl_xor(second, o, kWave));
            if (better_takes_second(mine, other)) mine_nr = onr;
        }
        mine = better(mine, other);
    }
    const int best = mine.i == 0x7fffffff ? 0 : mine.i;
    const float best_v = mine.v;
    // near-tie flag (one GPU, counts4's third array is free there): the runner-up -- the best DISTINCT gain -- is within near_rel of the
    // winner, relative to the scores' magnitude, or (greedy) the winning gain is that close to zero, where "split" and "leaf" part
    // (fitter.cpp:357).  The host then has the few candidates in the window re-scored in the reference's float32 order (neartie.hip).
    if (threadIdx.x == 0 && node == src_node && !hist_global) {
        counts4[3 * static_cast<size_t>(max_front) + node] = __float_as_int(second);   // (diagnostics: GBRL_HIP_NEARTIE_DEBUG prints it)
        if (pub) pub_counts[3 * static_cast<size_t>(max_front) + node] = __float_as_int(second);
    }
    if (threadIdx.x == 0 && node == src_node) {
        best_idx[node] = best; best_score[node] = best_v;
        if (pub) { pub_idx[node] = best; pub_score[node] = best_v; }
    }
    const int j = ref_to_internal[best];
    const int fs = cand_slot[j];
    const FeatureSlot sl = slots[fs];
    const int bin = sl.is_cat ? (j - sl.cand_base + 1) : (j - sl.cand_base);
    const int W = D + 1;
    const int NBe = min(NB, sl.n_cand + 1);   // classes of the winner's slot (k_score wrote / derived only those)
    int n_left = 0;
    for (int pass = 0; pass < (hist_global ? 2 : 1); ++pass) {
        const int64_t *src = (pass ? hist_global : hist_local) + (static_cast<size_t>(node) * Fp + fs) * NB * W;
        // sub_par != nullptr (last level, one GPU): k_score did not write the derived slices back; a derived node's counts are
        // parent - sibling here as well (sub_sib < 0: the sibling has no rows)
        const int par = (sub_par && pass == 0) ? sub_par[node] : -1;
        const int64_t *sub = nullptr;
        if (par >= 0) {
            const int sib = sub_sib[node];
            src = hist_prev + (static_cast<size_t>(par) * Fp + fs) * NB * W;
            sub = sib >= 0 ? hist_local + (static_cast<size_t>(sib) * Fp + fs) * NB * W : nullptr;
        }
        long long tot = 0, right = 0;
        for (int c0 = threadIdx.x; c0 < NBe; c0 += 8 * kWave) {     // the class counts of the winner's slice: eight loads in flight per lane
            long long n[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int c = c0 + u * kWave; n[u] = c < NBe ? src[c * W + D] : 0; }
            if (sub) {
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int c = c0 + u * kWave; n[u] -= c < NBe ? sub[c * W + D] : 0; }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = c0 + u * kWave;
                tot += n[u];
                if (c < NBe && (sl.is_cat ? (c == bin) : (c > bin))) right += n[u];
            }
        }
        for (int o = kWave / 2; o > 0; o >>= 1) { tot += __shfl_xor(tot, o, kWave); right += __shfl_xor(right, o, kWave); }
        if (threadIdx.x == 0) {
            counts4[(2 * pass + 0) * static_cast<size_t>(max_front) + node] = tot;
            counts4[(2 * pass + 1) * static_cast<size_t>(max_front) + node] = right;
            if (pub) {
                pub_counts[(2 * pass + 0) * static_cast<size_t>(max_front) + node] = tot;
                pub_counts[(2 * pass + 1) * static_cast<size_t>(max_front) + node] = right;
            }
            if (pass == 0) n_left = static_cast<int>(tot - right);
            if (pass == 0 && !hist_global) {
                // near-tie flag (one GPU: counts4's third array is free there): the runner-up -- the best DISTINCT gain -- is within the window of
                // the winner, relative to the scores' magnitude, or (greedy) the winning gain is that close to zero, where "split" and "leaf"
                // part (fitter.cpp:357).  The host then has the candidates in the window re-scored in the reference's float32 order (neartie.hip).
                // A zero gain needs no replay under L2 when the winner sends every row to ONE side: the reference's split score is then its
                // parent score operation for operation (node.cpp:321-376 against split_candidate_generator.cpp:293-320) and its gain is exactly
                // 0 as well.  (Cosine divides by sqrtf in one and by a double sqrt in the other: there the last bit decides, and is replayed.)
                long long near = 0;
                if (part_s && best_v != -INFINITY && node == src_node) {   // (an oblivious level carries ONE flag; the other nodes' words are cleared:
                    float mag;                                               //  row-sharded levels count this rank's right-going rows into them next)
                    if (oblivious) mag = fabsf(best_v);
                    else { const float par = is_root[node] ? 0.0f : parent[node]; mag = fmaxf(fabsf(best_v + par), fabsf(par)); }
                    const float win = near_window_rel(near_rel, oblivious ? near_rows : tot) * mag;
                    if (second != -INFINITY && best_v - second <= win) near = 1;
                    if (!oblivious && !is_root[node] && fabsf(best_v) <= win && !(cosine_score == 0 && (right == 0 || right == tot))) near = 1;
                }
                counts4[2 * static_cast<size_t>(max_front) + node] = near;
                if (pub) pub_counts[2 * static_cast<size_t>(max_front) + node] = near;
            }
        }
    }
    if (threadIdx.x == 0) {
        NodeSplit q{};
        q.fslot = fs; q.bin = bin; q.is_cat = sl.is_cat;
        q.thr_key = (!sl.is_cat && thr_keys) ? thr_keys[static_cast<size_t>(fs) * B + bin] : 0u;
        if (seg_start) {
            // complete descriptor: the partition of this level is enqueued without waiting for the host's read-back.
            // Same decision rule as the host (fitter.cpp:357 greedy: score >= 0; fitter.cpp:458 oblivious: any finite best)
            const float bs = best_v;
            q.do_split = oblivious ? (bs != -INFINITY) : (bs >= 0.0f);
            q.seg_start = seg_start[node];
            q.n_left = n_left;
            cursors[2 * node] = 0;
            cursors[2 * node + 1] = 0;
        }
        out[node] = q;
        if (pub) {
            __threadfence_system();
            if (atomicAdd(pub_done, 1u) == gridDim.x - 1) {
                *pub_done = 0;     // ready for the next launch (launches on one stream do not overlap)
                __hip_atomic_store(pub_flag, pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}
}  // namespace

void resolve_splits(const float *part_v, const int32_t *part_i, int n_parts, int32_t *best_idx, float *best_score, bool oblivious, int n_nodes, const int32_t *ref_to_internal, const int32_t *cand_slot,
                    const FeatureSlot *slots, const int64_t *hist_local, const int64_t *hist_global, int Fp, int NB, int D,
                    NodeSplit *out, int64_t *counts4, int max_front, const int32_t *seg_start, int32_t *cursors, const uint32_t *thr_keys,
                    int B, hipStream_t s, void *pub, uint32_t *pub_flag, uint32_t pub_seq, unsigned *pub_done, const int64_t *hist_prev,
                    const int32_t *sub_par, const int32_t *sub_sib, const NearDetect *near) {
    hipLaunchKernelGGL(k_resolve_splits, dim3(n_nodes), dim3(64), 0, s, part_v, part_i, n_parts, best_idx, best_score, oblivious ? 1 : 0,
                       ref_to_internal, cand_slot, slots, hist_local, hist_global, Fp, NB, D, out, counts4, max_front, seg_start, cursors, thr_keys, B,
                       static_cast<char *>(pub), pub_flag, pub_seq, pub_done, hist_prev, sub_par, sub_sib,
                       near ? near->part_s : nullptr, near ? near->part_n : nullptr, near ? near->rel : 0.0f, near ? near->parent : nullptr, near ? near->is_root : nullptr, near ? near->cosine : 1, near ? near->rows : 0);
}

// ------------------------------------------------------------------------------------------------------------ diagnostics

// gbrl_hip_score_probe: host arrays in, host arrays out -- score_candidates and, on request, argmax (the oblivious form, the only one a step
// reaches) and resolve_splits behind it, launched as a step launches them (pub = nullptr).  Every output array goes to the device holding the
// caller's values and comes back afterwards, so a cell no kernel stored keeps them.  Every index a kernel will form is checked here first.
int score_selftest(::gbrl_hip_score_probe_t &p, const char **why) {
    const auto refuse = [&](const char *text) { *why = text; return static_cast<int>(kHistProbeInvalid); };
    *why = "";
    const int NB = p.n_classes, D = p.output_dim, W = D + 1, Fp = p.Fp, B = p.B, n_cand = p.n_cand, n_nodes = p.n_nodes;
    if (p.n_hist_nodes < 1 || p.n_hist_nodes > 4096 || p.n_prev_nodes < 0 || p.n_prev_nodes > 4096 || n_nodes < 1 || n_nodes > p.n_hist_nodes || Fp < 1 || Fp > 4096 || NB < 2 || NB > 65535 ||
        D < 1 || D > 512 || p.n_table_slots < 1 || p.n_table_slots > Fp || B < 1 || B > 65535 || n_cand < 1 || n_cand > (1 << 22) || p.sbits < 0 || p.sbits > 40 || p.min_data < 0 ||
        p.max_front < n_nodes || p.max_front > 65536 || p.n_parts < 0 || p.n_parts > (1 << 20))
        return refuse("score_probe: a size is out of range");
    if (p.do_score < 0 || p.do_score > 2 || (p.do_argmax != 0 && p.do_argmax != 1) || (p.do_resolve != 0 && p.do_resolve != 1) || (p.do_score == 2 && p.do_argmax) ||
        (p.do_score == 2 && p.oblivious) || (p.do_argmax && !p.oblivious && p.do_resolve))
        return refuse("score_probe: do_score is 0, 1 or 2, do_argmax and do_resolve 0 or 1; the fused greedy form has no argmax stage and argmax is the oblivious form");
    if (static_cast<size_t>(NB + 2) * W * sizeof(int64_t) > 150 * 1024) return refuse("score_probe: (n_classes + 2) x (output_dim + 1) x 8 bytes does not fit the LDS");
    const size_t node_elems = static_cast<size_t>(Fp) * NB * W;
    if (node_elems * std::max(p.n_hist_nodes, p.n_prev_nodes) > (size_t{1} << 28) || static_cast<size_t>(n_nodes) * n_cand > (size_t{1} << 26))
        return refuse("score_probe: a size is out of range");
    if (!p.hist || !p.slots || !p.thr || !p.path_len || !p.path_slot || !p.path_bin || !p.path_val || !p.cand_w || !p.cand_ref || !p.ref_to_internal || !p.cand_slot || !p.is_root ||
        !p.parent)
        return refuse("score_probe: null array");
    const bool uses_parts = p.do_score == 2 || p.do_argmax || p.do_resolve;
    if ((p.do_score == 1 || p.do_argmax) && !p.scores) return refuse("score_probe: null array");
    if (uses_parts && (!p.part_v || !p.part_i || p.n_parts < 1)) return refuse("score_probe: null array");
    if (p.part_n && !p.part_s) return refuse("score_probe: part_n needs part_s");
    if (p.do_resolve && (!p.best_idx || !p.best_score || !p.counts4 || !p.splits || !p.cursors)) return refuse("score_probe: null array");
    if (p.do_resolve && p.near && !p.part_s) return refuse("score_probe: near-tie detection needs part_s");
    if (p.slot0 < 0 || p.n_slots < 1 || p.n_slots > p.n_table_slots - p.slot0) return refuse("score_probe: the launch window leaves the slot table");
    if (p.do_score == 2 && p.n_parts != p.n_slots) return refuse("score_probe: n_parts must be n_slots after the fused greedy form");
    if (p.do_argmax && p.n_parts != argmax_parts(n_cand)) return refuse("score_probe: n_parts must be ceil(n_cand / 256) after argmax");
    for (int f = 0; f < p.n_table_slots; ++f) {
        const int32_t is_cat = p.slots[4 * f], nc = p.slots[4 * f + 1], base = p.slots[4 * f + 2];
        if ((is_cat != 0 && is_cat != 1) || nc < 0 || base < 0 || base > n_cand || nc > n_cand - base) return refuse("score_probe: a slot's candidates leave [0, n_cand)");
        if (nc + 1 > NB || (!is_cat && nc > B)) return refuse("score_probe: a slot has more candidates than classes or thresholds");
    }
    if (p.sub_par) {
        if (!p.sub_sib) return refuse("score_probe: sub_par without sub_sib");
        for (int k = 0; k < n_nodes; ++k) {
            if (p.sub_par[k] >= 0 && (!p.hist_prev || p.sub_par[k] >= p.n_prev_nodes)) return refuse("score_probe: sub_par names a node outside hist_prev");
            if (p.sub_par[k] >= 0 && p.sub_sib[k] >= p.n_hist_nodes) return refuse("score_probe: sub_sib names a node outside hist");
        }
    }
    for (int k = 0; k < n_nodes; ++k)
        if (p.path_len[k] < 0 || p.path_len[k] > kMaxPath) return refuse("score_probe: path_len above 32");
    {
        std::vector<char> seen(n_cand, 0);
        for (int j = 0; j < n_cand; ++j) {
            const int32_t r = p.cand_ref[j];
            if (r < 0 || r >= n_cand || seen[r]) return refuse("score_probe: cand_ref is no permutation of [0, n_cand)");
            seen[r] = 1;
        }
    }
    for (int j = 0; j < n_cand; ++j) {
        const int32_t i = p.ref_to_internal[j], f = p.cand_slot[j];
        if (i < 0 || i >= n_cand) return refuse("score_probe: ref_to_internal leaves [0, n_cand)");
        if (f < 0 || f >= p.n_table_slots || j < p.slots[4 * f + 2] || j >= p.slots[4 * f + 2] + p.slots[4 * f + 1]) return refuse("score_probe: cand_slot does not name the slot that holds the candidate");
    }
    const size_t n_part = uses_parts ? static_cast<size_t>(n_nodes) * p.n_parts : 0;
    if (p.do_resolve && p.do_score != 2 && !p.do_argmax) {   // part_* as given: an index that can win must be a candidate
        const int rows_read = p.oblivious ? 1 : n_nodes;
        for (size_t q = 0; q < static_cast<size_t>(rows_read) * p.n_parts; ++q)
            if ((p.part_i[q] < 0 || p.part_i[q] >= n_cand) && !(p.part_i[q] == 0x7fffffff && p.part_v[q] == -INFINITY)) return refuse("score_probe: a given part_i is no candidate");
    }

    // ---- device half
    struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } };
    const auto up = [](Dev &d, const void *src, size_t bytes) {
        if (hipMalloc(&d.p, std::max<size_t>(16, bytes)) != hipSuccess) { (void)hipGetLastError(); return false; }
        return !src || bytes == 0 || hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    const auto down = [](void *dst, const Dev &d, size_t bytes) { return !dst || bytes == 0 || hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    Dev dhist, dprev, dglob, dpar, dsib, dslots, dthr, dkeys, dplen, dpslot, dpbin, dpval, dw, dref, dr2i, dcslot, droot, dseg, dsc, dscores, dparent, dpv, dps, dbs, dnr, dpi, dpn, dbi,
        dsplits, dcur, dcnt;
    StepScales sc{};
    sc.inv_scale = std::ldexp(1.0, -p.sbits); sc.leaf_scale = 1.0; sc.scale = std::ldexp(1.0f, p.sbits); sc.sbits = p.sbits;
    const size_t nk = static_cast<size_t>(n_nodes), n_sc = nk * n_cand, mf = static_cast<size_t>(p.max_front);
    bool ok = up(dhist, p.hist, 8 * node_elems * p.n_hist_nodes) && (!p.hist_prev || up(dprev, p.hist_prev, 8 * node_elems * p.n_prev_nodes)) &&
              (!p.hist_global || up(dglob, p.hist_global, 8 * node_elems * nk)) && (!p.sub_par || (up(dpar, p.sub_par, 4 * nk) && up(dsib, p.sub_sib, 4 * nk))) &&
              up(dslots, p.slots, sizeof(FeatureSlot) * p.n_table_slots) && up(dthr, p.thr, 4 * static_cast<size_t>(p.n_table_slots) * B) &&
              (!p.thr_keys || up(dkeys, p.thr_keys, 4 * static_cast<size_t>(p.n_table_slots) * B)) && up(dplen, p.path_len, 4 * nk) && up(dpslot, p.path_slot, 4 * nk * kMaxPath) &&
              up(dpbin, p.path_bin, 4 * nk * kMaxPath) && up(dpval, p.path_val, 4 * nk * kMaxPath) && up(dw, p.cand_w, 4 * static_cast<size_t>(n_cand)) &&
              up(dref, p.cand_ref, 4 * static_cast<size_t>(n_cand)) && up(dr2i, p.ref_to_internal, 4 * static_cast<size_t>(n_cand)) && up(dcslot, p.cand_slot, 4 * static_cast<size_t>(n_cand)) &&
              up(droot, p.is_root, 4 * nk) && (!p.seg_start || up(dseg, p.seg_start, 4 * nk)) && up(dsc, &sc, sizeof(sc)) && (!p.scores || up(dscores, p.scores, 4 * n_sc)) &&
              up(dparent, p.parent, 4 * nk) && (!p.cand_nr || up(dnr, p.cand_nr, 4 * n_sc)) && (!n_part || (up(dpv, p.part_v, 4 * n_part) && up(dpi, p.part_i, 4 * n_part))) &&
              (!n_part || !p.part_s || up(dps, p.part_s, 4 * n_part)) && (!n_part || !p.part_n || up(dpn, p.part_n, 4 * n_part));
    if (ok && p.do_resolve)
        ok = up(dbi, p.best_idx, 4 * mf) && up(dbs, p.best_score, 4 * mf) && up(dcnt, p.counts4, 8 * 4 * mf) && up(dsplits, p.splits, sizeof(NodeSplit) * nk) && up(dcur, p.cursors, 8 * nk);
    if (!ok) return kHistProbeDevice;
    const auto ran = [] { const bool good = hipGetLastError() == hipSuccess /* a refused launch */ && hipDeviceSynchronize() == hipSuccess; if (!good) (void)hipGetLastError(); return good; };
    const FeatureSlot *slots = static_cast<const FeatureSlot *>(dslots.p);
    const bool greedy = p.do_score == 2;
    if (p.do_score) {
        score_candidates(static_cast<int64_t *>(dhist.p), static_cast<const int64_t *>(dprev.p), static_cast<const int32_t *>(dpar.p), static_cast<const int32_t *>(dsib.p), n_nodes, Fp, NB, D,
                         slots, p.n_slots, static_cast<const float *>(dthr.p), B, n_cand, p.min_data, p.cosine ? 1 : 0, static_cast<const StepScales *>(dsc.p),
                         static_cast<const int32_t *>(dplen.p), static_cast<const int32_t *>(dpslot.p), static_cast<const float *>(dpval.p), static_cast<const int32_t *>(dpbin.p),
                         static_cast<float *>(dscores.p), static_cast<float *>(dparent.p), static_cast<const float *>(dw.p), static_cast<const int32_t *>(dref.p),
                         static_cast<const int32_t *>(droot.p), greedy ? static_cast<float *>(dpv.p) : nullptr, static_cast<int32_t *>(dpi.p), nullptr, p.slot0, p.keep_derived != 0,
                         greedy ? static_cast<float *>(dps.p) : nullptr, greedy ? static_cast<int32_t *>(dpn.p) : nullptr, greedy ? nullptr : static_cast<int32_t *>(dnr.p));
        if (!ran()) return kHistProbeDevice;
    }
    if (p.do_argmax) {
        argmax(static_cast<const float *>(dscores.p), n_nodes, n_cand, static_cast<const float *>(dw.p), static_cast<const int32_t *>(dref.p), static_cast<const float *>(dparent.p),
               static_cast<const int32_t *>(droot.p), true, static_cast<float *>(dpv.p), static_cast<int32_t *>(dpi.p), nullptr, nullptr, nullptr, static_cast<float *>(dps.p));
        if (!ran()) return kHistProbeDevice;
    }
    if (p.do_resolve) {
        const NearDetect near{static_cast<const float *>(dps.p), static_cast<const int32_t *>(dpn.p), p.near_rel, static_cast<const float *>(dparent.p), static_cast<const int32_t *>(droot.p),
                              p.cosine ? 1 : 0, p.near_rows};
        const bool derive = p.keep_derived == 0 && p.sub_par;   // the last level: the derived slices were not written back
        resolve_splits(static_cast<const float *>(dpv.p), static_cast<const int32_t *>(dpi.p), p.n_parts, static_cast<int32_t *>(dbi.p), static_cast<float *>(dbs.p), p.oblivious != 0, n_nodes,
                       static_cast<const int32_t *>(dr2i.p), static_cast<const int32_t *>(dcslot.p), slots, static_cast<const int64_t *>(dhist.p), static_cast<const int64_t *>(dglob.p), Fp, NB, D,
                       static_cast<NodeSplit *>(dsplits.p), static_cast<int64_t *>(dcnt.p), p.max_front, static_cast<const int32_t *>(dseg.p), static_cast<int32_t *>(dcur.p),
                       static_cast<const uint32_t *>(dkeys.p), B, nullptr, nullptr, nullptr, 0, nullptr, derive ? static_cast<const int64_t *>(dprev.p) : nullptr,
                       derive ? static_cast<const int32_t *>(dpar.p) : nullptr, derive ? static_cast<const int32_t *>(dsib.p) : nullptr, p.near ? &near : nullptr);
        if (!ran()) return kHistProbeDevice;
    }
    ok = down(p.hist, dhist, 8 * node_elems * p.n_hist_nodes) && down(p.scores, dscores, 4 * n_sc) && down(p.parent, dparent, 4 * nk) && down(p.cand_nr, dnr, 4 * n_sc);
    if (ok && n_part) ok = down(p.part_v, dpv, 4 * n_part) && down(p.part_i, dpi, 4 * n_part) && down(p.part_s, dps, 4 * n_part) && down(p.part_n, dpn, 4 * n_part);
    if (ok && p.do_resolve)
        ok = down(p.best_idx, dbi, 4 * mf) && down(p.best_score, dbs, 4 * mf) && down(p.counts4, dcnt, 8 * 4 * mf) && down(p.splits, dsplits, sizeof(NodeSplit) * nk) && down(p.cursors, dcur, 8 * nk);
    return ok ? kHistProbeOk : kHistProbeDevice;
}

}  // namespace kern
}  // namespace gbrl
