// gram_core.h -- the rule behind GBRL::tree_gram_prepared / gbrl_cpp.tree_gram_host, host-compilable (no device code, no HIP header):
//
//   gram[t][u] = sum over rows r, outputs d of v_t(r, d) * v_u(r, d)        moment[t] = sum over rows r, outputs d of v_t(r, d) * y(r, d)
//
// v_t(r, :) is the stored float32 value row of the leaf tree t routes row r to (all zeros where a greedy search runs off the ensemble).  A float32
// converts to float64 exactly and the product of two such values is exact in float64 (48 significand bits), so only the additions round.  Two
// bounds follow, for two different quantities, terms = rows * D:
//   against the EXACT sum   every evaluation below -- whatever its order -- lies within (terms - 1) * 2^-53 * sum |v_t v_u| of it (include/gbrl_hip.h
//                           states the rounder terms * 2^-53);
//   between TWO evaluations (the streaming kernel, the general kernel, the host rule, NumPy) the worst case is twice that.  The tests hold every
//                           pair to the tighter (terms + 8) * 2^-53 * sum |v_t v_u| all the same: the worst case needs every rounding of both
//                           sides to fall the opposite way, and the measured distances stay under a quarter of it.
//
//   gram_plan        the launch plan of tree_gram.hip, a pure function of (m, T, D) -- and of the data set's width, which only decides whether
//                    the streaming kernel's LDS fits.  Trees are cut into chunks of kGramChunk; a block owns one chunk pair (a <= b) and every
//                    row_blocks-th 64-row tile, and writes its partial kGramChunk x kGramChunk tile to scratch [row_blocks][pairs][chunk][chunk]
//                    (+ [row_blocks][chunks][chunk] moments).  row_blocks is the largest count that keeps that scratch under kGramScratchBudget
//                    (pd_core.h's 64 MiB figure), at most kGramMaxRowBlocks and at most the tile count.
//   gram_pair_index  where the pair (a, b), a <= b, lies in the pair list: (0,0) (0,1) .. (0,C-1) (1,1) ..
//   gram_host_rule   the reference evaluation: plain float64 loops, rows in order, then outputs; the upper triangle mirrored.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gbrl {
namespace kern {

constexpr int kGramChunk = 64;                                // trees per chunk: a 4 x 4 grid of 16 x 16 MFMA blocks per chunk pair
constexpr int kGramTileRows = 64;                             // rows per tile (predict_rowwalk.h's kStreamRows) = the K of one operand slab
constexpr int kGramOpStride = kGramTileRows + 1;              // doubles per operand row in LDS: odd, so 16 trees at one k meet 16 distinct bank pairs
constexpr int kGramMaxTrees = 2048;                           // the float64 Gram is 32 MiB there
constexpr int kGramMaxD = 128;
constexpr int kGramMaxRowBlocks = 512;
constexpr size_t kGramScratchBudget = size_t(64) << 20;       // bytes of partials one call may write (pd_core.h: kPdScratchBudget)
constexpr size_t kGramLdsBudget = 156 * 1024;                 // leaf_accum.h: kStreamLdsBudget
constexpr int kGramBadValue = 1, kGramBadTarget = 2;          // bits of the status word

struct GramPlan {
    int chunk, chunks, pairs, tiles, row_blocks;
    size_t per_block;       // doubles one row block writes: pairs * chunk^2 Gram entries, then chunks * chunk moments
    size_t scratch_bytes;   // row_blocks * per_block * 8
    size_t lds_bytes;       // the streaming kernel's dynamic LDS: code tile, one or two operands, one slab of targets
    int streaming;          // 0: the LDS does not fit, the general kernel takes the call
};

inline GramPlan gram_plan(long long m, int T, int D, int groups) {
    GramPlan p{};
    (void)D;   // (K is consumed in slabs of one output: D changes the time, not the geometry)
    p.chunk = kGramChunk;
    p.chunks = (std::max(T, 1) + kGramChunk - 1) / kGramChunk;
    p.pairs = p.chunks * (p.chunks + 1) / 2;
    p.tiles = static_cast<int>((std::max<long long>(m, 1) + kGramTileRows - 1) / kGramTileRows);
    p.per_block = static_cast<size_t>(p.pairs) * kGramChunk * kGramChunk + static_cast<size_t>(p.chunks) * kGramChunk;
    const size_t fit = kGramScratchBudget / (p.per_block * sizeof(double));
    p.row_blocks = static_cast<int>(std::max<size_t>(1, std::min<size_t>({static_cast<size_t>(p.tiles), static_cast<size_t>(kGramMaxRowBlocks), fit})));
    p.scratch_bytes = static_cast<size_t>(p.row_blocks) * p.per_block * sizeof(double);
    const size_t tile = static_cast<size_t>(kGramTileRows) * ((static_cast<size_t>(std::max(groups, 0)) * 8) | 1) * sizeof(uint32_t);
    const size_t ops = static_cast<size_t>(p.chunks > 1 ? 2 : 1) * kGramChunk * kGramOpStride * sizeof(double);
    p.lds_bytes = tile + ops + kGramTileRows * sizeof(double);
    p.streaming = groups >= 1 && p.lds_bytes <= kGramLdsBudget;
    return p;
}

inline int gram_pair_index(int a, int b, int chunks) { return a * chunks - a * (a - 1) / 2 + (b - a); }

// leaf_of(r, t) -> global leaf of (row r, tree t of the range), < 0: none.  values [n_leaves][D]; y [n][D] or null; gram [T][T]; moment [T] or null.
// Returns the status bits (kGramBadValue: a non-finite leaf value was met; kGramBadTarget: a non-finite target).
template <typename LeafOf>
int gram_host_rule(int n, int T, int D, const float *values, LeafOf &&leaf_of, const float *y, double *gram, double *moment) {
    int status = 0;
    std::fill(gram, gram + static_cast<size_t>(T) * T, 0.0);
    if (moment) std::fill(moment, moment + T, 0.0);
    std::vector<const float *> v(static_cast<size_t>(T));
    for (int r = 0; r < n; ++r) {
        for (int t = 0; t < T; ++t) {
            const int leaf = leaf_of(r, t);
            v[t] = leaf >= 0 ? values + static_cast<size_t>(leaf) * D : nullptr;
            for (int d = 0; v[t] && d < D; ++d)
                if (!std::isfinite(v[t][d])) status |= kGramBadValue;
        }
        const float *yr = y ? y + static_cast<size_t>(r) * D : nullptr;
        for (int d = 0; yr && d < D; ++d)
            if (!std::isfinite(yr[d])) status |= kGramBadTarget;
        for (int t = 0; t < T; ++t) {
            if (!v[t]) continue;
            double *g = gram + static_cast<size_t>(t) * T;
            for (int u = t; u < T; ++u) {
                if (!v[u]) continue;
                double s = g[u];
                for (int d = 0; d < D; ++d) s += static_cast<double>(v[t][d]) * static_cast<double>(v[u][d]);
                g[u] = s;
            }
            if (yr) {
                double s = moment[t];
                for (int d = 0; d < D; ++d) s += static_cast<double>(v[t][d]) * static_cast<double>(yr[d]);
                moment[t] = s;
            }
        }
    }
    for (int t = 0; t < T; ++t)
        for (int u = t + 1; u < T; ++u) gram[static_cast<size_t>(u) * T + t] = gram[static_cast<size_t>(t) * T + u];
    return status;
}

// the Gram and the moments from the reduced chunk-pair tiles [pairs][chunk][chunk] (+ [chunks][chunk]): the upper triangle, mirrored
inline void gram_assemble(const double *tiles, int T, double *gram, double *moment) {
    const int C = (T + kGramChunk - 1) / kGramChunk;
    const size_t tile = static_cast<size_t>(kGramChunk) * kGramChunk;
    for (int t = 0; t < T; ++t)
        for (int u = t; u < T; ++u) {
            const int a = t / kGramChunk, b = u / kGramChunk;
            const double g = tiles[gram_pair_index(a, b, C) * tile + static_cast<size_t>(t % kGramChunk) * kGramChunk + (u % kGramChunk)];
            gram[static_cast<size_t>(t) * T + u] = g;
            gram[static_cast<size_t>(u) * T + t] = g;
        }
    if (moment) {
        const double *mo = tiles + static_cast<size_t>(C) * (C + 1) / 2 * tile;
        for (int t = 0; t < T; ++t) moment[t] = mo[t];   // ([chunks][chunk] is the trees in order)
    }
}

}  // namespace kern
}  // namespace gbrl
