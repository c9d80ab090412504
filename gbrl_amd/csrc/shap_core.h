// shap_core.h -- the host half of SHAP values on a prepared data set (engine_explain.hip calls it, shap.hip has the kernels; no device and no HIP
// header is needed: tests/cxx/shap_core_check.cpp compiles it alone and checks every rule against a plain loop).
//
// The reduction rule.  phi is float32 [m][C], C = F * D columns, row p = position p of the row list.  Positions fall into tiles t = p / 64.  For a
// column c a tile's partial is the sequential float64 sum, from 0.0, ascending in p, of (double)phi[p][c]; a second partial does the same with
// fabs of the float32.  The total of a column is the sequential ascending sum of its tile partials from 0.0.  Additions only: nothing can contract
// into a fused multiply-add, and the pragma keeps it so.  The tile is the unit: a total does not depend on how the tiles were cut into launches.
//   shap_tile_sums     one tile of one column (host and device: k_shap_tile_sums is a loop of calls)
//   shap_finish_sums   the total of one column from its tile partials (host and device: k_shap_finish)
//   shap_sums_host     the whole rule on a host matrix (gbrl_hip_shap_sums_host)
// A NaN or an infinity in a column propagates into that column's two totals by IEEE addition (fabs of a NaN is a NaN); no other column sees it.
//
// The chunk plan.  shap_importance_prepared evaluates chunk_rows positions at a time into a float32 scratch [chunk_rows][C] and reduces every
// chunk to its tile partials in a buffer [tiles][2][C] before the scratch is reused.  chunk_rows is a positive multiple of 64; its default is the
// largest multiple of 64 whose scratch stays within kShapScratchBudget (64 MiB, partial dependence's budget), and at least 64.  The scratch that
// is allocated never exceeds the rows of the call rounded up to a tile.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_SHAP_HD __host__ __device__
#else
#define GBRL_SHAP_HD
#endif

namespace gbrl {
namespace kern {

constexpr int kShapTileRows = 64;                            // positions per float64 partial
constexpr size_t kShapScratchBudget = size_t(64) << 20;      // bytes of float32 scratch one chunk may fill (= kPdScratchBudget)

// rows [0, rows) of one column: col[r * stride]
GBRL_SHAP_HD inline void shap_tile_sums(const float *col, size_t stride, int rows, double *sum, double *sum_abs) {
#pragma clang fp contract(off)
    double s = 0.0, a = 0.0;
    for (int r = 0; r < rows; ++r) {
        const float v = col[static_cast<size_t>(r) * stride];
        s = s + static_cast<double>(v);
        a = a + static_cast<double>(__builtin_fabsf(v));
    }
    *sum = s;
    *sum_abs = a;
}

// the partials of one column: part[t * stride], t ascending
GBRL_SHAP_HD inline double shap_finish_sums(const double *part, size_t stride, int tiles) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s = s + part[static_cast<size_t>(t) * stride];
    return s;
}

inline int shap_tiles(long long m) { return static_cast<int>((m + kShapTileRows - 1) / kShapTileRows); }

// phi [m][C] on the host -> sum_out [C], abs_out [C]
inline void shap_sums_host(const float *phi, long long m, size_t C, double *sum_out, double *abs_out) {
#pragma clang fp contract(off)
    const int tiles = shap_tiles(m);
    for (size_t c = 0; c < C; ++c) {
        double total = 0.0, total_abs = 0.0;
        for (int t = 0; t < tiles; ++t) {
            const long long p0 = static_cast<long long>(t) * kShapTileRows;
            double s, a;
            shap_tile_sums(phi + static_cast<size_t>(p0) * C + c, C, static_cast<int>(std::min<long long>(kShapTileRows, m - p0)), &s, &a);
            total = total + s;
            total_abs = total_abs + a;
        }
        sum_out[c] = total;
        abs_out[c] = total_abs;
    }
}

// the largest multiple of 64 rows whose float32 scratch [rows][F * D] stays within the budget, and at least 64
inline int shap_default_chunk_rows(int F, int D, size_t budget = kShapScratchBudget) {
    const unsigned long long row_bytes = sizeof(float) * static_cast<unsigned long long>(F < 1 ? 1 : F) * static_cast<unsigned long long>(D < 1 ? 1 : D);
    unsigned long long rows = budget / row_bytes;
    rows -= rows % kShapTileRows;
    return static_cast<int>(std::min<unsigned long long>(std::max<unsigned long long>(rows, kShapTileRows), 0x7fffffc0ull));
}

struct ShapChunkPlan {
    int chunk_rows;          // positions per chunk: the caller's, or the default (the value reported)
    int alloc_rows;          // rows of scratch allocated: min(chunk_rows, m rounded up to a tile)
    int n_chunks, tiles;     // launches of the evaluation, float64 partials per column and kind
    size_t scratch_bytes;    // float32 [alloc_rows][F * D]
    size_t partial_bytes;    // float64 [tiles][2][F * D]
};

// chunk_rows == 0: the default.  The caller has checked chunk_rows (shap_chunk_rows_error) and m >= 1.
inline ShapChunkPlan shap_chunk_plan(long long m, int F, int D, int chunk_rows) {
    ShapChunkPlan p{};
    const size_t C = static_cast<size_t>(F) * static_cast<size_t>(D);
    p.chunk_rows = chunk_rows > 0 ? chunk_rows : shap_default_chunk_rows(F, D);
    p.tiles = shap_tiles(m);
    p.alloc_rows = static_cast<int>(std::min<long long>(p.chunk_rows, static_cast<long long>(p.tiles) * kShapTileRows));
    p.n_chunks = static_cast<int>((m + p.chunk_rows - 1) / p.chunk_rows);
    p.scratch_bytes = sizeof(float) * static_cast<size_t>(p.alloc_rows) * C;
    p.partial_bytes = sizeof(double) * static_cast<size_t>(p.tiles) * 2 * C;
    return p;
}

// ---- the argument checks that need no device: an empty string, or the refusal's text behind "<call>: "
inline std::string shap_chunk_rows_error(int chunk_rows) {
    if (chunk_rows < 0 || chunk_rows % kShapTileRows != 0)
        return "chunk_rows " + std::to_string(chunk_rows) + " is not a positive multiple of " + std::to_string(kShapTileRows) + " (0 / None: the default)";
    return std::string();
}

inline std::string shap_matrix_error(long long m, int F, int D) {
    if (static_cast<unsigned long long>(m) * static_cast<unsigned long long>(F) * static_cast<unsigned long long>(D) >= (1ull << 31))
        return "the matrix of " + std::to_string(m) + " rows x " + std::to_string(F) + " features x " + std::to_string(D) +
               " outputs has 2^31 elements or more: pass rows= to explain fewer rows, or use shap_importance_prepared";
    return std::string();
}

inline std::string shap_tree_error(int tree_idx, int n_trees) {
    if (n_trees == 0) return "the model has no trees";
    if (tree_idx < -1 || tree_idx >= n_trees)
        return "tree_idx " + std::to_string(tree_idx) + " is outside [0, " + std::to_string(n_trees) + "), the model's trees (None / -1: all)";
    return std::string();
}

}  // namespace kern
}  // namespace gbrl
