// gather_cols.hip -- gfx950 kernels behind the column subsets of a prepared data set (Engine::step_prepared with `cols`, fit_prepared(colsample=),
// gbrl_hip_dataset_codes_cols).
//
// The class codes of a batch are group-major: [group][row][16] u16 (kern::kCodeGroup), one 32-byte record per (group, row).  A subset of the
// columns, ascending, is a compact re-packing of those records into ceil(F' / 16) groups, on which every growth path runs unchanged:
//   k_gather_code_columns     dst[g'][j][i] = src[cols[16 g' + i] / 16][r][cols[16 g' + i] % 16], r = rows ? rows[j] : j; the padding slots of the
//                             last group are zero, as prepare_dataset leaves them.  One wave per block, a block owns a tile of 64 rows.  It
//                             stages the records of the source groups that hold a selected column -- the host lists them (gather_cols_plan) --
//                             with predict_rowwalk.h's staging: 16-byte loads, two lanes per record, into an LDS tile of 8 words per staged group
//                             and row at an odd word stride.  An output half-record (8 codes) is then built by one lane from 8 two-byte LDS
//                             reads through a per-slot offset table (one 16-byte load of 8 u16 offsets, two distinct addresses per wave) and
//                             leaves as one 16-byte store: lane i writes bytes [16 i, 16 i + 16) of a 1 KiB run of the output group, so the
//                             stores are fully coalesced.  The lanes of a 32-lane half read 16 rows x 2 halves: the odd stride keeps the rows on
//                             distinct banks, the two halves of a row may meet (2-way at worst).  A padding slot reads the stride's spare word,
//                             which the block zeroes: no branch per code.
//                             Wide subsets: at most kGatherColsMaxStaged source groups are staged at a time.  The host cuts the OUTPUT groups
//                             into chunks whose source groups fit (an output group touches at most 16 source groups, so every chunk fits and
//                             any F works; a source group on a chunk boundary is staged twice); the block walks the chunks with the tile reused.
//                             There is no other kernel: no shape leaves this one.
//                             Traffic: 32 * Gt * m bytes read (Gt touched groups, + one group per chunk boundary), 4 m of indices, 32 * G' * m
//                             written.
//   k_gather_threshold_rows   out[f'][b] = table[cols[f']][b] for the [F][B] thresholds and their keys, one launch for both.
#include "kernels.h"
#include "predict_rowwalk.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace gbrl {
namespace kern {

namespace {

static_assert(kGatherColsRows == kStreamRows, "the tile is predict_rowwalk.h's: one wave, lane = row");

__global__ __launch_bounds__(kStreamRows) void k_gather_code_columns(const uint16_t *__restrict__ codes, const int32_t *__restrict__ rows, uint4 *__restrict__ dst,
                                                                     const int4 *__restrict__ chunks, const int32_t *__restrict__ groups,
                                                                     const uint4 *__restrict__ offs, int n, int m, int n_chunks) {
    extern __shared__ __align__(16) uint32_t gctile[];   // [kStreamRows][stream_code_stride(staged groups of the chunk)]
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * kStreamRows;
    const int nrows = min(kStreamRows, m - r0);
    const int at = r0 + (lane < nrows ? lane : 0);   // (a lane without a row names the block's first: a valid record, never stored)
    const int my_row = rows ? rows[at] : at;          // checked against [0, n) by the caller
    const int h = lane & 1;
    for (int c = 0; c < n_chunks; ++c) {
        const int4 ch = chunks[c];   // first output group, output groups, first entry of `groups`, staged groups
        const int32_t *gl = groups + ch.z;
        const int ws = stream_code_stride(ch.w);
        stream_stage_code_groups(gctile, codes, static_cast<size_t>(n), ch.w, [gl](int i) { return gl[i]; }, my_row, nrows, lane);
        gctile[lane * ws + ch.w * 8] = 0u;   // the spare word of the row: what a padding slot reads
        __syncthreads();
        for (int g = ch.x; g < ch.x + ch.y; ++g) {
            const uint4 o = offs[2 * g + h];   // u16 offsets of this half-record's 8 codes within a tile row
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int j = pass * (kStreamRows / 2) + (lane >> 1);
                if (j < nrows) {
                    const uint16_t *x = reinterpret_cast<const uint16_t *>(gctile + j * ws);
                    uint4 v;
                    v.x = static_cast<uint32_t>(x[o.x & 0xffffu]) | (static_cast<uint32_t>(x[o.x >> 16]) << 16);
                    v.y = static_cast<uint32_t>(x[o.y & 0xffffu]) | (static_cast<uint32_t>(x[o.y >> 16]) << 16);
                    v.z = static_cast<uint32_t>(x[o.z & 0xffffu]) | (static_cast<uint32_t>(x[o.z >> 16]) << 16);
                    v.w = static_cast<uint32_t>(x[o.w & 0xffffu]) | (static_cast<uint32_t>(x[o.w >> 16]) << 16);
                    dst[((static_cast<size_t>(g) * static_cast<size_t>(m) + static_cast<size_t>(r0 + j)) << 1) + h] = v;
                }
            }
        }
        __syncthreads();   // the tile is staged again for the next chunk
    }
}

__global__ __launch_bounds__(256) void k_gather_threshold_rows(const uint32_t *__restrict__ thr, const uint32_t *__restrict__ keys, const int32_t *__restrict__ cols,
                                                               uint32_t *__restrict__ thr_out, uint32_t *__restrict__ keys_out, int B, size_t n_el) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_el; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const size_t f = i / B, b = i - f * B;
        const size_t src = static_cast<size_t>(cols[f]) * B + b;
        thr_out[i] = thr[src];
        keys_out[i] = keys[src];
    }
}

}  // namespace

GatherColsPlan gather_cols_plan(const int32_t *cols, int n_cols, std::vector<int32_t> &words) {
    constexpr uint16_t kPad = 0xffffu;
    const int Gp = (n_cols + kCodeGroup - 1) / kCodeGroup;
    std::vector<int32_t> chunks, groups;
    std::vector<uint16_t> offs(static_cast<size_t>(Gp) * kCodeGroup, kPad);
    int chunk_g0 = 0, chunk_at = 0;   // the open chunk: its first output group, its first entry of `groups`
    auto close = [&](int g_end) {
        const int n_tg = static_cast<int>(groups.size()) - chunk_at;
        for (int s = chunk_g0 * kCodeGroup; s < g_end * kCodeGroup; ++s)
            if (offs[s] == kPad) offs[s] = static_cast<uint16_t>(n_tg * kCodeGroup);   // the spare word of a tile row
        chunks.insert(chunks.end(), {chunk_g0, g_end - chunk_g0, chunk_at, n_tg});
        chunk_g0 = g_end;
        chunk_at = static_cast<int>(groups.size());
    };
    for (int g = 0; g < Gp; ++g) {
        const int s0 = g * kCodeGroup, s1 = std::min(n_cols, s0 + kCodeGroup);
        // cols ascends, so do the source groups: only the first one can be staged already (the last of the open chunk)
        int fresh = 0;
        for (int s = s0, last = groups.size() > static_cast<size_t>(chunk_at) ? groups.back() : -1; s < s1; ++s) {
            const int sg = cols[s] / kCodeGroup;
            if (sg != last) { ++fresh; last = sg; }
        }
        if (g > chunk_g0 && static_cast<int>(groups.size()) - chunk_at + fresh > kGatherColsMaxStaged) close(g);
        for (int s = s0; s < s1; ++s) {
            const int sg = cols[s] / kCodeGroup;
            if (groups.size() == static_cast<size_t>(chunk_at) || groups.back() != sg) groups.push_back(sg);
            offs[s] = static_cast<uint16_t>((static_cast<int>(groups.size()) - 1 - chunk_at) * kCodeGroup + cols[s] % kCodeGroup);
        }
    }
    close(Gp);
    GatherColsPlan p{};
    p.n_cols = n_cols; p.n_out_groups = Gp; p.n_chunks = static_cast<int>(chunks.size() / 4);
    p.chunks_at = 0;
    p.groups_at = static_cast<int>(chunks.size());
    p.offs_at = (p.groups_at + static_cast<int>(groups.size()) + 3) & ~3;   // read as uint4
    p.cols_at = p.offs_at + Gp * kCodeGroup / 2;
    p.n_words = static_cast<size_t>(p.cols_at) + n_cols;
    for (int c = 0; c < p.n_chunks; ++c) p.max_staged = std::max(p.max_staged, chunks[4 * c + 3]);
    p.staged_groups = groups.size();
    words.assign(p.n_words, 0);
    std::copy(chunks.begin(), chunks.end(), words.begin() + p.chunks_at);
    std::copy(groups.begin(), groups.end(), words.begin() + p.groups_at);
    std::memcpy(words.data() + p.offs_at, offs.data(), offs.size() * sizeof(uint16_t));
    std::copy(cols, cols + n_cols, words.begin() + p.cols_at);
    return p;
}

void gather_code_columns(const uint16_t *codes, int n, const int32_t *rows, int m, const int32_t *d_plan, const GatherColsPlan &p, uint16_t *out, hipStream_t s) {
    if (m <= 0 || p.n_cols <= 0) return;
    const size_t lds = stream_code_tile_bytes(p.max_staged);   // <= 33 KiB: inside the default dynamic LDS
    hipLaunchKernelGGL(k_gather_code_columns, dim3(static_cast<unsigned>((static_cast<size_t>(m) + kStreamRows - 1) / kStreamRows)), dim3(kStreamRows), lds, s, codes,
                       rows, reinterpret_cast<uint4 *>(out), reinterpret_cast<const int4 *>(d_plan + p.chunks_at), d_plan + p.groups_at,
                       reinterpret_cast<const uint4 *>(d_plan + p.offs_at), n, m, p.n_chunks);
}

void gather_threshold_rows(const float *thr, const uint32_t *thr_keys, int B, const int32_t *d_plan, const GatherColsPlan &p, float *thr_out, uint32_t *keys_out,
                           hipStream_t s) {
    const size_t n_el = static_cast<size_t>(p.n_cols) * B;
    if (n_el == 0) return;
    hipLaunchKernelGGL(k_gather_threshold_rows, dim3(static_cast<unsigned>(std::min<size_t>((n_el + 255) / 256, 4096))), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t *>(thr), thr_keys, d_plan + p.cols_at, reinterpret_cast<uint32_t *>(thr_out), keys_out, B, n_el);
}

}  // namespace kern
}  // namespace gbrl
