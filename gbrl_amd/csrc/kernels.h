// kernels.h -- launch wrappers of the gfx950 kernels behind GBRL::step / GBRL::predict.
// Each wrapper enqueues on `stream` and returns immediately; errors surface through hipGetLastError in the engine.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

struct gbrl_hip_score_probe_t;   // include/gbrl_hip.h (diagnostics)
struct gbrl_hip_rows_probe_t;

namespace gbrl {
namespace kern {

// hipFuncSetAttribute (and anything else that is per-device state) must run once per DEVICE, not once per process: one process
// can hold models on several GPUs.  `static PerDeviceOnce once; if (once.first()) hipFuncSetAttribute(...)`.
struct PerDeviceOnce {
    uint64_t done = 0;
    bool first() {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return true;
        if ((done >> d) & 1ull) return false;
        done |= 1ull << d;
        return true;
    }
};


// A contiguous run of positions [start, start+len) of the row list that belongs to one slot (node or leaf).
struct Chunk {
    int32_t slot;
    int32_t start;
    int32_t len;
    int32_t pad;
};

// Descriptor of one feature slot (numeric feature or categorical feature) for the scoring kernel.
struct FeatureSlot {
    int32_t is_cat;     // 0 numeric: candidate k <-> threshold k, right = classes > k; 1 categorical: candidate j <-> class j+1
    int32_t n_cand;     // number of candidates of this slot
    int32_t cand_base;  // index of the slot's first candidate in the global candidate order
    int32_t pad;
};

// Per-node split decision used by the partition kernel.
struct NodeSplit {
    int32_t do_split;   // 0: copy the segment unchanged
    int32_t fslot;      // feature slot of the chosen candidate
    int32_t bin;        // numeric: threshold index k (right <=> code > k); categorical: class id (right <=> code == bin)
    int32_t is_cat;
    int32_t seg_start;  // first position of the node's segment
    int32_t n_left;     // rows going left (right child starts at seg_start + n_left)
    uint32_t thr_key;   // numeric: ordered key of the threshold -- right <=> key(row, feature) > thr_key, read from the
                        // feature-major keys (4 coalesced bytes per row instead of a 32-byte code record)
    int32_t pad1;
};

// Fixed-point scales of one step, derived from the gradient statistics.  They live in device memory so that the whole
// statistics -> scale -> quantisation chain runs without a host round trip (the host reads them once, later).
struct StepScales {
    double inv_scale;   // 2^-sbits : histogram sums -> standardised-gradient units (k_score)
    double leaf_scale;  // 2^lbits  : raw-gradient fixed point of the leaf sums (k_leaf_sums)
    float scale;        // 2^sbits  (k_quantize)
    float hmax_build;   // max |standardised gradient| * 1.0001 (or max |g| for Cosine)
    float hmax_raw;     // max |g|
    int32_t sbits, lbits, pad;
};

constexpr int kMaxPath = 32;
constexpr int kPartitionRows = 4096;  // rows per partition block (chunk size the engine must use)  // max_depth supported by the duplicate-on-path check

// ---- gradient preprocessing (A2) ----
// out[0..D) = sum_i g[i,d] (center == null) or sum_i (g[i,d]-center[d])^2 ; out[D..2D) = max_i |g[i,d] (- center[d])|
// block_partials: n_blocks * 2D doubles.  Deterministic (fixed reduction tree).
void column_sums(const float *g, int n, int D, const float *center /*nullable [D]*/, double *block_partials,
                 int n_blocks, double *out /*[2D]*/, hipStream_t s);
// The same reduction -- grid, order, finishing tree -- with a per-row factor: out[d] = sum_i (double)factor[i] * (double)g[i,d] (the product of two
// float32 is exact in float64: a factor of 1 leaves every bit of the plain sums).  g == nullptr: the matrix is the one-hot of labels (int32 [n],
// every entry in [0, D)), so out[d] is the factor summed over the rows of class d.  out[D..2D) stays the maxima of |g|.  fit_prepared's weighted bias.
void column_sums_weighted(const float *g, const int32_t *labels, const float *factor /*[n]*/, int n, int D, double *block_partials, int n_blocks,
                          double *out /*[2D]*/, hipStream_t s);
int column_sums_blocks(int n, int D);
// max |standardised g| as float bits in out[0]; mean/inv_std nullable (Cosine: raw grads)
// Device-side statistics chain (one GPU): mean from the column sums; then std + 1e-8, the maxima and both fixed-point scales.
void stats_mean(const double *stat /*[2D] sums | max*/, long long n, int D, float *meanden /*[2D] mean | denom*/, hipStream_t s);
void stats_finish(const double *stat_raw /*[2D] sums | max|g|*/, const double *stat_centred /*nullable [2D] sum sq | max|g-mean|*/,
                  long long n, int D, int chunk_rows, float *meanden, StepScales *sc, hipStream_t s);
// RL-sized batches on one GPU: the whole chain above + the quantisation in one launch, same bits (k_small_stats); false: not covered
bool small_stats(const float *g, int n, int D, bool centred, int chunk_rows, double *stat /*[4D]*/, float *meanden /*[2D]*/, StepScales *sc, int32_t *qg,
                 hipStream_t s);
// qg = rint(((g - mean) / denom) * scale) as int32  (mean/denom nullable)
void quantize_grads(const float *g, size_t n_el, int D, const float *mean, const float *denom, const StepScales *sc,
                    int32_t *qg, hipStream_t s);

// ---- split candidates (A3, A4) ----
void column_minmax(const uint32_t *kt /*feature-major keys [F][n]*/, int n, int F, uint32_t *mn, uint32_t *mx, hipStream_t s);  // ordered keys
void uniform_thresholds(const uint32_t *min_keys, const uint32_t *max_keys, int F, int B, float *thr, hipStream_t s,
                        uint32_t *thr_keys = nullptr /*the thresholds' ordered keys, written by the same launch*/);
// counts[f][j] += #{rows : j == #{k : trial[f][k] (strict ? < : <=) key(x)}}; optionally writes codes[row*code_stride + code_off + f]
void bin_rows(const float *obs, int n, int F, const uint32_t *trial_keys, int B, bool strict, int64_t *counts,
              uint16_t *codes, int code_stride, int code_off, hipStream_t s);
void qsel_init(uint32_t *prefix, uint32_t *trial, int F, int B, hipStream_t s);
// one bisection step on bit `bit`: uses counts of trial = prefix|bit; then prepares trial for `next_bit` (or final keys if <0)
void qsel_update(uint32_t *prefix, uint32_t *trial, const int64_t *counts, const int64_t *cum_ranks, int F, int B,
                 int bit, int next_bit, hipStream_t s);
// fit(): MultiRMSE gradients g = pred - target (loss.cpp:42-56) and a row gather for the shuffled copy of the data set
void sub_arrays(const float *a, const float *b, float *out, size_t n, hipStream_t s);
void gather_rows(const float *src, const int32_t *perm, float *dst, int n, int width, hipStream_t s);
void f64_to_f32(const double *in, float *out, int n, hipStream_t s);
// row-sharded statistics: [D sums | P x D maxima, one row per rank] summed over ranks = sums + gathered maxima (step_stats.hip)
// (+ one trailing word, `extra`, summed like the rest: this rank's row count in the first round)
void stats_pack(const double *st, int D, int P, int rank, double *msg, hipStream_t s, double extra = 0.0);
void stats_unpack(const double *msg, int D, int P, double *st, hipStream_t s);
void negate_f32(float *p, int n, hipStream_t s);
void f32_to_f64(const float *in, double *out, int n, hipStream_t s);
void keys_to_floats(uint32_t *keys /*NaN-range keys are raised to -inf's key in place*/, float *out, size_t n, hipStream_t s);
void floats_to_keys(const float *in, uint32_t *keys, size_t n, hipStream_t s);
// The level's result block handed to the host without a copy engine: one block copies `bytes` (a multiple of 4) from device memory to
// pinned, device-mapped host memory and then stores `seq` to `flag` (system scope).  The host polls the flag; what it then reads is
// complete (the stores are fenced before the flag) and every earlier operation of the stream has finished.
void publish_block(void *d_src, void *h_dst_mapped, size_t bytes, uint32_t *flag_mapped, uint32_t seq, hipStream_t s, bool zero_src = false /*clear the source words after copying them*/);
// Two device arrays (sizes multiples of 4 bytes) into pinned, device-mapped host memory with one launch, no flag.
void publish_pair(const void *d_a, void *h_a_mapped, size_t a_bytes, const void *d_b, void *h_b_mapped, size_t b_bytes, hipStream_t s);
// Up to 8 small host -> device uploads with ONE launch: the sources live in pinned, device-mapped host memory (pass their DEVICE
// aliases), every segment is a multiple of 4 bytes.  Replaces a handful of copy-engine transfers (each ~10 us of stream time for a
// few KB) in steps that are bound by stream operations, not bytes.  The host must leave the sources alone until the kernel has run.
struct FetchSegments { void *dst[8]; const void *src[8]; uint32_t words[8]; int n; };
void fetch_segments(const FetchSegments &fs, hipStream_t s);
// up to 16 byte ranges out of one mapped pinned staging block by ONE launch (the model's device mirror after a step: a dozen appended slices
// of a few hundred bytes each; a hipMemcpyAsync per slice from pageable memory cost ~10 us apiece).  Ranges need no alignment.
constexpr int kStageSegments = 32;   // (a greedy model appends 17-18 slices per tree: one launch, not two)
struct StageSegments { void *dst[kStageSegments]; uint32_t src_off[kStageSegments]; uint32_t bytes[kStageSegments]; int n; };
void stage_copy(const StageSegments &ss, const void *stage_mapped, hipStream_t s);
// up to four regions filled with a 32-bit pattern each by ONE launch (an RL-sized step pays 4-5 us per hipMemsetAsync)
struct FillSegments { void *dst[4]; uint32_t words[4]; uint32_t value[4]; int n; };
void fill_segments(const FillSegments &fs, hipStream_t s);
void iota_rows(int32_t *rows, int n, hipStream_t s);

// ---- exact quantile selection and binning on transposed keys (quantile.hip) ----
struct QuantilePlan { int sample, n_split, n_chunks, chunk; };
constexpr int kQuantileClasses = 8192;
constexpr int kQuantileMaxSplit = 4095;
QuantilePlan quantile_plan(int n);
void transpose_keys(const float *obs, int n, int F, uint32_t *kt /*[F][n]*/, hipStream_t s);
void sample_splitters(const uint32_t *kt, int n, int F, const QuantilePlan &p, uint32_t *splitters /*[F][4095] sorted*/,
                      uint32_t *splitters_bfs /*[F][4095] breadth-first order, used by the searches*/, hipStream_t s);
void class_count(const uint32_t *kt, int n, int F, const QuantilePlan &p, const uint32_t *splitters_bfs,
                 uint32_t *partial /*[n_chunks][F][8192]*/, hipStream_t s);
// global_counts (nullable): all-reduced class counts of a row-sharded run -- ranks come from them, list lengths stay local
void quantile_targets(const uint32_t *partial, const int64_t *global_counts, const uint32_t *splitters, const int64_t *cum, int F, int B,
                      const QuantilePlan &p, uint32_t *class_off /*[F][8192], preset 0xff*/, uint32_t *tgt_off, uint32_t *tgt_len,
                      uint32_t *tgt_rank, uint32_t *thr_keys, uint32_t *alloc /*[1], zeroed*/, uint32_t max_elems,
                      uint32_t *overflow /*zeroed*/, hipStream_t s);
// row-sharded selection: raw local sample -> exchange -> identical splitters on every rank; bisection on the extracted lists
void sample_only(const uint32_t *kt, int n, int F, int S, uint32_t *sample_out /*[F][S]*/, hipStream_t s);
void place_sample(const uint32_t *samp, int F, int S, int rank, int SU, int64_t *uni /*[F][SU], zeroed*/, hipStream_t s);
void union_splitters(const int64_t *uni, int F, int SU, int n_split, uint32_t *splitters, uint32_t *splitters_bfs, hipStream_t s);
void counts_to_i64(const uint32_t *partial, int n_chunks, size_t fc, int64_t *out, hipStream_t s);
void select_count(const uint32_t *lists, const uint32_t *tgt_off, const uint32_t *tgt_len, const uint32_t *prefix, int bit, int n_targets,
                  int64_t *counts, hipStream_t s);
void select_update(uint32_t *prefix, const int64_t *counts, const uint32_t *tgt_off, const uint32_t *tgt_rank, int bit, int n_targets,
                   uint32_t *thr_keys, hipStream_t s);
void quantile_extract(const uint32_t *kt, int n, int F, const QuantilePlan &p, const uint32_t *splitters_bfs, const uint32_t *class_off,
                      const uint32_t *partial, uint32_t *out, hipStream_t s);
void quantile_select(const uint32_t *lists, const uint32_t *tgt_off, const uint32_t *tgt_len, const uint32_t *tgt_rank, int n_targets,
                     uint32_t *thr_keys, hipStream_t s);
// codes[(slot/16)*n*16 + row*16 + slot%16] (u16) = #{k : thr_key[f][k] < key(row, f)}
// small batches: one LDS sort per column (n <= sort_quantiles_max_rows()); thr_keys[f][k] = key of 1-based rank cum[k]
int sort_quantiles_max_rows();
bool sort_quantiles_fits(int n, int B);   // the LDS sort takes (S + B) * 4 bytes, S = n rounded up to a power of two: <= 64 KiB
void sort_quantiles(const uint32_t *kt, int n, int F, const int64_t *cum, int B, uint32_t *thr_keys, float *thr_floats /*the same thresholds as floats*/, hipStream_t s, uint16_t *codes = nullptr /* also write the class codes (k_bin_cols' output) */);
// radix_select.hip: exact order statistics by MSD radix counting (one GPU)
size_t radix_state_bytes(int F, int B);
size_t radix_partial_bytes(int F);
int radix_max_targets();
size_t radix_list_bytes(int n, int F);
// Row-sharded runs pass the exchange hook and two scratch buffers; cum then holds GLOBAL ranks and every rank ends with the
// same thresholds.  Returns 0, or non-zero when a HIP call (1) / the all-reduce (2) failed.
struct RadixComm {
    void *ctx;
    int (*allreduce_sum_i64)(void *ctx, int64_t *dev_buf, size_t count);   // called with the stream synchronised unless stream_ordered
    bool stream_ordered;        // the all-reduce is enqueued on the stream (native RCCL): radix_select never waits for the device -- the messages are
                                // sized by their upper bound (B slot rows per feature) instead of the slot counts read back after every pass
    int64_t *gbuf;              // radix_exchange_words(F) int64
    uint32_t *partial_global;   // radix_global_partial_bytes(F)
};
size_t radix_exchange_words(int F);
size_t radix_global_partial_bytes(int F);
int radix_select(const uint32_t *kt, int n, int F, const int64_t *cum, int B, void *state, uint32_t *partial, uint32_t *lists,
                 uint32_t *thr_keys, hipStream_t s, const RadixComm *comm /*nullable: one GPU*/,
                 int pass1_chunks = 0 /*> 0: `partial` already holds the first-digit counts written by transpose_keys_count*/,
                 uint32_t *le_out = nullptr /*[F][B] + [F]: number of keys <= each threshold (global, after the NaN-range fix-up of
                 keys_to_floats), for the root's class counts; the F trailing words are scratch*/);
// obs [n][F] -> kt [F][n] keys AND the first radix digit counted on the way (partial: the radix_partial_bytes(F) buffer).
// Returns the chunk count to pass to radix_select, or 0 when the shape does not qualify (nothing was done).
int transpose_keys_count(const float *obs, int n, int F, uint32_t *kt, uint32_t *partial, hipStream_t s);
void bin_cols(const uint32_t *kt, int n, int F, const uint32_t *thr_keys, int B, uint16_t *codes, hipStream_t s);
void scatter_cat_codes_grouped(const uint16_t *cat_codes, int n, int Fc, int F, uint16_t *codes, hipStream_t s);
constexpr int kCodeGroup = 16;  // code layout: groups of 16 feature slots, [group][row][16]
// row subsets of a prepared data set (gather_codes.hip): out[g][j][0..16) = codes[g][rows[j]][0..16) for g < n_groups, j < m -- whole 32-byte records,
// 16 bytes per lane.  Every rows[j] must lie in [0, n): the caller checks (a host vector on the host, a device vector with rows_minmax).
void gather_code_records(const uint16_t *codes /*[n_groups][n][16]*/, int n, int n_groups /*<= 65535*/, const int32_t *rows /*[m], device*/, int m,
                         uint16_t *out /*[n_groups][m][16]*/, hipStream_t s);
// rows binned against thresholds that already exist (bin_like.hip): codes[g][r][fl] = min(B, #{b : thr_keys[f][b] < float_to_key(obs[r][f])}),
// f = 16 g + fl, padding slots (f >= F) zero -- bin_cols' records from row-major float32 obs [n][F] in one pass, no transposed key copy.
// thr_keys [F][B] ascending per feature.  The keys of a group are searched in LDS while 16 * B * 4 bytes fit the opt-in, else in global memory.
void bin_like(const float *obs, int n, int F, const uint32_t *thr_keys, int B, uint16_t *codes /*[ceil(F/16)][n][16]*/, hipStream_t s);
// mm[0] = min rows[j], mm[1] = min ~rows[j] (= ~max) of a device index vector, m >= 1
void rows_minmax(const int32_t *rows, int m, int32_t *mm /*[2], device*/, hipStream_t s);
// column subsets of a prepared data set (gather_cols.hip): out[g'][j][i] = codes[cols[16 g' + i] / 16][rows ? rows[j] : j][cols[16 g' + i] % 16],
// the padding slots of the last output group zero.  cols (host, strictly ascending, every entry in [0, 16 * source groups)) is turned into a plan
// on the host -- the output groups cut into chunks of at most kGatherColsMaxStaged source groups, the source groups of every chunk, the tile
// offset of every output slot, cols itself -- which the caller uploads (n_words int32, 16-byte aligned) before the launch.  One kernel for every
// shape; a block owns kGatherColsRows rows.  rows as gather_code_records.
constexpr int kGatherColsRows = 64, kGatherColsMaxStaged = 16;
struct GatherColsPlan {
    int n_cols, n_out_groups, n_chunks, max_staged;   // max_staged: the most source groups a chunk stages
    int chunks_at, groups_at, offs_at, cols_at;       // word offsets into the plan
    size_t n_words, staged_groups;                    // staged_groups: source groups staged per row tile over all chunks (the records a row reads)
};
GatherColsPlan gather_cols_plan(const int32_t *cols, int n_cols, std::vector<int32_t> &words);
void gather_code_columns(const uint16_t *codes /*[groups][n][16]*/, int n, const int32_t *rows /*[m], device, nullable*/, int m, const int32_t *d_plan,
                         const GatherColsPlan &p, uint16_t *out /*[p.n_out_groups][m][16]*/, hipStream_t s);
// thr_out[f'][b] = thr[cols[f']][b] and the same for the keys ([F][B] tables, cols from the plan)
void gather_threshold_rows(const float *thr, const uint32_t *thr_keys, int B, const int32_t *d_plan, const GatherColsPlan &p, float *thr_out, uint32_t *keys_out,
                           hipStream_t s);
// the row sampler on the device (sample_rows.hip; the rule is sample_core.h's): rows_out[0 .. m) = the kept rows of [row0, row0 + n), ascending,
// as absolute indices; scratch[0] = m; with G (device [n][D], row r - row0 for row r) also G_out[j][:] = G[rows_out[j] - row0][:] in the same
// pass.  Three launches (count, a one-block scan of the block counts, write), positions from ranks only: the bytes do not depend on scheduling.
// rows_out / G_out need room for n rows unless the caller knows m; scratch holds sample_rows_blocks(n) + 1 words.  row0 + n <= 2^31.
constexpr int kSampleRowsPerBlock = 2048, kSampleScanWidth = 512;
int sample_rows_blocks(int n);
void sample_rows(int row0, int n, uint32_t thr /*sample_threshold(subsample)*/, uint64_t seed, int32_t draw, const float *G /*nullable*/, int D,
                 int32_t *rows_out, float *G_out /*nullable*/, int32_t *scratch, hipStream_t s);
// one-side sampling on the device (goss.hip, sample_rows.hip; the rule is sample_core.h's).  sample_goss enqueues, on one stream: the scores and keys
// of G's rows with the count of their first digit, the MSD radix selection of the k-th largest key (integer counts only; tau, #{key > tau} and the
// ties to take stay in device memory: gs.state), the tie counts per sampler block and their scan, then the sampler's count / scan / write with the
// one-side keep rule.  rows_out / factor_out [m], G_out [m][D] (room for n), gs.m_out[0] = m; weights (nullable, by absolute row) and eff_out (nullable,
// by absolute row: fl32(w * factor) of every kept row) serve fit_prepared's Newton sums.  Nothing waits for the host; the bytes do not depend on scheduling.
constexpr int kGossDigitBits = 8, kGossDigits = 1 << kGossDigitBits, kGossPasses = 32 / kGossDigitBits;
struct GossScratch { int32_t *m_out /*[2]: m, all ties*/; uint32_t *state /*[4]: tau, #{key > tau}, take, k*/; uint32_t *hist /*[passes][digits]*/; int32_t *tie_off, *blk /*[blocks] each*/; uint32_t *keys /*[n]*/; };
size_t goss_scratch_words(int n);
GossScratch goss_scratch(int32_t *words, int n);
void sample_goss(int row0, int n, int k /*floor(top_rate * n)*/, uint32_t thr, float amp, uint64_t seed, int32_t draw, const float *G, int D, int32_t *rows_out,
                 float *factor_out, float *G_out /*nullable*/, const float *weights /*nullable*/, float *eff_out /*nullable*/, const GossScratch &gs, hipStream_t s);
// the two halves of sample_goss (fit_prepared times them apart): scores, keys, selection and tie counts; then the tie scan and the sampler's passes
void goss_select(int n, int k, const float *G, int D, const GossScratch &gs, hipStream_t s);
void goss_sample_passes(int row0, int n, uint32_t thr, float amp, uint64_t seed, int32_t draw, const GossScratch &gs, const float *G, int D, int32_t *rows_out,
                        float *factor_out, float *G_out, const float *weights, float *eff_out, hipStream_t s);

// ---- split-score histograms (A6) ----
size_t hist_lds_bytes(int NB, int D, int FG);
// HistDirect (optional): every node of the level is ONE chunk (RL-sized batches), so a block's LDS tile already holds the node's
// complete sums for its feature group and leaves as hist[slot_map ? slot_map[chunk.slot] : chunk.slot][feature][class][D+1] (int64)
// -- no partials, no hist_reduce launch.  hist_build returns true when it wrote the histograms this way (the wide / quad variants
// for more than 16 outputs do not: the caller then reduces the partials as usual).
struct HistDirect {
    int64_t *hist = nullptr;
    const int32_t *slot_map = nullptr;
    int Fp = 0;
};
bool hist_direct_supported(int FG);   // the kernel hist_build will take for this layout can store the histograms itself
bool hist_build(const uint16_t *codes, int n_rows, const int32_t *qg, int D, const int32_t *rows,
                const Chunk *chunks, int n_chunks, int n_groups, int FG, int NB, int32_t *partials, hipStream_t s,
                hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr /*the dispatch's own begin / end timestamps*/,
                const HistDirect *direct = nullptr,
                bool count_rows = true /* false: the rows' count field is NOT accumulated (FG == 16, D <= 16 kernels only; returns as if
                true otherwise -- check hist_countless_supported): the root's class counts come from the selection, hist_reduce root_le */);
bool hist_countless_supported(int D, int FG, int n_rows);
constexpr size_t kHistLdsLimit = 160 * 1024 - 512;   // the largest LDS tile (hist_lds_bytes) a build block may ask for
// Features per block (16, 8, 4, 2 or 1) of a step with NB classes per feature and D outputs: the largest group whose LDS tile fits, halved further
// while more than 16 outputs leave a 16-lane row too few parts for the D + 1 fields.  The FG = 1 tile may still exceed kHistLdsLimit: callers check.
int hist_feature_group(int NB, int D);
// diagnostics (gbrl_hip_hist_plan): what hist_build does with a shape -- the route's kind (0 run-time D, 1 compile-time D, 2 wide, 3 quad), its
// parameter and abilities, read from the same rule and the same hooks as a launch; no HIP call
struct HistPlan { int kind, param; bool pipe, direct_ok, countless_ok; };
HistPlan hist_plan(int D, int FG, int n_rows);
// diagnostics (gbrl_hip_hist_probe): one hist_build (+ hist_reduce) on host arrays.  Everything is validated on the host before the first HIP call.
struct HistProbe {
    const uint16_t *codes;     // [ceil(Fp / 16)][n_rows][16], Fp = n_fslots rounded up to FG
    const int32_t *qg;         // [n_rows][D]
    const int32_t *rows;       // [m]
    const int32_t *chunks;     // [n_chunks][3] = (slot, start, len): slots ascending; behind the last entry with rows, len = 0 entries only
    const uint32_t *root_le;   // nullable [root_F][root_B]
    const int32_t *slot_map;   // nullable [n_nodes]
    int64_t *hist;             // in: the caller's sentinel; out: what the kernels stored over it.  hist_elems values
    long long hist_elems, root_n;
    int n_rows, D, m, n_chunks, n_nodes, n_fslots, FG, NB, mode /*0: partials + hist_reduce, 1: HistDirect*/, count_rows, root_F, root_B, chunks_per_slot, scatter_fs;
    int kind, param, pipe, counted, direct;   // out: the kernel launched (route kind and parameter, pipelined form, COUNT form), and whether the build stored the histograms itself
};
enum { kHistProbeOk = 0, kHistProbeInvalid = 1, kHistProbeDevice = 2 };
int hist_selftest(HistProbe &p, const char **why /*what was refused (static text)*/);
// diagnostics (gbrl_hip_score_probe, gbrl_hip_rows_probe): the kernels of step_score.hip / step_partition.hip on host arrays, through the launchers a
// step uses.  The same return codes; everything is validated on the host before the first HIP call.
int score_selftest(::gbrl_hip_score_probe_t &p, const char **why);
int rows_selftest(::gbrl_hip_rows_probe_t &p, const char **why);
// hist[slot_map ? slot_map[k] : k] = sum of the partials of chunk-slot k
void hist_reduce(const int32_t *partials, const int32_t *slot_chunk_begin /*[n_slots+1]*/, const int32_t *slot_map, int n_slots,
                 int n_groups, int FG, int NB, int D, int Fp, int64_t *hist, hipStream_t s,
                 int chunks_per_slot = 1 /* average chunks per node: picks the kernel variant */,
                 int scatter_fs = 0 /* > 0: write the feature-scattered send layout [f / fs][n_slots][f % fs][class][D+1] of a
                                       reduce-scatter over feature slices of fs features instead of hist[slot][Fp][class][D+1] */,
                 const uint32_t *root_le = nullptr /* [F][B] keys <= threshold: the count field of numeric feature f, class c becomes
                                       le[c] - le[c-1] (c = B: n_total - le[B-1]) instead of the partials' sum (root level, FG == 16) */,
                 int root_F = 0, int root_B = 0, long long root_n = 0);
// Row-sharded runs, feature-parallel scoring: the reduce-scattered slice [n][fs][class][D+1] of this rank's features goes to its
// place hist[slot_map[k]][lo + f][class][D+1] (f < min(fs, Fp - lo))
void hist_place_slice(const int64_t *recv, int64_t *hist, const int32_t *slot_map, int n, int fs, int lo, int Fp, size_t feat_elems, hipStream_t s);
void fill_f32(float *p, size_t n, float v, hipStream_t s);
// Winner of a level across ranks with ONE small sum all-reduce: every rank fills its own row of gather[P][n_win + 2 * n_act]
// (order-preserving key of (local best score, lowest reference index) per winner slot; total | right row counts of ITS best
// candidate per node) -- the other rows stay zero, so the sum is an all-gather -- and winner_adopt picks the highest key (ties:
// lowest index, the order of the single-GPU arg-max) and rebuilds best_idx / best_score / counts4 / the NodeSplit descriptors from
// the owning rank's counts.  n_win = 1 (oblivious: one condition per level) or n_act (greedy).
void winner_pack(const int32_t *best_idx, const float *best_score, const int64_t *counts4, int max_front, int n_win, int n_act, int rank,
                 int64_t *gather /*[P][n_win + 2 * n_act]: the kernel clears the other ranks' rows*/, hipStream_t s, int P);
void winner_adopt(const int64_t *gather, int P, int n_win, int n_act, bool oblivious, const int32_t *ref_to_internal, const int32_t *cand_slot,
                  const FeatureSlot *slots, const int32_t *seg_start, const uint32_t *thr_keys, int B, int32_t *best_idx, float *best_score,
                  int64_t *counts4, int max_front, NodeSplit *out, int32_t *cursors, hipStream_t s);
// cur[dst] = prev[parent] - cur[sibling]  (entries: triples {dst, parent, sibling or -1})

// ---- scoring / selection (A6, A7, A8) ----
// sub_par[node] >= 0: the node's histogram is hist_prev[sub_par] - hist[sub_sib] (sub_sib < 0: no sibling rows) -- computed,
// scored AND written back by the kernel (fused sibling subtraction); sub_par nullable
void score_candidates(int64_t *hist, const int64_t *hist_prev, const int32_t *sub_par, const int32_t *sub_sib, int n_nodes, int Fp, int NB, int D, const FeatureSlot *slots, int n_slots,
                      const float *thr /*[F][B]*/, int B, int n_cand, int min_data, int cosine, const StepScales *sc,
                      const int32_t *path_len, const int32_t *path_slot, const float *path_val, const int32_t *path_bin,
                      float *scores /*[n_nodes][n_cand]*/, float *parent /*[n_nodes]*/,
                      const float *cand_w, const int32_t *cand_ref, const int32_t *is_root,
                      float *part_v /*nullable.  greedy: [n_nodes][n_slots] best gain per feature -- arg-max stage 1 fused, scores not written*/,
                      int32_t *part_i, hipStream_t s, int slot0 = 0 /* first feature slot scored (n_slots of them): feature-parallel scoring */,
                      bool keep_derived = true /* false (last level only): derived slices are scored but not written back; resolve_splits
                      must then be given hist_prev / sub_par / sub_sib */,
                      float *part_s = nullptr /* greedy, nullable: [n_nodes][n_slots] the best gain of another candidate class than part_v's (near-tie detection) */,
                      int32_t *part_n = nullptr /* with part_s: rows the slot's best sends right (0 when it sends all of them: one class with 'none') */,
                      int32_t *cand_nr = nullptr /* nullable, scores mode (part_v == nullptr): [n_nodes][n_cand] rows every candidate sends right */);
// best_idx holds REFERENCE candidate indices (cand_ref[j]); ties go to the lowest reference index.  oblivious: one
// result (sum over nodes); greedy: one per node.  part_v/part_i: scratch of n_nodes * argmax_parts(n_cand).
int argmax_parts(int n_cand);
void argmax(const float *scores, int n_nodes, int n_cand, const float *cand_weight, const int32_t *cand_ref, const float *parent,
            const int32_t *is_root, bool oblivious, float *part_v, int32_t *part_i, int32_t *best_idx, float *best_score,
            hipStream_t s, float *part_s = nullptr /* nullable: per block the best score strictly below part_v */);

// near-tie detection inside resolve_splits (one GPU): counts4[2 * max_front + node] = 1 when the best DISTINCT runner-up is within
// rel * (magnitude of the scores) of the winner, or (greedy) the winning gain is that close to zero
struct NearDetect { const float *part_s; const int32_t *part_n /* nullable: oblivious */; float rel; const float *parent; const int32_t *is_root; int cosine; long long rows; /* of the batch (oblivious levels) */ };

// winner -> (feature slot, class) and the child sizes it induces, per active node (one read-back per level)
void resolve_splits(const float *part_v, const int32_t *part_i, int n_parts /*argmax stage-1 output; the final stage runs here*/,
                    int32_t *best_idx, float *best_score, bool oblivious, int n_nodes, const int32_t *ref_to_internal, const int32_t *cand_slot,
                    const FeatureSlot *slots, const int64_t *hist_local, const int64_t *hist_global /*nullable*/, int Fp, int NB, int D,
                    NodeSplit *out, int64_t *counts4 /*[4][max_front]*/, int max_front,
                    const int32_t *seg_start /*nullable: when given, out[] is a complete partition descriptor (do_split from
                    best_score, seg_start, n_left from hist_local) and cursors[2*node..] are zeroed*/,
                    int32_t *cursors, const uint32_t *thr_keys /*[F][B] ordered threshold keys*/, int B, hipStream_t s,
                    void *pub = nullptr /*pinned, device-mapped copy of the result block [best_idx | best_score | counts4]: mirrored, then ...*/,
                    uint32_t *pub_flag = nullptr /*... the last block stores pub_seq here (system scope)*/, uint32_t pub_seq = 0,
                    unsigned *pub_done = nullptr /*device counter, zero between launches*/,
                    const int64_t *hist_prev = nullptr, const int32_t *sub_par = nullptr /*non-null: derived nodes' counts = hist_prev[par] - hist_local[sib]*/,
                    const int32_t *sub_sib = nullptr, const NearDetect *near = nullptr);

// ---- near-tie replay (neartie.hip): the candidates inside the window of a flagged node are re-scored in the reference's float32
// sequence, and the arg-max input of resolve_splits (part_v / part_i) is rewritten with the reference's comparison of them.
constexpr int kNearCands = 16;         // distinct gains replayed per node (the closest ones)
constexpr int kNearMaxRows = 65536;    // batches up to this many rows keep the replay's row bitmaps in LDS; larger ones use a per-node bitmap in global memory (round 6)
constexpr int kNearMaxD = 1024;      // (the replay block keeps two mean vectors, a tile and two row bitmaps in 64 KB of LDS)
struct NearTieIO {
    const int32_t *rows;        // the level's row list
    const int32_t *seg_start;   // [n_act] first position of every active node's segment
    const int32_t *n_rows;      // [n_act] its length
    const uint16_t *codes;      // [group][row][16] class codes
    int N, D;
    const float *grads;         // [N][D] raw gradients
    const float *meanden;       // L2: [D] mean | [D] std + 1e-8f of the step; nullptr: raw gradients (Cosine)
    int cosine, oblivious, min_data;
    const FeatureSlot *slots;
    const int32_t *cand_slot;   // internal candidate -> feature slot
    const float *cand_w;        // [n_cand] feature weight of every internal candidate
    const int32_t *cand_ref;    // [n_cand] reference index of every internal candidate
    int n_cand;
    const float *scores;        // [n_act][n_cand] exact scores (score_candidates without part_v)
    const int32_t *cand_nr;     // greedy: [n_act][n_cand] rows every candidate sends right (same launch); nullptr: oblivious
    const float *parent;        // [n_act] exact parent scores
    const int32_t *is_root;     // [n_act]
    const float *best_score;    // [n_act] exact best gain (oblivious: [0])
    const int64_t *near;        // [n_act] flags (oblivious: [0])
    float rel;
    int n_act;
    int32_t *list;              // scratch [n_act][kNearCands]
    int32_t *list_n;            // scratch [n_act]
    int32_t *ent;               // scratch [max((kNearCands + 1) * N, n_cand)]: ordered row lists (the candidate list of an oblivious level keeps its level scores there first)
    float *rep;                 // scratch [n_act][kNearCands + 1]: replayed scores, [kNearCands] = the parent's
    float *part_v;              // arg-max stage-1 arrays of the level: rewritten for the replayed nodes
    int32_t *part_i;
    int n_parts;
    // N > kNearMaxRows and D % 4 == 0 (round 6): the chains are evaluated by seqsum.hip on the whole GPU instead of one lane per chain
    int lvl_ready;              // oblivious: the level scores of all candidates already sit in `ent` (k_near_level_scores ran: big levels)
    int fast;                   // 1: the order, the chains and the scores are produced by the whole GPU (k_near_rows .. k_near_finish)
    int32_t *pos;               // scratch [(kNearCands + 1) * N]: a listed row's place among the rows of its side
    int32_t *nr;                // scratch [n_act][kNearCands + 1]: rows going right (-1: block not replayed)
    int32_t *rowsort;           // scratch [N]: every replayed node's rows in ascending order (one list per node, shared by its candidates)
    int32_t *tiles;             // scratch [near_tie_fast_tiles]: per 2048-entry tile of a (node, candidate) list: rows going right, then their exclusive prefix
    float *vals;                // scratch [(kNearCands + 1) * N * D]: the chains' elements (column-major per side, then the dot chains' products)
    float *means;               // scratch [n_act][kNearCands + 1][2][D]
    float *sums;                // scratch [n_act][kNearCands + 1][2][D]: chain results (pass 1: per column; pass 2: [side][0])
    void *chains;               // scratch: SeqChain table [n_act * (kNearCands + 1) * 2 * D] + seq_sums scratch behind it
    size_t chains_bytes;
    uint32_t seq_blocks;        // upper bound of the chains' 256-element blocks
    uint32_t *maps;             // N > kNearMaxRows: scratch [n_act][ceil(N / 32)] -- a bit per row of the batch, set for the node's rows (k_near_rowmaps)
    int max_node_rows;          // nodes of more rows are not replayed (an oblivious level: when ANY of its nodes is larger); 0: no limit
};
size_t near_tie_map_words(int N, int n_act);   // 0 when the batch fits the LDS bitmaps
bool near_tie_fast_supported(int N, int D);     // big batch, D a multiple of 4: chains through seqsum.hip
uint32_t near_tie_fast_blocks(int N, int D, int n_act);
size_t near_tie_fast_chain_bytes(int N, int D, int n_act);
size_t near_tie_fast_tiles(int N, int n_act);
bool near_tie_supported(int N, int D);
void near_tie_replay(const NearTieIO &io, hipStream_t s);
// diagnostics (gbrl_hip_replay_scores): one node given by per-row flags, host pointers; out[0] = split score, out[1] = parent score
bool near_tie_selftest(const float *grads, const uint8_t *in_node, const uint8_t *goes_right, int n_rows, int D, const float *meanden, bool cosine, int min_data, float *out);

// seqsum.hip: sequential float32 sums of many arrays ("chains"), evaluated in parallel and bit for bit (block summaries that depend on the
// running sum's parity only; the serial loop where a power of two is crossed)
struct SeqChain { const float *x; uint32_t len; uint32_t blk0; float start; };   // blk0: first of the chain's ceil(len / 256) blocks in the flat block arrays (ascending over the chains)
size_t seq_sums_scratch_bytes(uint32_t n_blocks);
void seq_sums(const SeqChain *d_chains, int n_chains, uint32_t n_blocks, void *d_scratch, float *d_out, uint32_t *d_n_slow /*nullable*/, hipStream_t s);
bool seq_sums_selftest(const float *x, const uint32_t *lens, const float *starts /*nullable*/, int n_chains, float *out, uint32_t *n_slow_out /*nullable*/);
// diagnostics (gbrl_hip_seq_sums_model): the same chains walked on the CPU with the arithmetic of seqsum_core.h, the kernels' decisions in the kernels' order; no HIP call
bool seq_sums_model(const float *x, const uint32_t *lens, const float *starts /*nullable*/, int n_chains, float *out, uint32_t *n_slow_out /*nullable*/, uint32_t *n_fast_out /*nullable*/);

// rows going right per node for the chosen splits (row-sharded runs: local child sizes without a local histogram)
void localize_splits(NodeSplit *splits, const int32_t *n_local, const int64_t *right_local, int n_nodes, hipStream_t s);
void localize_publish(NodeSplit *splits, const int32_t *n_local, const int64_t *right_local, int n_nodes, void *d_src, void *h_dst_mapped, size_t bytes,
                      uint32_t *flag_mapped, uint32_t seq, hipStream_t s);   // localize_splits + publish_block in one launch
void hist_place(const int64_t *src, int64_t *dst, const int32_t *slot_map, int n, size_t node_elems, hipStream_t s);
void count_right(const int32_t *rows, const uint16_t *codes, const uint32_t *kt /*nullable: feature-major keys*/, int n_rows, const Chunk *chunks, int n_chunks, const NodeSplit *splits,
                 int64_t *n_right /*[n_nodes], zeroed*/, hipStream_t s);

// ---- device-side level planning (oblivious trees on one GPU) ----
// All descriptors of tree level L -- node segments, the histogram chunk table of the smaller child of every pair, slot maps for the
// sibling subtraction, path arrays, partition chunks -- built on the device from the previous level's resolved splits, so that a
// whole tree is enqueued without a host round trip per level (the host replays the bookkeeping from the per-level result blocks
// after ONE synchronisation).  Unused entries of the chunk tables (up to cap_h / cap_p) get len 0: the consumers are launched with
// those worst-case grids and empty chunks exit at once.  state[0] != 0: growth has stopped (fitter.cpp:458), state[1] = level.
struct ObliviousPlan {
    int32_t *node_seg, *node_n;            // [max_depth + 1][mf] segment start / row count of the level's nodes
    int mf;
    Chunk *chunks; int cap_h;              // histogram chunks of the level
    int32_t *chunk_begin;                  // [mf + 1]
    int32_t *slot_map, *sub_par, *sub_sib; // [mf]
    int32_t *path_len, *path_slot, *path_bin, *is_root;   // [mf] / [mf][kMaxPath]
    float *path_val;
    Chunk *part_chunks; int cap_p;         // partition chunks of the level
    int32_t *seg_starts;                   // [mf]
    int32_t *state;                        // [2]
    int32_t *cond_slot, *cond_bin;         // [kMaxPath] the conditions chosen so far (one per level)
    float *cond_val;
};
void plan_oblivious_level(int level, int n_rows, int chunk_rows, int budget, const NodeSplit *resolved_prev, const float *best_score_prev,
                          const float *thr, int B, const ObliviousPlan &pl, hipStream_t s);

// ---- partition (A9) ----
void partition_rows(const int32_t *rows_in, int32_t *rows_out, const uint16_t *codes, const uint32_t *kt /*nullable*/, int n_rows,
                    const Chunk *chunks, int n_chunks, const NodeSplit *splits, int32_t *cursors /*[n_nodes*2], zeroed*/,
                    hipStream_t s);

// ---- RL-sized steps: the whole preparation in ONE launch (small_prep.hip) ----
// Split candidates (quantile: <= 4096 rows, `cum` = the device copy of the target ranks; uniform: <= 8192 rows) and class codes of every
// numeric feature from the row-major matrix, and -- when `want_stats` and the shape qualifies (small_stats' limits) -- the gradient statistics,
// scales and quantised gradients (*stats_done).  false: nothing was launched (the caller runs the separate kernels).
bool small_prep(const float *obs, int N, int F, int B, bool uniform, const int64_t *cum, float *thr, uint32_t *thr_keys, uint16_t *codes,
                uint16_t *codes_fm /*[F][N]: a second, feature-major copy of the numeric codes for kern::small_grow*/, const float *grads, int D, bool centred, int chunk_rows, double *stat, float *meanden, StepScales *sc, int32_t *qg,
                bool want_stats, bool *stats_done, hipStream_t s);

// ---- RL-sized steps: the whole growth of one tree in ONE launch (small_grow.hip) ----
// Per level: LDS histograms of the owned feature slots, scores, arg-max, ONE grid barrier, row routing; then the leaf sums.  The host reads
// `status[0] == seq` (pinned), then MD result blocks of small_grow_res_stride(MD) bytes -- [best_idx i32 x mf][best_score f32 x mf]
// [counts i64 x 4 x mf: total | right | - | -][winner threshold f32 x mf], mf = 2^(MD-1) -- and acc[node id][D+1] of every leaf.
struct SmallGrowIO {
    const uint16_t *codes; const int32_t *qg; const float *grads; const StepScales *scales;
    const uint16_t *codes_fm = nullptr;   // nullable: feature-major copy [n_fm][N] of the codes of the slots < n_fm (written by kern::small_prep)
    int n_fm = 0;
    int n_thr_slots = 0;                  // numeric slots (the rows of thr)
    const FeatureSlot *slots; const float *thr; const float *cand_w; const int32_t *cand_ref;
    int N, D, B, n_slots, NB, MD, min_data;
    bool cosine, oblivious;
    int G;                 // blocks: small_grow_blocks(n_slots)
    void *bests;           // device scratch, small_grow_bests_bytes(MD, G, oblivious)
    unsigned *sync;        // device, 4096 bytes, zero before the first launch (the kernel hands them back zeroed)
    char *res;             // pinned, device-mapped
    char *res_dev;         // device staging of the result blocks, MD * small_grow_res_stride(MD) bytes
    int64_t *acc;          // pinned, device-mapped, [2 << MD][D + 1]
    uint32_t *status;      // pinned, device-mapped, 16 words: sequence word | levels | node count | error (2 = near-tie: level loop) | levels replayed in the kernel
    uint32_t seq;
    uint32_t *prof = nullptr;   // measurement: pinned, 16 words (block 0's time per phase, 10 ns units)
    StepScales *scales_out = nullptr;   // pinned, device-mapped: the step's scales for the host (what publish_pair hands over in the level loop)
    void *near_scratch = nullptr;   // device, small_grow_near_bytes(G, N): the kernel replays a near-tie at one node of a greedy level itself
    const float *meanden = nullptr; // L2: the step's standardisation (mean | std + 1e-8f) for that replay; nullptr: raw gradients (Cosine)
    bool resume = false;        // with replay: continue from the checkpoint the default variant left (status word 5 = 1) instead of growing from the root
    bool replay = false;        // the kernel variant that replays a flagged node itself (launched for a tree the default variant gave up: status word 3 = 2)
    float near_rel = 0.0f;      // > 0: near-tie detection -- the kernel gives the tree up (status word 3 = 2) at the first level whose runner-up
                                // is within near_rel of the winner; the level loop then grows it with the replay (neartie.hip)
};
bool small_grow_supported(int N, int D, int NB, int MD, int n_slots, int n_cand);
int small_grow_blocks(int n_slots);
size_t small_grow_bests_bytes(int MD, int G, bool oblivious);
size_t small_grow_res_stride(int MD);
size_t small_grow_near_bytes(int G, int N, int MD);
bool small_grow(const SmallGrowIO &io, hipStream_t s);   // false: nothing was launched

// ---- leaf values (A11) ----
void leaf_sums(const float *grads, int D, const int32_t *rows, const Chunk *chunks, int n_chunks, const StepScales *sc,
               int64_t *acc /*[n_leaves][D+1], zeroed*/, hipStream_t s);

// ---- prediction (A13) ----
struct PredictModel {
    const int32_t *tree_indices, *depths, *feature_indices, *cat_ids;
    const float *feature_values, *values, *bias;
    const uint8_t *is_numerics, *inequality_directions;
    int n_trees, n_leaves, max_depth, D, oblivious;
    int n_opts;
    const int32_t *opt_start, *opt_stop;
    const float *opt_lr;
    // fast oblivious path (k_predict_obl): per split row 2*max_depth ints (feature index | ~categorical index, threshold bits |
    // category id), and -- when the optimisers' output ranges do not overlap -- one learning rate per output
    const int32_t *cond_pack;
    // fast greedy path (k_predict_grd): every greedy tree rebuilt as a binary tree from its leaves' paths.  Node = int4
    // (feature | ~categorical feature, threshold bits | category id, left child, right child); a child >= 0 is a node of the
    // same tree, < 0 encodes ~(leaf index within the tree).  grd_node_off[t] .. grd_node_off[t+1] are tree t's nodes (root
    // first); grd_ok == 0 when some tree is not a proper binary tree (or has depth 0, Q7): the generic walk is used then.
    const int32_t *grd_nodes;
    const int32_t *grd_node_off;
    int grd_ok, grd_max_nodes, grd_max_leaves;
    int obl_ok, coef_ok;
    uint64_t coef_cover;
    float coef[64];
    // Linear schedules (predict_sched.hip): rate[t * n_opts + o] = learning rate of optimizer o for the tree with absolute index t, for
    // every tree of the ensemble; nullptr when every optimizer is Const.  owner[j] = the optimizer of output j (valid when coef_ok).
    const float *rate;
    uint8_t owner[64];
    float *partial;          // scratch for tree-split prediction of small batches (nullable), partial_floats elements
    size_t partial_floats;
    int tree_chunk;          // set by kern::predict: trees per block column (0 = every block walks the whole range)
    int tree_splits;         // set by kern::predict: block columns (the last one takes the remainder of the range)
    int par_th;              // the model's par_th (the reference's rows / trees per host thread, utils.h:64-80)
    int32_t *slots;          // scratch of the two-launch chain path (predict_chain.hip), slot_ints elements; nullptr: path not offered
    size_t slot_ints;
    // second-generation oblivious path (predict_obl2.hip): leaf values pre-swizzled per tree as [worker 0..3][leaf < 2^max_depth]
    // [DMAX/4] (DMAX = obl2_padded_outputs(D), zero padded), and per tree 2*obl2_maxd condition words RIGHT-aligned (a tree of depth
    // d < obl2_maxd starts with obl2_maxd - d never-true conditions: feature 0, threshold +inf); obl2_maxd = 0: not available
    const float *values_sw;
    const int32_t *cond_ra;
    int obl2_maxd;
    int cat_dict_size;       // dictionary ids of categorical conditions are 1..cat_dict_size (the kernel packs them in 16 bits)
    // packed-code path (predict_reg.hip, k_pack_codes + k_predict_pc): the ensemble's code book, built by the engine when the shape
    // qualifies (nullptr otherwise).  A row becomes pc_row_words dwords: pc_wn numeric words (two 16-bit fields: 0xffff - number of
    // the feature's sorted distinct thresholds below x), then categorical words (one inverted one-hot bit per mentioned category).
    const int32_t *pc_cond;       // per tree obl2_maxd x (word, shift, T), right-aligned like cond_ra (padding: 0, 0, 0 = never true)
    const float *pc_thr;          // sorted distinct thresholds, feature by feature
    const int32_t *pc_thr_off;    // [F + 1]
    const int32_t *pc_cat_slot;   // [cat_dict_size + 1]: dictionary id -> bit slot (-1: none; id 0 = unknown cell)
    const int32_t *pc_word_cols;  // [2 x categorical words]: first and last + 1 column with a slot in the word
    uint32_t *pc_rows;            // scratch [n][pc_row_words]
    int pc_wn, pc_nw, pc_row_words, pc_iters;
};
int obl2_padded_outputs(int D);     // 4, 8, 16, 32, 64 (0: D > 64)
int obl2_levels(int max_depth);     // 4, 6, 8 (0: max_depth > 8)
bool obl2_feasible(int max_depth, int D, bool greedy);   // false: no launch plan can take the shape (the mirror is then not built)
// Small / medium batches against large ensembles: leaf search spread over the chip, then one fused multiply-add chain per (row,
// output) in tree order -- the bits of the one-chain-per-row kernels (predict_chain.hip).  false: not covered, nothing was launched.
constexpr int kChainU = 64;              // slot rows are padded in multiples of this many trees
constexpr int kSlotPad = 10 * kChainU;   // the relays request up to 3 W - 2 batches behind the range (k_chain_relay / k_sched_relay assert it)
size_t predict_chain_slot_ints(int n, int trees);
bool predict_chain(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                   float *out, hipStream_t s);
// The first launch of predict_chain alone: slots[row][tree of the range] = byte offset of the leaf's values row, *Ts_out = the row stride of
// `slots`.  false: not covered, nothing was launched.  (predict_sched.hip runs its own chain stage behind it.)
bool predict_chain_slots(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                         int *Ts_out, hipStream_t s);
// Ensembles with a Linear learning-rate schedule (PredictModel::rate != nullptr; predict_sched.hip): general, streaming and chain kernels
// that scale tree t by rate[t][optimizer].  Always launches.
// out[r][j] = bias[j] + the pm.tree_splits partial sums of pm.partial, in tree order (small batches whose trees were spread over block columns)
void predict_combine(const PredictModel &pm, int n, float *out, hipStream_t s);
void predict_sched(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                   float *out, hipStream_t s);
bool predict_obl2(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                  float *out, hipStream_t s);   // false: shape not covered, nothing was launched
// Small greedy ensembles over large batches (predict_grd_stream.hip, round 6): the whole ensemble in LDS, one barrier-free pipeline per
// wave with the next row tile held in registers.  Same mirror and the same bits as predict_obl2's greedy mode; false: not covered.
bool predict_grd_stream(const PredictModel &pm, const float *obs, int F, int Fc, int n, int start_tree, int stop_tree, float *out, hipStream_t s);
// Third-generation oblivious path for large batches (predict_reg.hip): the row tile lives in a bank of VGPRs, every level is a
// VGPR-relative compare, the only LDS traffic is the leaf-value gather.  Same mirrors as predict_obl2; false: not covered.
bool predict_reg(const PredictModel &pm, const float *obs, int F, int Fc, int n, int start_tree, int stop_tree, float *out, hipStream_t s);
// The same walk over PACKED rows (categorical columns, rows wider than the fp32 bank, feature counts that are not multiples of 4).
bool predict_pc(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree, float *out,
                hipStream_t s);
int predict_pc_bank_words();                      // dwords of a packed row the kernel can hold
bool predict_pc_shape_ok(int obl2_maxd, int D);   // levels / outputs the packed-code kernels are compiled for
// Dictionary encoding of categorical cells on the device (predict): cells [n][Fc][128 B]; the dictionary holds, per
// categorical feature f, its entries sorted by hash: feat_off[f] .. feat_off[f+1] index dict_hash / dict_id / dict_words
// (16 uint64 per entry, normalised).  codes[i*Fc+f] = id of the matching entry, 0 when the cell is not in the dictionary.
// Distinct categorical cells of a batch (A5 on the device).  cat_distinct_insert fills per-feature open-addressing tables
// (keys = raw 128-byte hash, first = smallest row that holds the key) and appends the table slot of every NEW key to list_slot
// (counter = number of distinct (feature, cell) pairs); cat_distinct_verify confirms that every cell equals the cell of its
// key's first row (flags[1] = 1 on a 64-bit hash collision); cat_publish writes header + (feature, first row, hash, cell) of the
// first `cap` list records into mapped pinned host memory.  flags[0] = 1 when a table or the list overflowed.  cat_step_codes
// writes the class of every cell (dictionary sorted by
// hash per feature, id = class, words = raw cell) straight into the grouped u16 code array (slot F+f).
void cat_distinct_insert(const char *cells, int n, int Fc, uint64_t *keys, int32_t *first, int log2_cap, int32_t *flags, int32_t *list_slot,
                         int32_t *counter, int list_cap, hipStream_t s);
void cat_distinct_verify(const char *cells, int n, int Fc, const uint64_t *keys, const int32_t *first, int log2_cap, int32_t *flags,
                         hipStream_t s);
// rank_count / rank_total (nullable, device): the ranking statistics of cat_rank, published as two more words per record (h_count, h_total);
// h_names null: a second publish of records whose feature, first row, hash and cell have already arrived -- only the statistics travel.
void cat_publish(int32_t *meta, const int32_t *list_slot, const uint64_t *keys, const int32_t *first, int log2_cap, const char *cells,
                 int Fc, int cap, int32_t *h_hdr, int32_t *h_feat, int32_t *h_first, uint64_t *h_hash, char *h_names, int32_t *slot_q,
                 uint32_t seq, hipStream_t s, const int32_t *rank_count = nullptr, const float *rank_total = nullptr, int32_t *h_count = nullptr,
                 float *h_total = nullptr);
// cat_rank.hip: more distinct (feature, cell) pairs than candidates are kept -- per list record q of the scan above the number of rows that
// carry it (count) and the float32 sum of their squared gradient norms in ascending row order from 0.0f (total), bit for bit the reference's
// loop (split_candidate_generator.cpp:119-129).  n_q = records in the list (the host has read it from the published header); slot_q is
// filled for all of them; meta[0] is set when a cell is not found in the tables.  Everything is enqueued on s, nothing is read back.
bool cat_rank_fits(int N, int Fc);
size_t cat_rank_scratch_bytes(int N, int Fc, int n_q);
void cat_rank(const char *cells, int N, int Fc, const float *grads, int D, const uint64_t *keys, int log2_cap, int32_t *meta,
              const int32_t *list_slot, int n_q, int32_t *slot_q, void *scratch, int32_t *count, float *total, hipStream_t s);
// diagnostics: host arrays in, (feature, first row, count, total) of every distinct pair out; returns their number, -2: more than cap, -1: failed
int cat_rank_selftest(const char *cells, int n, int Fc, const float *grads, int D, int cap, int32_t *feat, int32_t *first_row, int32_t *count,
                      float *total);
// radix_sort.hip: one pass (8 bits at `shift`) of a stable LSD radix sort of (key, value) pairs over `segments` arrays of n elements each,
// laid out [segments][n]: every segment is sorted on its own, from (key, val) into (key_out, val_out).  hist is scratch for
// segments * 256 * radix_sort_tiles(n) words.  Three launches on s; segments * n < 2^31 - kRadixSortTile, segments <= 65535.
constexpr int kRadixSortTile = 2048;   // elements one block owns: 256 threads x 8 rounds
uint32_t radix_sort_tiles(size_t n);
void radix_sort_pass(const uint32_t *key, const uint32_t *val, uint32_t n, int segments, int shift, uint32_t *hist, uint32_t *key_out, uint32_t *val_out,
                     hipStream_t s);
// metric.hip: the integers of the classifier metrics (metric_core.h) of a prediction matrix P [n][D] (device), added to counters the caller
// has ZEROED on s.  D <= 128.
//   metric_error      wrong [D] (softmax: [1]; T is then int32 [n], every label in [0, D)) += wrong cells per column
//   metric_positives  pos [D] += rows with Y[r][d] > 0.5
//   metric_auc        u2 [D] += 2U_d; pos (nullable) as metric_positives.  metric_auc_fits: n * D < 2^31 - kRadixSortTile.  scratch holds
//                     metric_auc_scratch_bytes(n, D): 16 n D bytes of key / flag ping-pong, the sort's histograms, n + 1 prefix words per column
void metric_error(int objective, const float *P, const void *T, int n, int D, unsigned long long *wrong, hipStream_t s);
bool metric_auc_fits(int n, int D);
size_t metric_auc_scratch_bytes(int n, int D);
void metric_positives(const float *Y, int n, int D, unsigned long long *pos, hipStream_t s);
void metric_auc(const float *P, const float *Y, int n, int D, void *scratch, unsigned long long *pos, unsigned long long *u2, hipStream_t s);
// class codes of a step batch from the scan's own tables: cls_of_q[slot_q[slot of the cell]] (see k_cat_step_codes_table)
void cat_step_codes_table(const char *cells, int n, int Fc, int F, const uint64_t *keys, const int32_t *slot_q, const int32_t *cls_of_q,
                          int log2_cap, uint16_t *codes, hipStream_t s);
void cat_step_codes(const char *cells, int n, int Fc, int F, const int32_t *feat_off, const uint64_t *dict_hash, const int32_t *dict_cls,
                    const uint64_t *dict_words, uint16_t *codes, hipStream_t s);
void encode_categories(const char *cells, int n, int Fc, const int32_t *feat_off, const uint64_t *dict_hash, const int32_t *dict_id,
                       const uint64_t *dict_words, int32_t *codes, hipStream_t s);
void predict(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
             int stop_tree, float *out, hipStream_t s);
// Continue a held prediction (predict_continue.hip): out[r][j] = base[r][j] carried through the trees [start_tree, stop_tree) in tree order,
// p = fma(-rate(t, o), value, p) for every optimizer o that owns output j; an output no optimizer owns keeps its base value, the bias is never
// added.  ONE chain per (row, output) at every batch size and range length (no tree-range split, unlike kern::predict).  base and out are
// device pointers and may be the same buffer.  generic: the one-thread-per-row kernel only (GBRL_HIP_CONTINUE_GENERIC=1).  Always launches.
void predict_continue(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree,
                      const float *base, float *out, bool generic, hipStream_t s);
// The same chain with the row read from a prepared data set's bin codes (predict_continue_codes.hip): the bits of predict_continue on the
// observations the data set was made from, for a model whose numeric conditions all compare against that data set's thresholds.
//   CodeTables  device tables of the engine's mirror with the threshold word replaced by the condition's bin (x > v <=> code > bin): `bins`
//               indexed like feature_values, `cond_pack` like PredictModel::cond_pack, `grd_nodes` like PredictModel::grd_nodes (same offsets)
//   CodeRows    the rows to walk: row j of the call is data set row rows[row0 + j] (rows != nullptr, device, every entry in [0, n_rows)) or
//               row0 + j; codes [groups][n_rows][16] u16
// base / out (may be the same buffer) / targets / grad_out are device [m][D], indexed by j.  targets != nullptr: grad_out = fl32(out - targets)
// of the new out in the same pass (kern::sub_arrays' bits).  loss_targets != nullptr (device [m][D], independent of the gradient tail):
// loss_part[j / 64] = the wave's sum of the rows' sum_d (double)fl32(out - loss_targets)^2 for the new out -- the partials
// loss_partials_of_predictions writes for these predictions (staged_loss_partials(m) doubles; staged_loss_finish sums them).
// generic: the one-thread-per-row kernel only.  Always launches (m > 0).
struct CodeTables { const int32_t *bins, *cond_pack, *grd_nodes; };
struct CodeRows { const uint16_t *codes; int n_rows, groups; const int32_t *rows; int row0; };
void predict_continue_codes(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int start_tree, int stop_tree, const float *base,
                            float *out, const float *targets, float *grad_out, const float *loss_targets, double *loss_part, bool generic, hipStream_t s,
                            int objective = 0, const float *weights = nullptr, const float *alpha = nullptr);
// objective (kObjRmse / kObjLogistic / kObjSoftmax of objective_core.h) selects the two tails: logistic takes the same [m][D] float targets and
// writes dL/dp of the sigmoid cross-entropy, its loss tail sums that loss; softmax takes ONE int32 label per row -- targets / loss_targets then
// point at int32 [m] -- and writes softmax(p) - onehot.  A range without a tree runs the stand-alone kernel below on the copied base.
// weights (nullable, device float32 [m], indexed by j; every entry checked by the caller, weight_stats below): the gradient tail stores
// fl32(w * g) and the loss tail sums (double)w * the row loss (objective_core.h).  nullptr launches the kernels of the call without weights.
// kObjQuantile (quantile_core.h): float targets [m][D] as rmse, alpha the device table of its D levels (required; weights are not taken): the gradient
// tail writes the pinball step, the loss tail sums the pinball loss.
//
// The loss of "one column shuffled" variants of a data set's rows (perm_loss.hip; perm_core.h has the permutation), none of them materialised.
// A variant is (col, repeat): row i reads column col from row perm(n, seed, col, repeat)(i) and every other column from itself; col < 0 is the
// data set as it is (the baseline).  For each of the n_variants entries of `variants` (device) the trees [0, n_trees) are walked from the model's
// bias over all n rows of `codes` ([groups][n][16] u16) and loss_part[v][j / 64] = the wave's sum of the objective's row losses: the partials the
// loss tail of predict_continue_codes writes for that variant's rows (n_variants x staged_loss_partials(n) doubles; staged_loss_finish_rows sums
// them).  No prediction is stored.  targets / alpha as predict_continue_codes' loss_targets / alpha (no weights).  n_variants <= kPermLaunchVariants
// per launch keeps the partials bounded; n_trees >= 1 and a model with an optimizer: the caller checks.  generic: the one-thread-per-row kernel only
// (GBRL_HIP_PERM_GENERIC=1; same bytes).  Always launches (n > 0, n_variants > 0).
constexpr int kPermLaunchVariants = 64;
struct PermVariant { int32_t col, repeat; };
void perm_loss(const PredictModel &pm, const CodeTables &ct, const uint16_t *codes, int n, int groups, int n_trees, int objective, const float *targets,
               const float *alpha, uint64_t seed, const PermVariant *variants, int n_variants, double *loss_part, bool generic, hipStream_t s);
int perm_tile_rows();   // rows of the streaming kernel's LDS tile = rows per loss partial
//
// The predictions of "columns held constant" variants of a data set's rows (pd_rows.hip; pd_core.h has PdVariant, the break rule and the launch
// plan), none of them materialised.  A variant (col0, code0, col1, code1) reads column col0 -- and col1 when >= 0 -- of every row as that constant
// code (in [0, n_bins]: the caller checks) and every other column from the row; col0 < 0 is the data set as it is.  For each of the n_variants
// entries of `variants` (device) the trees [0, n_trees) are walked from the model's bias over the m rows of cr (predict_continue_codes' CodeRows) and
// part[(v * D + d) * nb + j / 64] = the wave's sum of (double)p[j][d], nb = ceil(m / 64): n_variants x D x nb doubles, summed by
// staged_loss_finish_rows(part, nb, n_variants * D, ...).  ice != nullptr (device): the row itself goes to ice[(slots[v] * m + j) * D + d] -- the
// bits predict_continue_codes writes from a tiled bias for a data set that holds those codes; slots is device int32 [n_variants] (read only then).
// n_variants <= pd_launch_variants(m, D) per launch keeps the partials under pd_core.h's budget; n_trees >= 1: the caller checks.  generic: the
// one-thread-per-row kernel only (GBRL_HIP_PD_GENERIC=1; same bytes).  Always launches (m > 0, n_variants > 0).
struct PdVariant;
void pd_rows(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int n_trees, const PdVariant *variants, const int32_t *slots, int n_variants,
             double *part, float *ice, bool generic, hipStream_t s);
//
// The objectives on a prediction matrix (objective.hip): the device functions of the tails applied to pred [n][D] (device).  targets: float32
// [n][D] (rmse, logistic) or int32 [n] (softmax; every label in [0, D): the caller checks, label_counts below).  grad_out (device [n][D]) and
// loss_part (staged_loss_partials(n) doubles, one per 64 rows, finished by staged_loss_finish) may each be null.  D <= 128.
void objective_rows(int objective, const float *pred, const void *targets, int n, int D, float *grad_out, double *loss_part, hipStream_t s,
                    const float *weights = nullptr /*device [n]: the weighted forms*/, const float *alpha = nullptr /*device [D]: kObjQuantile's levels*/);
// What the engine needs to know of a weight vector (device float32 [n]) in one pass: stat[0] = the smallest row whose weight is a NaN, negative,
// infinite or above kWeightMax (INT32_MAX: none), stat[1] = the bits of the largest entry (non-negative floats order like their bits; a refused
// entry does not enter); part[j / 64] = the wave's sum of (double)w in the loss partials' fixed order, finished into *sum by staged_loss_finish: two
// calls give the same bits.  stat is device int32 [2], set to {INT32_MAX, 0} by the caller on `s`; part holds staged_loss_partials(n) doubles.
void weight_stats(const float *weights, int n, int32_t *stat, double *part, double *sum, hipStream_t s);
// counts[c] += rows with label c (integer atomics; counts is device int32 [D + 1], ZEROED by the caller on `s` except counts[D] = INT32_MAX);
// counts[D] = the smallest row index whose label is outside [0, D)
void label_counts(const int32_t *labels, int n, int D, int32_t *counts, hipStream_t s);
void tile_rows(const float *row /*[D], device*/, int D, int n, float *out /*[n][D]*/, hipStream_t s);   // out[r] = row: fit_prepared's held prediction starts as the bias
// Ranking objectives (rank.hip; rank_core.h has the rule).  off: device int32 [Q + 1], the queries' first rows (off[0] = 0, off[Q] = n, every size in
// [1, kRankMaxQuery]: the caller has checked); disc: device float64 [kRankMaxQuery], rank_discount_table's.  stat: device unsigned long long [3] =
// {flag word, first row with a label outside [0, kRankMaxLabel], pair count P}, set to {0, ~0, 0} by the caller on `s`.
// rank_queries (once per label vector): qid int32 [n] the row's query, max_dcg / inv float64 [Q], stat[1], stat[2]; ideal float64 [n] and beats int32
// [n] are scratch.  rank_rows (per score vector; labels checked): pos int32 [n], term float64 [n] (scratch: the DCG terms), then -- each where its
// output is not null -- g_out / h_out float32 [n], pair_part (kObjPairwise only: staged_loss_partials(n) doubles, the loss sums of the pairs each row
// wins), ndcg float64 [Q] with ndcg_part (staged_loss_partials(Q) doubles); both partial vectors are finished by staged_loss_finish.  stat[0] collects
// kRankBadPred.
void rank_queries(const int32_t *labels, const int32_t *off, int n, int Q, const double *disc, int ndcg_at, int32_t *qid, double *ideal, int32_t *beats,
                  double *max_dcg, double *inv, unsigned long long *stat, hipStream_t s);
void rank_rows(int objective, const float *scores, const int32_t *labels, const int32_t *off, const int32_t *qid, const double *max_dcg, const double *inv, int n,
               int Q, const double *disc, int ndcg_at, int32_t *pos, double *term, float *g_out, float *h_out, double *pair_part, double *ndcg, double *ndcg_part,
               unsigned long long *stat, hipStream_t s, int stages = 7 /* kRankStage*: a caller that times the kernels one by one launches them one by one */);
constexpr int kRankStagePositions = 1, kRankStagePairs = 2, kRankStageNdcg = 4;
// Newton leaf sums (newton.hip; newton_core.h has the rule): the rows of cr routed through `tree` (leaves [leaf0, leaf0 + n_leaves)) by the code walk,
// acc[l][2 D + 1] += (q(g)[D], q(h)[D], 1) with q(x) = llrint((double)x * 2^bits), g and h the objective's (kObjLogistic: targets float32 [.][D];
// kObjSoftmax: int32 labels in [0, D), checked by the caller) at pred -- the prediction over the trees [0, tree).  pred and targets are indexed by
// the position j < m, or with abs_index by the data set row position j names.  acc (device, n_leaves * (2 D + 1) + 1 words, ZEROED by the caller on
// `s`): the last word collects kNewtonBadTarget / kNewtonBadPred.  D <= 128.  Returns true when the streaming kernel took the launch.
// weights (nullable, device float32, indexed like pred): q(fl32(w * g)) and q(fl32(w * h)) are summed; bits is then newton_sum_bits(m, weight_max).
void newton_check_targets(const float *targets, size_t n_el, unsigned long long *flag /*device, zeroed by the caller*/, hipStream_t s);   // *flag |= kNewtonBadTarget: an entry outside [0, 1] (a NaN counts)
bool newton_leaf_sums(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int tree, int leaf0, int n_leaves, const float *pred,
                      const void *targets, bool abs_index, int objective, int bits, unsigned long long *acc, bool generic, hipStream_t s,
                      const float *weights = nullptr);
// Leaf quantiles (leaf_quantile.hip; quantile_core.h has the rule): the rows of cr routed through `tree` (leaves [leaf0, leaf0 + n_leaves)) by the code
// walk; per (leaf, output d) the k-th largest x = fl32(pred - targets) among the leaf's rows, k = quantile_rank(rows of the leaf, alpha[d]).  pred and
// targets (device float32 [.][D]) are indexed by the position j < m, or with abs_index by the data set row position j names; alpha is device float32 [D]
// (every level checked by the caller).  res (device uint32, leaf_quantile_result_words(n_leaves, D) words, ZEROED by the caller on `s`): the selected keys
// [n_leaves][D] (quantile_key_value gives the float; 0 for an empty leaf), the ranks [n_leaves][D], the rows per leaf [n_leaves], and the flag word
// (kQuantileBadPred / kQuantileBadTarget / kQuantileBadResidual).  The plan decides the path once per call: the select path (an MSD radix select per
// (leaf, output), trees of up to max_select_leaves leaves) or the general path (radix_sort.hip: by key, then stably by leaf id; needs leaf_quantile_fits:
// m * D < 2^31 - kRadixSortTile) -- generic forces the latter.  Two different algorithms, the same bytes.  scratch holds plan.scratch_bytes.  D <= 128.
struct LeafQuantilePlan { bool select = false; size_t scratch_bytes = 0; };
inline size_t leaf_quantile_result_words(int n_leaves, int D) { return 2 * static_cast<size_t>(n_leaves) * D + n_leaves + 1; }
void leaf_quantile_geometry(int *max_select_leaves, int *rows_per_chunk);
bool leaf_quantile_fits(int m, int D);
LeafQuantilePlan leaf_quantile_plan(int m, int D, int n_leaves, bool generic);
void leaf_quantile(const PredictModel &pm, const CodeTables &ct, const CodeRows &cr, int m, int tree, int leaf0, int n_leaves, const float *pred,
                   const float *targets, bool abs_index, const float *alpha, const LeafQuantilePlan &plan, void *scratch, uint32_t *res, hipStream_t s);
// ... and the bias of a fresh model by the same rule: one leaf of every row of targets [n][D] at p = 0, the select path's passes.  res as above with
// n_leaves = 1 (ZEROED by the caller): bias_d = -quantile_key_value(res[d]); the flag word collects kQuantileBadTarget.
void leaf_quantile_check_targets(const float *targets, size_t n_el, uint32_t *flag /*device, zeroed by the caller*/, hipStream_t s);   // *flag |= kQuantileBadTarget: an entry that is not finite
size_t leaf_quantile_bias_scratch_bytes(int n, int D);
void leaf_quantile_bias(const float *targets, int n, int D, const float *alpha, void *scratch, uint32_t *res, hipStream_t s);
// Every prefix [0, stops[s]) of the ensemble in one walk (predict_staged.hip): stage s has the bits of predict_continue(tiled bias, 0, stops[s]);
// stops[s] == 0 is the bias alone.  `stops` is a device array, strictly ascending, 0 <= stops[s] <= n_trees (the caller has checked);
// last_stop = stops[n_stops - 1].  Predict mode (targets == nullptr): out[s][r][j], device [n_stops][n][D].  Loss mode (targets != nullptr,
// device [n][D]): sums[s] = the float64 sum of (double)g * (double)g, g = fl32(p - y), over all rows and outputs, reduced in a fixed order --
// part is scratch for n_stops x staged_loss_partials(n) doubles, sums holds n_stops.  generic: the one-thread-per-row kernel only
// (GBRL_HIP_STAGED_GENERIC=1; same bytes in both modes).  Always launches.
struct StagedStops { const int32_t *stops; int n_stops; int last_stop; };
int staged_loss_partials(int n);
void predict_staged(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, const StagedStops &st, float *out,
                    const float *targets, double *part, double *sums, bool generic, hipStream_t s);
// The loss stage of predict_staged for predictions the caller already holds (device [n][D]): *sum = what sums[s] is for a stage with these
// bits -- the same row sums, butterflies and finishing tree.  part: scratch for staged_loss_partials(n) doubles.
void staged_loss_of_predictions(const float *preds, const float *targets, int n, int D, double *part, double *sum, hipStream_t s);
// its two halves: the partials alone (one per 64 consecutive rows), and the finishing sum of nb partials that any of the loss kernels wrote
void loss_partials_of_predictions(const float *preds, const float *targets, int n, int D, double *part, hipStream_t s);
void staged_loss_finish(const double *part, int nb, double *sum, hipStream_t s);
// ... of n_rows vectors of nb partials each, part[r][0 .. nb) -> sums[r]: the same kernel, one block per vector (predict_staged's own finishing launch)
void staged_loss_finish_rows(const double *part, int nb, int n_rows, double *sums, hipStream_t s);
// Where a row lands (predict_leaves.hip): the GLOBAL leaf index -- the row of `values` -- that each tree of [start_tree, stop_tree) routes a row to.
// Oblivious: tree_indices[t] + the bits of the tree's conditions.  Greedy: the first leaf in storage order from tree_indices[t] on whose conditions
// all hold; a depth-0 leaf never passes (Q7), and -1 when the search runs off the ensemble.  No leaf value is read: no limit on output_dim.
// predict_leaves: out is device int32 [n][stop_tree - start_tree], row-major (the caller keeps n * trees < 2^31).
// leaf_counts: counts is device uint32 [n_leaves], ZEROED by the caller on `s`; counts[l] += rows that reach leaf l.  The counters of a run of
// trees are kept in LDS (at most kLeafCountChunk per launch; longer ranges are cut into runs of whole trees, one launch each, the rows re-read
// per run) and added to `counts` once per block.  tree_first_leaf: the HOST copy of tree_indices (the runs are planned on the host).
// generic: the one-thread-per-row kernels only (GBRL_HIP_LEAVES_GENERIC=1; same bytes).  Both always launch.
constexpr int kLeafCountChunk = 4096;   // 16 KiB of counters behind the 64-row tile
int leaf_counts_chunk();
void predict_leaves(const PredictModel &pm, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree, int stop_tree, int32_t *out,
                    bool generic, hipStream_t s);
void leaf_counts(const PredictModel &pm, const int32_t *tree_first_leaf, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                 int stop_tree, uint32_t *counts, bool generic, hipStream_t s);

// Refit the leaf values of the trees [start_tree, stop_tree) on a batch, the structure kept (refit.hip).  Everything is enqueued on `s`; nothing
// is read back and the host never waits.  Per tree t, in order: g = fl32(P - targets); the fixed point 2^lbits from gmax[t - start_tree] by the
// step's rule (leaf_sum_bits_dev, n = the rows of this call); per leaf of the tree, routed as predict_leaves routes, the exact int64 sums of
// llrint((double)g * 2^lbits) and the row count (integer atomics: the same bytes on every run and on both kernel families); the new value
// (float)(sum / 2^lbits / count), mixed as decay * old + keep * mean (two rounded float64 products, one rounded sum) when decay != 0 -- a leaf
// without rows and a leaf of depth 0 keep the old value; P = fma(-rate(t, o), new value, P) for every optimizer o that owns the output (a row
// whose greedy search left the tree keeps its P and joins no sum); gmax[t + 1 - start_tree] from the new P.  pm.values is only read.
//   P           [n][D]      scratch; on return the prediction of the refitted ensemble over [0, stop_tree): predict_continue's bits
//   leaf_idx    [n]         scratch: the global leaf of the current tree per row
//   acc         [leaves of the range][D + 1] int64 sums | count, ZEROED by the caller on `s`; acc + (tree_first_leaf[t] - tree_first_leaf[start]) * (D + 1)
//   new_values  [leaves of the range][D]: the result (rows of `values` from tree_first_leaf[start_tree] on)
//   gmax        [trees of the range + 1] uint32, ZEROED by the caller: the bits of max |g| before each tree and, last, of the final P; a NaN
//               as +inf; the caller rejects the run when one is not finite
// tree_first_leaf: the HOST copy of tree_indices.  generic: the one-thread-per-row kernels only (GBRL_HIP_REFIT_GENERIC=1; same bytes).
// Returns the number of trees whose accumulate pass took the streaming kernel (a diagnostic: the tests pin the path with it).
int refit_leaves(const PredictModel &pm, const int32_t *tree_first_leaf, const float *obs, int F, const int32_t *cat_codes, int Fc, int n, int start_tree,
                 int stop_tree, double decay, const float *targets, float *P, int32_t *leaf_idx, unsigned long long *acc, float *new_values,
                 uint32_t *gmax, bool generic, hipStream_t s);

// ---- Linear TreeSHAP (shap.hip): a uniform program over explicit trees, one thread per (sample, output) ----
enum { SHAP_ENTER = 0, SHAP_AFTER_LEFT = 1, SHAP_AFTER_RIGHT = 2, SHAP_EXIT = 3 };
struct ShapOp { int32_t kind, node, level, via; };   // via: feature tested by the parent (-1 at a root)
struct ShapNodeRec {                                  // explain.h ShapNode, flattened; node indices are global over the program
    int32_t feature, flags /*1 numeric, 2 tied to parent, 4 leaf, 8 right child*/, cat_id, pred;
    int32_t n_unique, n_unique_parent, deg_left, deg_right;
    float threshold, weight, weight_parent, pad;
};
int shap_block_threads(int max_depth, int D);   // 0: this (max_depth, D) does not fit the kernel (LDS) -- evaluate on the host
// out [n_samples][n_num + n_cat][D] is accumulated into (zero it first)
void shap_values(const ShapOp *ops, int n_ops, const ShapNodeRec *nodes, const float *leaf_value, const float *obs, int n_num,
                 const int32_t *cat_ids, int n_cat, int n_samples, int D, int max_depth, const float *norm, const float *base,
                 const float *offset, float *out, hipStream_t s);
// The same kernel with the numeric cells read from a prepared data set's bin codes: sample j of the m is row cr.rows[cr.row0 + j] (or cr.row0 + j)
// of cr.codes, and a node record's `threshold` holds the condition's BIN (int32, bit cast; x > v <=> code > bin).  No categorical conditions.  out
// [m][n_features][D] is accumulated into (zero it first).  shap_block_threads(max_depth, D) != 0: the caller checks.
void shap_values_codes(const ShapOp *ops, int n_ops, const ShapNodeRec *nodes, const float *leaf_value, const CodeRows &cr, int n_features, int m, int D,
                       int max_depth, const float *norm, const float *base, const float *offset, float *out, hipStream_t s);
// The column sums of values [rows][n_cols] (device, n_cols = features x outputs) by shap_core.h's rule.  shap_reduce_tiles: one float64 partial per 64
// consecutive rows, column and kind into part[tile0 + t][2][n_cols] (t = the tile of the chunk; kind 0 the sum, 1 the sum of fabs).  shap_reduce_finish:
// sums [2][n_cols] = the partials of all `tiles` tiles added in ascending order.
void shap_reduce_tiles(const float *phi, int rows, int n_cols, double *part, int tile0, hipStream_t s);
void shap_reduce_finish(const double *part, int tiles, int n_cols, double *sums, hipStream_t s);

}  // namespace kern
}  // namespace gbrl
