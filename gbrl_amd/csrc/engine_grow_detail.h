// engine_grow_detail.h -- what the growth paths of Engine::grow_tree share (engine_grow.hip: the dispatcher, the constant tables, the
// one-launch growth and the host bookkeeping; engine_grow_levels.hip: the level loops and the final leaves): the per-tree constants, the
// view of a level's result block, the chunk tables and the TreeBuilder that books a level's decisions into the host tree.
#pragma once
#include "engine_step_detail.h"

namespace gbrl {
namespace detail {

// Per-tree constants derived from the step's context, computed once by grow_tree and read-only afterwards.
struct GrowDims {
    GrowDims(const GrowCtx &c, bool has_coll, int world_size, int rank, Engine::Parity parity);
    int max_front, max_nodes, max_chunks;
    bool l2_degenerate;      // L2 with ONE row: the reference's unbiased variance is 0/0 (math_ops.cpp:461-513), every standardised gradient and
                             // every split score is NaN, no comparison succeeds and the tree stays a depth-0 leaf (fitter.cpp:357, :458)
    size_t table_cap, stage_bytes;
    // A level is one balanced round of (chunks x feature groups) histogram blocks, one block per CU: 256 / n_groups chunks, at least
    // 32 (few features => more, smaller chunks; the chunk length only has an upper bound, `chunk_rows`, from the fixed-point scale).
    int hist_chunk_budget, hist_max_chunks;
    size_t n_acc, hist_node_elems, feat_elems;
    // Row-sharded runs exchange the level histograms by FEATURE: the local sums of the accumulated nodes are laid out
    // [owner rank][node][feature of the rank's slice] and reduce-scattered, so every rank receives the GLOBAL sums of its own
    // Fs = ceil(Fp / P) features only (half the bytes of an all-reduce on the xGMI ring), scores its own candidates, and the
    // level's winner is agreed with ONE small all-reduce (kern::winner_pack / winner_adopt).
    int coll_P, coll_Fs, coll_lo, own_slots;   // ranks, features per rank slice, first feature (= feature slot) of this rank, its slots
    // Small levels are all-reduced WHOLE instead (round 6): every rank then holds the global sums of all features, scores all candidates
    // and resolves the winner itself -- no winner exchange, no score fill, one exchange per level instead of two.  The all-reduce moves
    // twice the reduce-scatter's bytes, so it pays while that difference costs less than the winner's small all-reduce and its three
    // launches: up to ~10 MB of level payload on xGMI (8 ranks: (P-1)/P x 10 MB at ~200 GB/s bus bandwidth ~ 45 us against a ~25 us
    // all-reduce + ~20 us of launches; unmeasured beyond one GPU -- GBRL_HIP_HIST_ALLREDUCE_MAX_KB tunes it, 0 = always reduce-scatter).
    size_t ar_max_bytes;
    int am_parts;
    size_t am_cap;           // greedy: one arg-max part per feature slot
    size_t res_bytes;        // one level's result block (ResultBlock)
    // Near-tie replay (neartie.hip; one GPU, batches of <= 65 536 rows): the selection also tracks the best DISTINCT runner-up; a node whose
    // runner-up is within `near_rel` of the winner (or whose winning gain is that close to zero) has the candidates in the window re-scored
    // in the reference's float32 sequence.  GBRL_HIP_NO_NEARTIE_REPLAY=1: the exact arg-max decides everywhere (rounds 1-4).
    // Batches above 65 536 rows: at 2^20 rows x 32 768 candidates EVERY level has a runner-up inside the reference's float32 noise, and the
    // replay's chains are serial (a 2^20-row level costs 10-100 ms against a 1.85 ms step: profiles/r06_neartie_fullsize_cost.txt), so those
    // batches replay only on request -- GBRL_HIP_NEARTIE_MAX_ROWS=<n>: nodes of up to n rows (0: every node).  Unset: the exact arg-max, as in
    // rounds 1-5.  Batches of up to 65 536 rows replay every flagged node as before.
    // The model's parity setting (Engine::Parity, gbrl_hip_set_parity_mode) says the same per model: "reference" = GBRL_HIP_NEARTIE_MAX_ROWS=
    // <max_node_rows>, "exact_argmax" = GBRL_HIP_NO_NEARTIE_REPLAY=1, "default" = neither.  A hook that is set overrides the setting and does
    // what it always did: NO_NEARTIE_REPLAY turns the replay off whatever the mode, NEARTIE_MAX_ROWS turns it on with its limit for batches
    // above 65 536 rows whatever the mode (NO_NEARTIE_REPLAY wins over it).  near_on and near_max_rows are the ONLY outcome of all three:
    // every growth path (one-launch kernel, level loop; step() and fit()) reads them and nothing else.
    bool near_on;
    float near_rel;          // 2^-20 unless GBRL_HIP_NEARTIE_REL (measurement hook) says otherwise
    int near_max_rows;       // 0: no limit, -1: no replay
    bool reference_asked;    // the model's own setting is "reference" and GBRL_HIP_NO_NEARTIE_REPLAY does not override it: grow_tree refuses the paths that cannot replay
    bool event_results;      // GBRL_HIP_EVENT_RESULTS=1 (measurement hook): results through the copy engine and an event
};

// Device addresses of the step's constant tables (Engine::upload_step_tables).
struct StepTables {
    FeatureSlot *slots;
    float *cand_w;
    int32_t *cand_ref, *ref_to_internal, *cand_slot;
};

// One level's result block as the kernels write it, in device or host memory:
// [best_idx i32 x mf][best_score f32 x mf][counts i64 x 4 x mf]; the one-launch kernel appends the winners' thresholds [f32 x mf].
struct ResultBlock {
    char *base;
    size_t mf;
    static size_t bytes(int max_front) { return static_cast<size_t>(max_front) * (4 + 4 + 32) + 64; }
    int32_t *best_idx() const { return reinterpret_cast<int32_t *>(base); }
    float *best_score() const { return reinterpret_cast<float *>(base + 4 * mf); }
    int64_t *counts() const { return reinterpret_cast<int64_t *>(base + 8 * mf); }
    int64_t *total() const { return counts(); }                 // rows of the node (global)
    int64_t *right() const { return counts() + mf; }            // rows of its right child (global)
    int64_t *right_local() const { return counts() + 2 * mf; }  // row-sharded: this rank's rows of the right child
    int64_t *near_flags() const { return counts() + 2 * mf; }   // one GPU: near-tie flag of the node (k_resolve_splits) ...
    int64_t *near_second() const { return counts() + 3 * mf; }  // ... and the bits of its runner-up's gain
    float *win_thr() const { return reinterpret_cast<float *>(base + 40 * mf); }
};

// Chunk table of a list of nodes: the chunks, and per node the index of its first chunk (+ one end entry).
struct ChunkTable {
    std::vector<Chunk> chunks;
    std::vector<int32_t> begin;
};
// Equal parts of at most rows_per_chunk rows per node.  slot_is_node_id: the chunks carry the node's id instead of its position in `ids`
// (leaf sums), and the root gets none (Q7).
ChunkTable make_chunks(const std::vector<HNode> &nodes, const std::vector<int> &ids, int rows_per_chunk, bool slot_is_node_id);
// smallest chunk length t (<= chunk_rows) for which the nodes `ids` need at most `budget` chunks in total
int balanced_chunk_rows(const std::vector<HNode> &nodes, const std::vector<int> &ids, int chunk_rows, int budget);

// (categorical feature, class) -> index into cat_cands, built at the first categorical split of the step (a linear search per
// splitting node walked 2 000 x 136-byte records: 50 us per level at level 5 of configs[4])
struct CatIndex {
    std::vector<int> index, off;
    int find(const std::vector<CatCandidate> &cat_cands, int Fc, int feat, int cls);
};

// How digest_level reads a result block: the level loops pass the default, the one-launch growth sets all three.
struct DigestMode {
    const float *win_thr = nullptr;   // the winners' threshold values travel with the level's result block
    bool lazy_paths = false;          // children do not copy their parent's path (in_cond[id] = the condition into node id)
    bool counts_later = false;        // the node sizes are derived from the leaves' row counts after the replay
};
struct LevelOutcome { bool stop = false; std::vector<int> splitting, new_leaves, next; };

// The host tree of one step while it grows: `nodes`, `frontier` (the unsplit nodes of the current level) and the bookkeeping that turns a
// level's result block into decisions, children and paths.  Shared by all three growth paths.
class TreeBuilder {
   public:
    TreeBuilder(const GrowCtx &c, bool row_sharded, std::vector<HNode> &nodes, std::vector<int> &frontier)
        : nodes(nodes), frontier(frontier), c_(c), row_sharded_(row_sharded) {}
    std::vector<HNode> &nodes;
    std::vector<int> &frontier;
    void reset(int max_nodes);   // the root alone
    // nodes that take part at a level: oblivious -> the whole level; greedy -> nodes with rows (fitter.cpp:300)
    std::vector<int> active_nodes() const;
    LevelOutcome digest_level(const std::vector<int> &active, const ResultBlock &res, const DigestMode &mode);
    // After the one-launch growth's levels were digested with lazy paths: leaf marks, the leaves' sums from the kernel's accumulators,
    // (oblivious) node sizes and edge weights from the leaves' row counts, and the leaves' paths.
    void finish_small(const int64_t *h_acc, uint32_t kernel_nodes, std::vector<int64_t> &acc);

   private:
    const GrowCtx &c_;
    bool row_sharded_;
    CatIndex cat_index_;
    std::vector<HCond> in_cond_;
};

// Device workspace and stream position of the level loops (Engine::level_workspace); `cur`, `iota_root` and `ar_prefix` move with the levels.
struct LevelWork {
    int32_t *rows[2];        // the two row lists; rows[cur] is current
    int32_t *rows_scratch;   // what rows[0] becomes again once the cached root list has been partitioned
    bool iota_root = false;  // rows[0] is the cached list 0 .. N-1 (read-only)
    int cur = 0;
    bool ar_prefix = false;  // row-sharded: every level so far was all-reduced whole (a reduce-scattered level leaves only this rank's
                             // feature slice in the level buffer, and the next level's sibling subtraction reads that buffer)
    int32_t *partials;
    int64_t *hist_lvl[2];    // current / previous level, so that the larger child of every split can be derived as parent - sibling
    int64_t *hist_coll, *hist_recv, *gather;
    float *scores, *parent, *am_v, *am_s;
    int32_t *am_i, *am_n;    // am_n: child sizes tell classes apart in larger batches only (score_common.h near_class)
    int32_t *cursors;
    int64_t *leafacc;
    ResultBlock d_res;       // device copy of the level's results
    // The block also lives in pinned host memory that the device can write: a one-block kernel publishes it (k_publish_block) and the host
    // polls a sequence word behind it -- no copy-engine launch, no event, and the partition kernel starts right behind the selection.
    ResultBlock h_res;
    volatile uint32_t *h_flag;
    void *h_res_dev;
    uint32_t *d_flag;
    unsigned *d_pub_done;
    NodeSplit *resolved;
};

// One level of the host loop: which nodes are accumulated, its descriptor tables on the host and (stage A) on the device.
struct Level {
    int depth = 0, n_act = 0;
    std::vector<int> active, compute_ids;
    std::vector<int32_t> slot_map;
    ChunkTable hist;                               // chunks of the accumulated nodes
    std::vector<Chunk> count_chunks, part_chunks;  // row-sharded child counting / the partition: all active nodes
    bool hist_direct = false, root_countless = false, ar_level = false, drop_derived = false;
    int root_mode = 1, lvl_slots = 0, lvl_lo = 0;  // the feature slots this rank scores at this level
    int64_t *d_hist = nullptr;
    const int64_t *d_hist_prev = nullptr;
    Chunk *d_chunks, *d_count_chunks, *d_part_chunks;
    int32_t *d_chunk_begin, *d_slotmap, *d_sub_par, *d_sub_sib, *d_path_len, *d_path_slot, *d_path_bin, *d_isroot, *d_seg_starts, *d_n_locals;
    float *d_path_val;
};

}  // namespace detail
}  // namespace gbrl
