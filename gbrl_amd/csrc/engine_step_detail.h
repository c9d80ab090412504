// engine_step_detail.h -- what the translation units of step() share:
//   engine_candidates.hip  numeric split candidates: the threshold route and one function per route (A3, A4)
//   engine_cat_candidates.hip  categorical split candidates: the device scan in stages, the forms of its result, the sharded ranking (A5);
//                          cat_candidates_host.h has their host half (the reference's rule, the replay of its container), which needs no device
//   engine_grow.hip        Engine::grow_tree: the choice of the growth path, the one-launch growth of RL-sized steps, the host tree's bookkeeping
//   engine_grow_levels.hip Engine::grow_levels: the level loops and the final leaves (A6-A10); engine_grow_detail.h has what these two share
//   engine_step.hip        Engine::step in stages / Engine::fit, the tree joining the ensemble (A1, A2, A10-A11), and
//                          the stages step() shares with step_prepared(): run_grad_stats, prepare_numeric, grow_step_tree
//   engine_prepared.hip    Engine::prepare_dataset / Engine::step_prepared: a batch binned once and stepped on many times
//   engine_codes.hip       Engine::condition_bins / predict_continue_prepared: a data set's bin codes in the model's terms, the walk over them
//   engine_objective.hip   Engine::objective_gradient[_host] / eval_metric[_host]: an objective's checks, gradient, loss and metric of a prediction matrix
//   engine_leaves.hip      Engine::newton_leaves_prepared[_rank] / quantile_leaves_prepared: one tree's leaf values from a data set's rows
//   engine_fit_prepared.hip  Engine::fit_prepared: fit()'s loop on a data set, in stages over one FitRun (engine_codes_detail.h: what these four share)
//   engine_importance.hip  Engine::permutation_importance_prepared / permutation_host: the loss of a data set's rows with one column shuffled
//   engine_pd.hip          Engine::partial_dependence_prepared / partial_dependence_codes: the predictions of a data set's rows with columns held constant
#pragma once
#include "engine.h"
#include "hooks.h"

#include <numeric>
#include <random>
#include "cat_hash.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <unordered_map>


namespace gbrl {


using kern::Chunk;
using kern::FeatureSlot;
using kern::NodeSplit;


namespace detail {

struct HCond {       // splitCondition (types.h:64-70) + what the kernels need
    int fslot;       // feature slot (numeric f, or F + categorical c)
    int feat_idx;    // feature index as stored in the model (within its numeric / categorical block)
    float value;     // numeric threshold, +inf for categorical (split_candidate_generator.cpp:155)
    int bin;         // numeric: threshold index; categorical: class id
    bool is_cat;
    bool dir;
    float edge_w;
    int cat_cand;    // index into cat candidate strings, -1 for numeric
};

struct HNode {
    int depth = 0;
    int seg_start = 0;
    int n_local = 0;        // rows of this rank in the node
    long long n_global = 0;  // rows over all ranks
    std::vector<HCond> path;
    int left = -1, right = -1;
    int parent = -1;
    int hist_slot = -1;     // slot of this node's histogram in its level's buffer
    bool leaf = false;
};

// Everything Engine::grow_tree needs from the preparation stages of step().
struct GrowCtx {
    int N, F, Fc, D, B, MD, NB, FG, Fp, n_groups, n_slots, n_cand, chunk_rows;
    long long n_global;
    bool cosine, oblivious;
    const std::vector<kern::FeatureSlot> *slots;
    const std::vector<float> *cand_w;
    const std::vector<int32_t> *cand_ref;
    const std::vector<int> *ref_to_internal;
    const std::vector<int32_t> *cand_slot;
    bool const_cacheable;               // numeric-only step: the constants above live in Engine::step_const_
    const std::vector<CatCandidate> *cat_cands;
    bool prefix_cacheable;     // mixed step: numeric table prefixes stay on the device, categorical tails are uploaded per step
    int n_num_cand, cand_cap;  // numeric candidates (= prefix length), capacity of the fixed table layout
    char *pub_thr_dev, *pub_scales_dev; // device addresses of the pinned copies below (kern::publish_pair / the growth kernel write them)
    size_t pub_thr_bytes;
    const float *h_thr;                 // pinned; valid once the stream has passed the copy enqueued behind the binning
    const kern::StepScales *h_scales;   // pinned, same
    const float *d_thr;
    const uint32_t *d_thrkeys;   // [F][B] ordered keys of the thresholds
    const uint32_t *root_le;     // [F][B] #{keys <= threshold} from the radix selection (one GPU, numeric-only steps), else null
    const uint32_t *d_kt;        // [F][N] feature-major ordered keys of the observations (null when F == 0)
    const uint16_t *d_codes;
    const uint16_t *d_codes_fm;  // [F][N] feature-major copy of the numeric codes (fused preparation only), else null
    const int32_t *d_qg;
    const float *dgrads;
    const float *d_meanden;      // L2: [D] mean | [D] std + 1e-8f of the build gradients' standardisation; null for Cosine (raw gradients)
    kern::StepScales *d_scales;
};

// A histogram block accumulates one chunk of one node's rows.  Chunks are sized per level so that the whole level is ONE balanced round of
// <= 32 chunks x (feature groups) blocks (k_hist_build keeps one block per CU); `chunk_rows` is the cap the fixed-point scale is derived from.
// It depends on the GLOBAL row count only (clamped to [4096, 65536]), so the scale -- and with it every integer sum -- is the same for any
// sharding of the same rows.
inline int chunk_rows_of(long long n) { return static_cast<int>(std::min<long long>(65536, std::max<long long>(4096, 2 * ((n + 31) / 32)))); }

// The gradient statistics of a step (A2) and where they land: Engine::run_grad_stats fills them, Engine::prepare_numeric hands them to the fused
// preparation kernel when step() asks for it (`fuse`), and calls `run` behind that launch when the kernel did not cover them.
struct FusedStats {
    const float *dgrads;
    int D;
    bool cosine;
    double *d_stat;             // [4 D]
    float *d_meanden;           // [2 D]
    kern::StepScales *d_scales;
    int32_t *d_qg;              // [N][D]
    int chunk_rows;
    bool fuse;                  // !GBRL_HIP_NO_SMALL_STATS
    bool done = false;          // the statistics have been enqueued
};

// Everything Engine::grow_step_tree needs about a batch: the numeric preparation (the engine's workspace, or a PreparedDataset's buffers), the
// gradient statistics, and this step's categorical candidates (none for a prepared data set).
struct StepData {
    int N, F, Fc;
    long long n_global;
    int chunk_rows;
    NumericPrep prep;
    const FusedStats *stats;
    const std::vector<CatCandidate> *cat_cands;
    const std::vector<int> *cat_classes;
    const int32_t *cols = nullptr;      // step_prepared(cols): feature f of this step is the model's feature cols[f] (its candidate weight; host, F entries)
};

// A view of the distinct cells a publish delivered (engine_cat_candidates.hip): hdr = [list overflow, hash collision, distinct cells, records
// delivered]; per record its raw hash, feature, row of first occurrence and 128 bytes (in ordinary memory, or still in the pinned block), and
// -- CatPub modes with statistics only -- kern::cat_rank's count and float32 total.  Row-sharded: the gathered global list (no first rows).
struct CatList {
    const int32_t *hdr, *feat, *first;
    const uint64_t *hash;
    const char *names;
    const int32_t *count;
    const float *total;
    bool names_in_pinned;
};
// what a publish carries: the records; the records and the ranking statistics; only the statistics of records that a publish with the same
// capacity has already delivered (their feature, first row, hash and cell stay where they are)
enum class CatPub { Records, RecordsAndStats, StatsOnly };

// Engine::numeric_thresholds: the batch and where its thresholds go; the routes, chosen once by Engine::threshold_route
struct ThrArgs { const float *dobs; int N, F, B; long long n_global; const uint32_t *d_kt; float *d_thr; uint32_t *d_thrkeys; };
enum class ThrRoute { Fixed, Uniform, Bisection, LdsSort, Radix, Sample };

// Engine::step: the batch as the caller handed it over, and where its three inputs lie on the device
struct StepInputs {
    const float *obs; bool obs_dev; const char *cat; bool cat_dev; const float *grads; bool grads_dev;
    int N, F, Fc;
    const float *dobs = nullptr, *dgrads = nullptr;
    const char *dcells = nullptr;
};
// Engine::categorical_stage: this step's candidates and classes, and where the class codes come from -- the scan's tables, a dictionary
// on the device, or codes the host rules computed
struct CatStage {
    enum Codes { None, Table, Dict, Host } codes = None;
    std::vector<CatCandidate> cands;
    std::vector<int> classes;
    std::vector<uint16_t> h_codes;
};

}  // namespace detail

using detail::CatCandidate;
using detail::chunk_rows_of;
using detail::FusedStats;
using detail::StepData;
using detail::GrowCtx;
using detail::HCond;
using detail::HNode;

namespace detail {

// Packs many small host arrays into one pinned block and uploads them with ONE async copy; put() returns the DEVICE
// address the array will have.  The pinned block must not be refilled before the copy has executed (the caller's
// per-level synchronisation guarantees it).
class Stager {
   public:
    Stager(PinnedBuf &pin, DevBuf &dev, size_t cap, hipStream_t s) : s_(s) {
        host_ = static_cast<char *>(pin.ensure(cap));
        dev_ = static_cast<char *>(dev.ensure(cap));
        cap_ = cap;
    }
    void reset() { used_ = 0; }
    template <typename T>
    T *put(const T *src, size_t n) {
        const size_t bytes = n * sizeof(T);
        if (used_ + bytes + 256 > cap_) throw HipError("internal: staging buffer overflow");
        if (bytes) std::memcpy(host_ + used_, src, bytes);
        T *d = reinterpret_cast<T *>(dev_ + used_);
        used_ += (bytes + 255) & ~static_cast<size_t>(255);
        return d;
    }
    template <typename T>
    T *reserve(size_t n) {     // the device address put() would return, without touching the host copy (the block is already uploaded)
        const size_t bytes = n * sizeof(T);
        if (used_ + bytes + 256 > cap_) throw HipError("internal: staging buffer overflow");
        T *d = reinterpret_cast<T *>(dev_ + used_);
        used_ += (bytes + 255) & ~static_cast<size_t>(255);
        return d;
    }
    void flush() {
        if (used_) hip_check(hipMemcpyAsync(dev_, host_, used_, hipMemcpyHostToDevice, s_), "H2D staged descriptors");
    }
    const void *device_base() const { return dev_; }
    char *host_base() const { return host_; }

   private:
    hipStream_t s_;
    char *host_ = nullptr, *dev_ = nullptr;
    size_t cap_ = 0, used_ = 0;
};

// GBRL_HIP_DEVICE_LEVELS=1 (opt-in device-planned level loop)
inline bool device_levels_requested() { return hooks::on(hooks::DEVICE_LEVELS); }
// Host side of the copy-free hand-overs (engine_candidates.hip)
void spin_until_published(volatile uint32_t *flag, uint32_t seq, hipStream_t s, const char *what);
// split_candidate_generator.cpp:216-249 (engine_candidates.hip)
std::vector<int64_t> quantile_target_ranks(long long n_global, int B);
// A10-A11 (engine_step.hip)
void append_tree(Model &model, const std::vector<HNode> &nodes, const std::vector<int> &frontier, const std::vector<int64_t> &acc,
                 double leaf_scale, const std::vector<CatCandidate> &cat_cands);
// Row subsets of a prepared data set (engine_prepared.hip).  checked_rows: device copy of an index vector, every entry known to lie in [0, n)
// BEFORE anything reads through it: a host vector is checked on the host (check_host_rows, before the device is touched), a device vector by
// kern::rows_minmax, read back.  check_row_count: m rows of `noun` against the data set's n before either ("... (pass rows to `verb` a subset)").
const int32_t *checked_rows(DevBuf &copy, DevBuf &mm_buf, const int32_t *rows, bool rows_dev, int m, int n, hipStream_t s);
void check_host_rows(const int32_t *rows, int m, int n);
void check_row_count(const char *what, const char *noun, const int32_t *rows, int m, int n, const char *verb);

}  // namespace detail

using detail::Stager;
using detail::device_levels_requested;
using detail::spin_until_published;
using detail::quantile_target_ranks;
using detail::categorical_candidates;
using detail::append_tree;
using detail::checked_rows;
using detail::check_host_rows;
using detail::check_row_count;

}  // namespace gbrl
