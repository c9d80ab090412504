// engine.h -- device engine: owns the host model, its device mirror, the per-step workspace and the HIP stream, and
// drives the kernels of the step_*.hip units for GBRL::step / GBRL::predict.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <array>
#include <initializer_list>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "cat_candidates_host.h"   // HipError, Unsupported; detail::CatCandidate, CatMemory
#include "mirror_records.h"        // detail::GreedyNodes, RateTable, CatDict: the host half of the device mirror

namespace gbrl {

struct NoDeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct InvalidArgument : std::runtime_error { using std::runtime_error::runtime_error; };

void hip_check(hipError_t e, const char *what);

// grow-only device buffer
class DevBuf {
   public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf();
    void *ensure(size_t bytes);  // contents are NOT preserved when it grows
    void *ensure_keep(size_t bytes, size_t keep_bytes, hipStream_t s);  // preserves the first keep_bytes
    template <typename T>
    T *as() const { return static_cast<T *>(ptr_); }
    const void *raw() const { return ptr_; }
    size_t capacity() const { return cap_; }
    void release();

   private:
    void *ptr_ = nullptr;
    size_t cap_ = 0;
};

// grow-only pinned host buffer (async copies from/to it do not stage through pageable memory)
class PinnedBuf {
   public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf();
    void *ensure(size_t bytes);

   private:
    void *ptr_ = nullptr;
    size_t cap_ = 0;
};

// The numeric preparation of a batch -- everything the growth paths read about the observations (detail::GrowCtx: d_thr, d_thrkeys, root_le, d_kt,
// d_codes, d_codes_fm) lands in one buffer set: the engine's per-step workspace for step(), a PreparedDataset's own for prepare_dataset().
struct PrepBuffers {
    DevBuf kt;         // [F][N] feature-major ordered keys of the observations (the partition's 4-byte reads)
    DevBuf codes;      // [ceil(slots / 16)][N][16] u16 class codes, group-major
    DevBuf thr;        // [F][B] thresholds
    DevBuf thrkeys;    // [F][B] ordered keys of the thresholds
    DevBuf codes_fm;   // [F][N] feature-major copy of the numeric codes (kern::small_prep -> kern::small_grow)
    DevBuf root_le;    // [F][B] + [F]: #{keys <= threshold} from the radix selection
};
// What a preparation left in its buffer set (null: this path does not produce it; both are legal inputs of the growth paths).
struct NumericPrep {
    float *d_thr = nullptr;
    uint32_t *d_thrkeys = nullptr;
    uint16_t *d_codes = nullptr;
    const uint32_t *d_kt = nullptr;
    const uint16_t *d_codes_fm = nullptr;
    const uint32_t *root_le = nullptr;
};

// Extension: a batch of numeric observations binned ONCE (Engine::prepare_dataset) and stepped on many times (Engine::step_prepared) -- LightGBM's
// Dataset, XGBoost's QuantileDMatrix.  It owns its device buffers and is only ever read after its creation: any model on the same device with the
// same n_bins, generator_type and input_dim == F may step on it, several models may share one.  include/gbrl_hip.h has the contract.
class PreparedDataset {
   public:
    int n = 0, F = 0, n_bins = 0, generator_type = 0, device = -1;
    uint64_t id = 0;               // unique per data set of the process (a handle's address can come back)
    uint64_t thresholds_id = 0;    // the id of the data set the thresholds were selected for: its own id, or -- bound to a reference
                                   // (Engine::prepare_dataset_like), through any chain -- the reference's.  What an engine's code tables are keyed on:
                                   // the bins of a condition depend on the thresholds and on nothing else.
    PrepBuffers buf;
    NumericPrep prep;              // pointers into buf
    std::vector<float> h_thr;      // host copy of the thresholds [F][B]
    int code_groups() const { return (F + 15) / 16; }
    size_t nbytes() const {        // device bytes held + the host copy
        return buf.kt.capacity() + buf.codes.capacity() + buf.thr.capacity() + buf.thrkeys.capacity() + buf.codes_fm.capacity() + buf.root_le.capacity() +
               h_thr.size() * sizeof(float);
    }
    // the codes on the host (diagnostics; the data set's device, the null stream): out [G][m][16]; rows == nullptr: every row (m = n), else what
    // kern::gather_code_records gives for rows (int32 [m], host or device, every entry in [0, n) or InvalidArgument)
    // cols (host, as Engine::step_prepared's): out [ceil(n_cols / 16)][m][16], the subset's records from kern::gather_code_columns
    void codes_to_host(const int32_t *rows, bool rows_dev, int m, uint16_t *out, const int32_t *cols = nullptr, int n_cols = 0) const;
};

namespace detail {
struct GrowCtx;
struct HNode;
struct StepData;
struct FusedStats;
struct GrowDims;
struct StepTables;
struct LevelWork;
struct Level;
class TreeBuilder;
class Stager;
struct ThrArgs; struct StepInputs; struct CatStage; struct CatList; enum class ThrRoute;   // engine_step_detail.h
// The device scan for a step's distinct categorical cells (engine_cat_candidates.hip): its buffers, what the next step starts from, the
// round that is on the stream, and the form its result takes for the class-code kernels.
struct CatScan {
    DevBuf keys, first, meta, lslot, slotq, clsq;   // per-feature tables (hash | first row), flags + counter, the list's table slots, slot -> record, record -> class
    DevBuf rank, rank_cnt, rank_tot, sdict, xchg;   // kern::cat_rank: scratch, count and total per distinct cell; the step's dictionary; scratch of the row-sharded exchanges
    PinnedBuf pin, pin_cls, pin_dict;               // the published block; the class of every record; the dictionary as the host packs it
    std::vector<char> host;                         // the published block, copied out of the pinned mapping
    uint32_t pub_seq = 0;                           // sequence word of k_cat_publish's completion flag
    int log2_hint = 20, publish_guess = 256;        // the next step starts with: log2 of the per-feature table size (20: the full size); records published with the header (the last count + 25 %)
    bool launched = false;                          // a first round is on the stream, not yet collected
    int log2_cap = 0, full_log2 = 0, list_cap = 0, pub_cap = 0;   // that round: table size, the worst case's, capacity of the list and of the publish
    // ordinary steps on one GPU: the class codes come from the scan's own tables (k_cat_step_codes_table) instead of a dictionary
    struct { bool valid = false; const uint64_t *keys = nullptr; const int32_t *slot_q = nullptr, *cls_of_q = nullptr; int log2_cap = 0; } table;
    // the step's candidate dictionary inside sdict (one upload): per categorical feature the entries sorted by raw hash
    struct { const int32_t *off = nullptr, *cls = nullptr; const uint64_t *hash = nullptr, *words = nullptr; } dict;
};
}  // namespace detail

// The options of Engine::fit_prepared; the defaults are the plain MultiRMSE loop on every row and column.
struct FitOptions {
    double subsample = 1.0, colsample = 1.0; uint64_t seed = 0; int objective = 0 /* kern::kObjRmse */; int metric = 0 /* kern::kMetricNone */;
    int leaf_update = 0 /* kern::kLeafGradient; 1: kern::kLeafNewton; 2: kern::kLeafQuantile */; double leaf_l2 = 1.0;
    const float *weights = nullptr /* float32 [n], one per data set row; nullptr: the loop without weights */; bool weights_dev = false;
    double goss_top = 0.0, goss_other = 0.0 /* 0: off; else sample_core.h's one-side sampling takes the place of the subsample draw */;
    const float *alpha = nullptr /* host float32 [D]: the levels of kern::kObjQuantile (quantile_core.h); required with it, refused without it */;
    const int32_t *group = nullptr /* host int32 [n_groups]: the query sizes of a ranking objective (rank_core.h); required with one, refused without */;
    int n_groups = 0; int ndcg_at = 0 /* kern::kObjLambdarank: discounts from this position on count as 0; 0: no truncation */;
};

class Engine {
   public:
    explicit Engine(const gbrl_hip_config &cfg);
    explicit Engine(Model &&loaded, int device_ordinal);
    Engine(const Engine &other);  // deep copy of the model (GBRL::GBRL(GBRL&)); fresh device state
    ~Engine();

    Model model;

    void step(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *grads, bool grads_dev, int n,
              int n_num, int n_cat);
    // Extension (engine_prepared.hip): the numeric preparation of step() -- key transpose, thresholds, class codes, on the same code paths -- into
    // a data set of its own, and a step on it.  prepare_dataset waits for the stream: `obs` is not needed afterwards.  step_prepared runs the
    // gradient statistics, grows the tree from the data set's buffers and appends it; with rows == nullptr the model ends up byte for byte as
    // step(obs, nullptr, grads) would leave it.  rows (int32 [m], host or device, duplicates allowed, every entry in [0, n)): the tree is grown on
    // those m rows with THE DATA SET'S thresholds (not the quantiles of the subset; what fit() does with whole-data-set candidates), grads is
    // [m][D] in the order of rows.  Numeric-only, one GPU.  Every argument error is raised before the device is touched, an out-of-range index
    // before anything reads through it; after any failure the model is unchanged.
    PreparedDataset *prepare_dataset(const float *obs, bool obs_dev, int n, int n_num);
    // Extension: a data set BOUND to another one's thresholds (LightGBM's Dataset(reference=train)).  obs [n][ref->F] is binned against the
    // reference's threshold keys in one pass (kern::bin_like: no transpose, no selection); the result owns its codes and its own copies of the
    // thresholds, their keys and the host thresholds -- the reference may be destroyed -- and inherits the reference's thresholds_id.  It holds
    // no keys, no feature-major codes and no root table: a step on it hands them over as null, as a subset step does.  Refused before the
    // device is touched: what check_prepared_dataset refuses about (model, reference), n <= 0, null obs.  The model is never changed.
    PreparedDataset *prepare_dataset_like(const PreparedDataset *ref, const float *obs, bool obs_dev, int n);
    // cols (host int32 [n_cols], strictly ascending, entries in [0, ds->F), 1 <= n_cols <= F; anything else is InvalidArgument before anything
    // changes): the tree is grown on those columns only.  The records of the subset (and of rows, in the same pass: kern::gather_code_columns), the
    // thresholds and their keys are gathered into the workspace, the growth paths run on F' = n_cols features with the candidate weight the full
    // step gives feature cols[f'], and every condition's feature index is rewritten through cols before the tree is appended: the model is what
    // a model of input_dim F' with feature weights w[cols] grows on prepare_dataset(obs[:, cols]), with A's indices == cols[B's].  Ascending
    // order keeps the tie rule (the lowest candidate index wins).  cols covering every column is the call without cols.
    void step_prepared(const PreparedDataset *ds, const float *grads, bool grads_dev, const int32_t *rows, bool rows_dev, int m, const int32_t *cols = nullptr,
                       int n_cols = 0);
    static void check_cols(const char *what, const int32_t *cols, int n_cols, int F);   // the rule above (cols non-null)
    // Extension (engine_codes.hip): the walk over a data set's bin codes.  code(r, f) = #{b : thr[f][b] < obs[r, f]}, so a numeric condition
    // x[f] > v whose v is one of thr[f][*] is code > bin with bin = #{b : thr[f][b] < v} (include/gbrl_hip.h has the argument).
    // condition_bins: host only.  out has the length and indexing of feature_values; a used numeric slot (d < depths[split row]) gets its bin,
    // every other slot -1.  thresholds [F][B]; F / B that are not the model's: InvalidArgument; a used numeric condition whose value is not
    // among its feature's thresholds (float ==; NaN never is): Unsupported, naming the tree and the condition.
    void condition_bins(const float *thresholds, int F, int B, int32_t *out) const;
    // predict_continue_prepared: out [m][D] = base carried through [start_tree, stop_tree) for the data set rows rows[0..m) (rows == nullptr: every
    // row, m == ds->n) -- bit for bit predict_continue on the observations the data set was made from.  Ranges and base / out as predict_continue,
    // rows as step_prepared.  Refused before the device is touched: what step_prepared refuses about the model and the data set, output_dim > 128,
    // a tree of the range (greedy: through the first tree with a split behind the range's trailing depth-0 trees, which the walk runs into) with a
    // condition that is not among the data set's thresholds (Unsupported).  The model is never changed.
    void predict_continue_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *base, bool base_dev, int start_tree,
                                   int stop_tree, float *out, bool out_dev);
    // Extension (engine_importance.hip; perm_core.h has the permutation, perm_loss.hip the kernels): permutation importance on a data set.
    // *baseline_out = the loss of the trees [0, n_trees) on ds's rows against targets, walked from the bias, in the units of fit_prepared's
    // loss_out for the objective (mean_loss over ds->n rows); loss_out [n_cols][n_repeats] (host) = the same loss with column cols[c] read from
    // row perm(ds->n, seed, cols[c], r)(i) -- bit for bit fit_prepared's validation loss on a data set that holds the shuffled column.  cols
    // (host, check_cols' rule; nullptr: every column, n_cols ignored); n_trees in [1, model's] or -1 for all.  objective: rmse, logistic,
    // softmax, quantile (alpha then, host [D]); targets as fit_prepared's (host or device).  A column no condition of the walked trees tests is
    // not launched: its entries are the baseline.  At most kern::kPermLaunchVariants variants per launch; nothing but loss partials is stored.
    // Refused before the device is touched: n_repeats < 1, check_cols, n_trees, null targets or outputs, a model without trees, check_objective
    // (the ranking objectives), check_alpha, and what predict_continue_prepared refuses about the model and the data set.  A softmax label
    // outside [0, D) is refused once the labels are on the device.  Model and data set are never changed.
    void permutation_importance_prepared(const PreparedDataset *ds, const void *targets, bool targets_dev, int objective, const float *alpha, int n_repeats,
                                         uint64_t seed, const int32_t *cols, int n_cols, int n_trees, double *baseline_out, double *loss_out);
    static void permutation_host(int n, uint64_t seed, int col, int repeat, int32_t *out);   // the rule on the host: out [n] = perm(n, seed, col, repeat)
    // Extension (engine_pd.hip; pd_core.h has the break rule and the launch plan, pd_rows.hip the kernels): partial dependence and ICE on a data set.
    // partial_dependence_codes: host only.  out [*count] (room for B + 1 entries) = [0] + [bin + 1 for the sorted distinct bins of the numeric
    // conditions on column col that the walk of the trees [0, n_trees) reads] (n_trees == -1: all; greedy: through the trees a trailing run of
    // one-leaf trees runs on into, as check_code_range counts them), the bins being condition_bins' for thresholds [F][B].  Segment j is the code
    // range [out[j], out[j + 1] - 1], the last one runs to B; every code of a segment answers every walked condition on col alike.  A column no
    // walked condition tests: [0].  Only the column's walked conditions are converted.  Refused: null arguments, F / B that are not the model's
    // (InvalidArgument, as condition_bins), col outside [0, F), a model without trees, n_trees outside [1, model's], a walked condition on col whose
    // value is not among thr[col][*] (Unsupported, naming the tree).
    void partial_dependence_codes(const float *thresholds, int F, int B, int col, int n_trees, int32_t *out, int *count) const;
    // partial_dependence_prepared: for each of the V variants {col0, code0, col1, code1} (host; col1 == -1: one column; col0 == -1: the baseline, col1
    // then -1 too) the trees [0, n_trees) are walked from the bias over the rows rows[0..m) of ds (rows == nullptr: every row, m == ds->n; host or
    // device, duplicates allowed, as step_prepared's) with column col0 (and col1) read as the constant code for every row.  sums_out (host float64
    // [V][D]) = the sum over the rows of (double)p[r][d] in a fixed order: one partial per 64 consecutive positions of the row list
    // (predict_loss.h's butterfly), finished by kern::staged_loss_finish_rows -- two calls give the same bytes.  ice_out (nullable; host or device
    // float32 [V][m][D]) = the rows themselves, bit for bit predict_continue_prepared from a tiled bias over [0, n_trees) on a data set that holds
    // those codes.  A column of a variant that no walked condition tests is dropped from it; a variant left without a column IS the baseline: it is
    // not launched and reports the baseline's bits, and so does every variant of a model in which no optimizer owns an output.  At most
    // kern::pd_launch_variants(m, D) variants per launch (the partial scratch stays under pd_core.h's budget), ONE read-back of the sums.
    // Refused before the device is touched (InvalidArgument unless noted): what predict_continue_prepared refuses about the model, the data set and
    // rows (output_dim > 128: Unsupported), a model without trees, n_trees outside [1, model's] and not -1, V < 1 or null variants / sums_out, a
    // column outside [0, F) (or below -1), col0 == col1, col0 == -1 with col1 >= 0, a code outside [0, B], more than 2^20 launched variants,
    // V * m * D >= 2^31 with ice_out (Unsupported: pass rows).  Model and data set are never written.
    void partial_dependence_prepared(const PreparedDataset *ds, const int32_t *variants /*[V][4]*/, int V, const int32_t *rows, bool rows_dev, int m, int n_trees,
                                     double *sums_out, float *ice_out, bool ice_dev);
    // fit_prepared: fit()'s loop (shuffle = false) on a data set with nothing recomputed.  Each iteration takes the next batch_size rows (wrapping to
    // row 0), advances their held prediction by the trees grown since the batch last saw it -- one launch that also writes the objective's gradient
    // -- and grows one tree by step_prepared's body; at the end every batch is advanced and the loss on all rows returned (fit()'s MultiRMSE; an
    // objective's sum / rows in float64, the row losses reduced as MultiRMSE's are).  A fresh model first gets its bias; a model with trees keeps
    // it and continues from ALL its trees (unlike fit()).
    //   objective  (objective_core.h; kern::kObjRmse / kObjLogistic / kObjSoftmax)  rmse, logistic: targets float32 [n][D]; softmax: int32 [n] labels
    //              in [0, D), valid->targets likewise.  The bias, in double: the column means; log(c / (1 - c)), c = clamp(column mean, 1 / 2n,
    //              1 - 1 / 2n); log(max(n_c, 0.5) / n), n_c counted on the device (kern::label_counts, which also finds a label out of range).
    //   subsample  < 1: the tree grows on a sample of its batch, drawn once prediction and gradient are up to date with draw = the tree count before
    //              the step (a continued fit continues the sequence); the gradient rows are gathered in the same pass and m is read back (4 bytes).
    //              A draw that keeps no row takes the whole batch.  == 1 IS the unsampled loop: no sampler launch, no gather, no phase.
    //   goss       goss_other > 0 (sample_core.h: one-side sampling): the draw of the iteration is kern::sample_goss over the batch, on G as the held
    //              prediction's launch left it (with weights: the scores are those of fl32(w * g)), draw = the tree count before the step; tau stays on
    //              the device and m is read back (4 bytes), as for subsample.  A draw that keeps no row takes the whole batch unamplified.  newton: the
    //              sums run over the kept rows with the effective weights e_r = fl32(w_r * factor_r) (w_r = 1 without weights), written by absolute row
    //              by the sampler's write pass; the quantum's weight_max is fl32(wmax * amp).  Refused: check_goss's list, goss with subsample < 1, and
    //              fl32(wmax * amp) > kWeightMax once the weights are known, before any tree is grown.  goss_other == 0 enqueues nothing new.
    //   colsample  < 1: and on sample_cols_host's columns for the same seed and draw, by step_prepared's cols path; == 1, or a draw of every column
    //              (F == 1): nothing of it runs.  The held prediction, validation, the stopping rule and the loss see all rows and columns.
    //   valid      a set with ds's thresholds_id (it may be ds).  loss_out[k], k = 0 .. done, is the loss of the first T0 + k trees (T0: the count at
    //              entry) on its rows -- rmse: staged_loss's expression and summation order, bit for bit -- from a second held prediction advanced
    //              after EVERY iteration by one launch that also writes the loss partials.  rounds > 0: the loop ends after iteration k when k - best
    //              >= rounds (early_stop_scan's rule); rounds == 0: record only.  All trees grown stay: model and loss are what the call without
    //              valid gives for `done` iterations.  best_n_trees = T0 + best.
    //   metric     (metric_core.h; kern::kMetricError / kMetricAuc, with valid)  metric_out[k] is eval_metric_host of the validation rows' held
    //              prediction after k iterations, from integers counted on the device behind the loss launch (rounds == 0: they stay there
    //              until the end, as the loss sums do).  The stopping rule and best_n_trees then follow the metric curve -- the error as it is,
    //              the AUC negated -- in place of loss_out, which is recorded as ever.  It reads the held prediction only: the model is byte
    //              for byte what the call without it leaves after `done` iterations.
    //   leaf_update  (newton_core.h; kern::kLeafGradient / kLeafNewton)  newton: right after the step every leaf of the new tree gets sum g / (sum h +
    //              leaf_l2) over the rows the tree was grown on -- the batch, or the kept rows of a sampled iteration -- by newton_leaves_prepared's
    //              body on the held prediction (one launch, one read-back, the tree's value slice of the mirror sent again); the held predictions,
    //              the validation walk and the loss then see those values.  gradient enqueues nothing: the loop is the one without the option.
    //   weights    (objective_core.h, newton_core.h: row weights)  FitOptions::weights float32 [n], FitValid::weights [valid->ds->n].  The held
    //              prediction's launch stores fl32(w * g): the tree is grown on the weighted gradient, with the row counts of the split scores and
    //              min_data_in_leaf unchanged, and a gradient leaf stores the mean of w g over its rows.  newton: sum w g / (sum w h + leaf_l2), the
    //              quantum with room for the largest training weight of the data set.  The loss is sum w L / W, W the float64 sum of the weights in
    //              a fixed order (kern::weight_stats); a weighted rmse run takes it from the held prediction by the weighted objective_rows
    //              partials (the column sums of G hold (w g)^2).  A fresh model's bias: sum w y / W per column (kern::column_sums_weighted: the
    //              order of column_sums, so all-ones weights give the unweighted bits); its log odds, the clamp 0.5 / n kept; log(max(W_c, 0.5 W / n)
    //              / W), W_c the weight of class c.  valid->weights weigh valid->loss_out only; the metrics count rows (with a metric: Unsupported).
    //              A weight vector is checked once per call before anything changes (a NaN, negative, infinite entry or one above kWeightMax,
    //              naming the first row; W == 0).  No weights: the kernels and arguments of the call as it always was.
    // Refused before anything changes, in this order: precheck_fit's list; ds, then valid->ds, absent or not this model's (check_prepared_dataset);
    // another thresholds id; null valid->loss_out; a tree whose conditions the codes cannot express (Unsupported); softmax: a label outside [0, D)
    // in either set (InvalidArgument naming the first one found).
    struct FitValid {
        const PreparedDataset *ds; const void *targets; bool targets_dev; int rounds; double min_delta;
        double *loss_out /*[iterations + 1]*/; int done, best_n_trees;
        double *metric_out = nullptr /*[iterations + 1]; with FitOptions::metric*/;
        const float *weights = nullptr /*float32 [ds->n]: loss_out is the weighted loss*/; bool weights_dev = false;
        const int32_t *group = nullptr /*host int32 [n_groups]: the validation set's query sizes (a ranking objective)*/; int n_groups = 0;
    };
    float fit_prepared(const PreparedDataset *ds, const void *targets, bool targets_dev, int iterations, const FitOptions &opt = {}, FitValid *valid = nullptr,
                       float *weight_max_out = nullptr);
    // What fit_prepared refuses without a data set in hand, in this order (the C ABI runs it before it resolves the handles, so that these
    // refusals do not depend on a data set being at hand; valid->ds is not looked at): the model checks of step_prepared; null targets;
    // iterations < 0; batch_size <= 0; max_depth > 32, n_bins outside [1, 65534], output_dim > 128 (Unsupported); check_subsample;
    // check_colsample; with goss_other != 0: check_goss, goss with subsample < 1; check_objective; check_leaf_update; a metric without valid, check_metric; with valid: null targets, rounds < 0, min_delta negative or NaN.
    void precheck_fit(const void *targets, int iterations, const FitOptions &opt, const FitValid *valid) const;
    // Extension: row subsampling (stochastic gradient boosting).  The sampler is sample_core.h's pure function of (seed, draw, row): a row is
    // kept iff its 24-bit hash is below floor(subsample * 2^24); the sample of [row0, row0 + n) is the ascending list of its kept absolute indices.
    // sample_rows_host: the rule itself on the host, out [n], *count = m.  sample_rows: the same list from the device kernels (kern::sample_rows)
    // on the data set's device and the null stream, as codes_to_host runs; out (int32 [n], host or device) gets the m kept rows, which may be
    // none.  Refused (InvalidArgument): row0 < 0, n <= 0, draw < 0, a subsample that is NaN or outside [2^-24, 1], null outputs, a range whose
    // last row is above 2^31 - 1, and for the data set call a range outside [0, ds.n).
    static void check_subsample(const char *what, double subsample);
    static void sample_rows_host(int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out, int *count);
    static void sample_rows(const PreparedDataset *ds, int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out, bool out_dev, int *count);
    // Extension: one-side sampling (GOSS; sample_core.h has the rule).  goss_rows_host: the rule on the host for the rows [row0, row0 + n) with gradient rows
    // G [n][D]: rows_out / factor_out [n] get the m kept rows and their factors (1 or amp), G_out (nullable, [n][D]) their gradient rows with the
    // factor applied, *count = m.  sample_goss: the same from the device kernels (kern::sample_goss) on the data set's device and the null stream; G,
    // rows_out, factor_out and G_out are all host or all device (io_dev); *n_top = floor(top_rate * n), *tau_bits = the k-th largest key (kGossNoTau
    // for k == 0), read back from the device.  Refused (InvalidArgument): check_goss's list (a NaN rate, top_rate outside [0, 1), other_rate outside
    // (0, 1], top_rate + other_rate > 1, other_rate / (1 - top_rate) < 2^-24), what sample_rows refuses about the range and the draw, D outside [1, 512].
    static void check_goss(const char *what, double top_rate, double other_rate);
    static void goss_rows_host(const float *G, int D, int row0, int n, double top_rate, double other_rate, uint64_t seed, int draw, int32_t *rows_out,
                               float *factor_out, float *G_out, int *count);
    static void sample_goss(const PreparedDataset *ds, const float *G, int D, int row0, int n, double top_rate, double other_rate, uint64_t seed, int draw,
                            int32_t *rows_out, float *factor_out, float *G_out, bool io_dev, int *count, int *n_top, uint32_t *tau_bits);
    // The engine's fused sampler + gather on the CURRENT device and the null stream (what fit_prepared's loop enqueues per iteration; the tests
    // reach it through gbrl_hip_sample_gather): device G [n][D] -> device rows_out [n], G_out [n][D], *count = m.
    static void sample_gather(int row0, int n, double subsample, uint64_t seed, int draw, const float *G, int D, int32_t *rows_out, float *G_out, int *count);
    // Extension: column subsampling (colsample_bytree / feature_fraction).  The rule is sample_core.h's: k = max(1, floor(colsample * F + 0.5))
    // columns, the k smallest (u_f, f) with u_f the 24-bit hash of (seed ^ "colsampl", draw, f), ascending.  Host only.  sample_cols_host: out
    // [F], *count = k.  Refused (InvalidArgument): F < 1, draw < 0, a colsample that is NaN or outside (0, 1], null outputs.
    static void check_colsample(const char *what, double colsample);
    static void sample_cols_host(int F, double colsample, uint64_t seed, int draw, int32_t *out, int *count);
    // Extension: classification objectives.  Refused (InvalidArgument): an unknown objective, softmax with D < 2.
    static void check_objective(const char *what, int objective, int D);
    // objective_gradient: grad_out [n][D] = dL/dp and / or *loss_out = the loss of pred [n][D] against targets under the objective, on the model's
    // device and stream with D = output_dim (kern::objective_rows: the device functions of the code walk's tails).  grad_out is where pred is
    // (device iff pred_dev); either output may be null, not both.  kObjRmse: g = fl32(p - y) and staged_loss's expression.
    // weights (nullable, float32 [n]): grad_out = fl32(w * g), the loss sum w L / W (rmse: sqrt(0.5 sum w L / W)); checked as fit_prepared checks them.
    // alpha (host float32 [D]): the levels of kObjQuantile -- required with it, refused with another objective, as are weights with kObjQuantile.
    void objective_gradient(const float *pred, bool pred_dev, const void *targets, bool targets_dev, int n, int objective, float *grad_out, double *loss_out,
                            const float *weights = nullptr, bool weights_dev = false, const float *alpha = nullptr);
    // Extension: ranking objectives on query groups (rank_core.h has the rule, include/gbrl_hip.h the contract; engine_rank.hip).  rank_gradient:
    // scores pred float32 [n] of a model with output_dim 1, labels int32 [n], group HOST int32 [n_groups] -- the sizes of consecutive row runs --
    // under kObjPairwise or kObjLambdarank, on the model's device and stream (kern::rank_queries, kern::rank_rows).  grad_out, hess_out float32 [n]
    // and pos_out int32 [n] are where pred is (device iff pred_dev); ndcg_out float64 [n_groups] and pairs_out are host; every output may be null.
    // Refused before a kernel runs (InvalidArgument): output_dim != 1, another objective, no group, a size outside [1, kRankMaxQuery] (the first such
    // query is named), sizes that do not sum to n, ndcg_at < 0, ndcg_at > 0 with kObjPairwise; after the label pass: a label outside
    // [0, kRankMaxLabel] (the first such row is named); after the launch: a score that is not finite.  rank_gradient_host: the rule without a
    // device; no loss for kObjPairwise (a device-only float64 expression, as the logistic loss is), so loss_out is then refused.
    static void check_rank_group(const char *what, const int32_t *group, int n_groups, int n /* < 0: not known yet, the sum is not checked */, int objective,
                                 int ndcg_at, int D, const char *name = "group");
    void rank_gradient(const float *pred, bool pred_dev, const int32_t *labels, bool labels_dev, const int32_t *group, int n_groups, int n, int objective,
                       int ndcg_at, float *grad_out, float *hess_out, double *loss_out, double *ndcg_out, int32_t *pos_out, int64_t *pairs_out);
    static void rank_gradient_host(const float *pred, const int32_t *labels, const int32_t *group, int n_groups, int n, int objective, int ndcg_at,
                                   float *grad_out, float *hess_out, double *loss_out, double *ndcg_out, int32_t *pos_out, int64_t *pairs_out);
    static const double *rank_discounts();   // the table of kRankMaxQuery discounts, built once
    // newton_leaves_prepared for a ranking objective (engine_leaves.hip): g and h are rank_gradient's at pred [n] (labels int32 [n], group host) over EVERY row of the data
    // set (a row list would cut queries apart), written to device buffers and summed per leaf by kern::newton_leaf_sums' buffer form (kObjGiven);
    // bits = newton_sum_bits(n, (float)largest group), since |g| and h are below the query size.  Refusals: newton_leaves_prepared's about the model, the
    // data set and the tree, rank_gradient's about the rest.
    void newton_leaves_prepared_rank(const PreparedDataset *ds, const float *pred, bool pred_dev, const int32_t *labels, bool labels_dev, const int32_t *group,
                                     int n_groups, int objective, int ndcg_at, int tree, double leaf_l2, int64_t *sums_out, int *bits_out, float *values_out);
    // Extension: quantile regression (quantile_core.h has the rule, include/gbrl_hip.h the contract).  check_alpha: alpha with another objective,
    // kObjQuantile without alpha, weights with kObjQuantile (Unsupported), a level that is not finite and strictly inside (0, 1) (the output is named).
    static void check_alpha(const char *what, int objective, const float *alpha, int D, bool weighted);
    // quantile_leaves_prepared: the leaves of ONE tree (tree == -1: the last) get v[leaf][d] = the k-th largest x = fl32(pred - targets) among the
    // data set rows rows[0..m) (rows == nullptr: every row, m == ds->n) the tree routes to the leaf, k = quantile_rank(rows of the leaf, alpha[d]);
    // pred and targets are [m][D], indexed by position.  A leaf without rows or of depth 0 keeps its value.  values_out (nullable) float32 [leaves][D]
    // what the model now holds, counts_out (nullable) int64 [leaves], ranks_out (nullable) int64 [leaves][D] (0 for an empty leaf).  Only model.values
    // of that tree changes, and only its slice of the device mirror is sent again.  Refused before anything changes: what newton_leaves_prepared
    // refuses about the model, the data set, rows, the tree and output_dim; a bad level.  Refused after the launch, the model unchanged
    // (InvalidArgument): a prediction, a target or a residual that is not finite.
    void quantile_leaves_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *pred, bool pred_dev, const float *targets,
                                  bool targets_dev, const float *alpha, int tree, float *values_out, int64_t *counts_out, int64_t *ranks_out);
    // the rule on the host (no device): x float32 [m][D], leaves int32 [m] (an entry outside [0, n_leaves) joins no leaf) -> values_out float32
    // [n_leaves][D] (0 for an empty leaf), counts_out int64 [n_leaves], ranks_out int64 [n_leaves][D]; any output may be null
    static void leaf_quantile_host(const float *x, const int32_t *leaves, int m, int D, int n_leaves, const float *alpha, float *values_out, int64_t *counts_out,
                                   int64_t *ranks_out);
    static int64_t quantile_rank(int64_t m, float a);   // clamp(ceil(a * m), 1, m), the product exact; a bad level or m < 1 is refused
    // Extension: row weights.  The checks of a weight vector on the host (InvalidArgument naming the first refused row); on the device the same
    // through kern::weight_stats, with the largest weight and W = the float64 sum in its fixed order (need_sum: W == 0 is refused too).
    static void check_weights_host(const char *what, const float *weights, int n);
    struct WeightStats { float max = 0.0f; double sum = 0.0; };
    WeightStats check_weights(const char *what, const float *d_weights, int n, bool need_sum);
    // Extension: classifier metrics (metric_core.h has the definitions).  eval_metric: the error rate or the exact AUC of pred [n][D] against
    // targets under the objective, on the model's device and stream: integer counts from kern::metric_error / kern::metric_auc, the value from
    // them on the host.  counts (nullable): [D][3] = (2U_d, P_d, N_d) for auc, [D] (softmax: [1]) for error.  eval_metric_host: the same by
    // std::sort on the host, no device.  Refused (InvalidArgument): an unknown metric, a metric with rmse, a label outside [0, D), a column
    // without a positive or without a negative row (auc; the column is named); (Unsupported): auc with softmax, n * D >= 2^31 - 2048 (auc).
    static void check_metric(const char *what, int objective, int metric);
    void eval_metric(const float *pred, bool pred_dev, const void *targets, bool targets_dev, int n, int objective, int metric, double *value, int64_t *counts);
    static void eval_metric_host(const float *pred, const void *targets, int n, int D, int objective, int metric, double *value, int64_t *counts);
    // Extension: Newton leaf values (newton_core.h has the rule, include/gbrl_hip.h the contract).  newton_leaves_prepared: the leaves of ONE tree
    // (tree == -1: the last) get v = (sum g) / (sum h + leaf_l2) over the data set rows rows[0..m) (rows == nullptr: every row, m == ds->n), g and h
    // the objective's at pred [m][D] -- the caller's prediction over the trees [0, tree), indexed by position like targets ([m][D] float32, or int32
    // [m] labels for softmax).  The sums are exact int64 (kern::newton_leaf_sums) and the value is computed from them on the host in double; a leaf
    // without rows, of depth 0, or with sum h + leaf_l2 <= 0 keeps its value.  sums_out (nullable) int64 [leaves][2 D + 1] = (Sg, Sh, cnt),
    // *bits_out the bits of the quantum, values_out (nullable) float32 [leaves][D] what the model now holds.  Only model.values of that tree
    // changes, and only its slice of the device mirror is sent again.  Refused before anything changes: what predict_continue_prepared refuses
    // about the model, the data set and rows; output_dim > 128; the rmse objective (its Newton step is the gradient mean: InvalidArgument); a
    // leaf_l2 that is negative, NaN or infinite; a tree outside the model; a softmax label outside [0, D).  Refused after the launch, the model
    // unchanged (InvalidArgument): a logistic target outside [0, 1] (a NaN counts), a prediction that is not finite.
    // weights (nullable, float32 [m], indexed by position): Sg += q(fl32(w g)), Sh += q(fl32(w h)), bits = newton_sum_bits(m, weight_max); weight_max < 0:
    // the largest of the weights given; otherwise it must be at least that and at most kWeightMax (a caller's loop over sampled rows passes the
    // maximum of the whole data set and gets fit_prepared's bits).  A weight_max >= 0 without weights is refused.
    void newton_leaves_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *pred, bool pred_dev, const void *targets,
                                bool targets_dev, int objective, int tree, double leaf_l2, int64_t *sums_out, int *bits_out, float *values_out,
                                const float *weights = nullptr, bool weights_dev = false, float weight_max = -1.0f);
    static void check_leaf_update(const char *what, int objective, int leaf_update, double leaf_l2);   // unknown update, newton with rmse, a bad leaf_l2
    // the hessian rule on the host (no device): out [n][D] = obj_logistic_hess(p) / the diagonal softmax hessian q (1 - q); targets are not read
    static void objective_hessian_host(const float *pred, int n, int D, int objective, float *hess_out, const float *weights = nullptr /*[n]: fl32(w * h)*/);
    // the value rule on the host (no device): sums int64 [leaves][2 D + 1], old_values float32 [leaves][D], depths int32 [leaves] -> values_out [leaves][D]
    static void newton_values_host(const int64_t *sums, int n_leaves, int D, int bits, const float *old_values, const int32_t *depths, double leaf_l2,
                                   float *values_out);
    // the gradient rule on the host (no device): the same bits
    static void objective_gradient_host(const float *pred, const void *targets, int n, int D, int objective, float *grad_out,
                                        const float *weights = nullptr /*[n]: fl32(w * g)*/, const float *alpha = nullptr /*[D]: kObjQuantile's levels*/);
    // the stopping rule on a curve (host only): best = index of the minimum so far from k = 0, entry k improves iff curve[k] < curve[best] -
    // min_delta (a NaN never improves); *stop_after = the first k with k - best >= rounds (rounds > 0), else n - 1; *best = best at that point
    static void early_stop_scan(const double *curve, int n, int rounds, double min_delta, int *stop_after, int *best);
    // the model checks of step_prepared, for the C ABI calls that run them before they resolve a data set handle
    void precheck_prepared(const char *what) const { check_prepared_model(what); }
    void predict(const float *obs, bool obs_dev, const char *cat, bool cat_dev, int n, int n_num, int n_cat, int start_tree,
                 int stop_tree, float *out, bool out_dev);
    // Extension (not in the reference, which compares the 128-byte cells inside every predict call): the dictionary ids of a batch of
    // categorical cells, and predict from such ids.  `token` identifies the model's category dictionary (a hash of its entries in order): ids are
    // valid for any model whose dictionary is the same (this model until a later tree mentions a new category, its clones, its saved file).
    void encode_categorical(const char *cat, bool cat_dev, int n, int n_cat, int32_t *ids_out, bool out_dev, uint64_t *token);
    void predict_encoded(const float *obs, bool obs_dev, const int32_t *cat_ids, bool ids_dev, uint64_t token, int n, int n_num, int n_cat,
                         int start_tree, int stop_tree, float *out, bool out_dev);
    // Extension: continue a held prediction.  `base` [n][D] is the caller's prediction over the trees [0, start_tree); out[r][j] is base[r][j]
    // carried through the trees [start_tree, stop_tree) in tree order -- p = fma(-lr_o(t), value, p) for every optimizer o that owns output j,
    // lr_o(t) = scheduler_lr at the absolute tree index; an output no optimizer owns keeps its base value and the bias is never added -- so the
    // result has the bits of one walk over [0, stop_tree).  Never sliced over tree ranges, at any batch size.  stop_tree == 0: n_trees;
    // start_tree == stop_tree: out = base; start_tree > stop_tree or stop_tree > n_trees: InvalidArgument.  out == base is allowed.
    void predict_continue(const float *obs, bool obs_dev, const char *cat, bool cat_dev, int n, int n_num, int n_cat, int start_tree,
                          int stop_tree, const float *base, bool base_dev, float *out, bool out_dev);
    void predict_continue_encoded(const float *obs, bool obs_dev, const int32_t *cat_ids, bool ids_dev, uint64_t token, int n, int n_num,
                                  int n_cat, int start_tree, int stop_tree, const float *base, bool base_dev, float *out, bool out_dev);
    // Extension: every ensemble prefix in one walk.  `stops` (host, n_stops > 0) is a strictly ascending list of tree counts k, 0 <= k <= n_trees;
    // k == 0 is the bias alone -- unlike predict's stop_tree, 0 never means "all trees" here.  Stage s is, bit for bit, what
    // predict_continue(base = tiled bias, 0, stops[s]) returns.  predict_staged: out [n_stops][n][D].  staged_loss: loss_out[s] (host) =
    // sqrt(0.5 * S / n) in float64, S the float64 sum of (double)g * (double)g, g = fl32(p - y), over all rows and outputs in a fixed order
    // (MultiRMSE as fit() defines it).  Errors (InvalidArgument / Unsupported) are raised before the device is touched.
    void predict_staged(const float *obs, bool obs_dev, const char *cat, bool cat_dev, int n, int n_num, int n_cat, const int32_t *stops, int n_stops,
                        float *out, bool out_dev);
    void staged_loss(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *targets, bool targets_dev, int n, int n_num, int n_cat,
                     const int32_t *stops, int n_stops, double *loss_out);
    // Extension: where a row lands.  For every tree t of [start_tree, stop_tree) the GLOBAL leaf index -- the row of `values`; minus tree_indices[t]
    // it is the index within the tree.  Oblivious: tree_indices[t] + sum_d pass(cond[t * max_depth + d]) << (depths[t] - 1 - d).  Greedy: the first
    // leaf in storage order from tree_indices[t] on whose conditions all hold (a depth-0 leaf never passes, Q7; -1 when the search runs off the
    // ensemble -- neither happens in a well-formed tree with a split).  stop_tree == 0: n_trees; then 0 <= start_tree < stop_tree <= n_trees or
    // InvalidArgument, as for a model without trees, the data set errors of predict and a stale dictionary token.  No leaf value is read: no
    // output_dim limit.  predict_leaves: out int32 [n][stop_tree - start_tree], row-major; n * trees >= 2^31 is Unsupported (slice the range).
    // leaf_counts: counts_out (host) int64 [n_leaves] over the WHOLE ensemble, entry l = rows of the batch that reach leaf l, 0 outside the range;
    // reduced on the device with integer atomics (two calls, the same bytes).  Every error is raised before the device is touched.
    // cat_ids != nullptr: pre-encoded cells and their dictionary token (the _encoded variants); cat is ignored then.
    void predict_leaves(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const int32_t *cat_ids, bool ids_dev, const uint64_t *token, int n,
                        int n_num, int n_cat, int start_tree, int stop_tree, int32_t *out, bool out_dev);
    void leaf_counts(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const int32_t *cat_ids, bool ids_dev, const uint64_t *token, int n,
                     int n_num, int n_cat, int start_tree, int stop_tree, int64_t *counts_out);
    // Extension: refit the leaf values of the trees [start_tree, stop_tree) on a batch, the structure kept (kern::refit_leaves; include/gbrl_hip.h
    // has the contract).  stop_tree == 0: n_trees; then 0 <= start_tree < stop_tree <= n_trees.  decay_rate in [0, 1]: new value = decay * old +
    // (1 - decay) * leaf mean of fit()'s MultiRMSE gradient.  Only model.values of the range changes; *loss_out = staged_loss(..., {stop_tree})
    // of the refitted model.  One enqueue for the whole range and one wait; every argument error is raised before the device is touched, a
    // run that meets a non-finite gradient is InvalidArgument, and after any failure the model (host and device mirror) is unchanged.
    // A model with a communicator or collective hooks is Unsupported (the sums would need an exchange per tree), and so is a greedy tree of
    // depth 0 among the trees [start_tree - 1, stop_tree) (the prediction walks past it into values that are not refitted yet).
    void refit_leaves(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *targets, bool targets_dev, int n, int n_num, int n_cat,
                      int start_tree, int stop_tree, double decay_rate, double *loss_out);
    // GBRL::fit (gbrl.cpp:983-1104) + Fitter::fit_cpu (fitter.cpp:117-261): bias = mean(targets), split candidates from the
    // WHOLE data set once, then `iterations` boosting rounds over consecutive batches of metadata.batch_size rows
    // (predict -> MultiRMSE gradients -> one tree per batch); returns the final MultiRMSE loss on the whole data set.
    float fit(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *targets, bool targets_dev, int n, int n_num,
              int n_cat, int iterations, bool shuffle);

    // Linear TreeSHAP of tree `tree_idx` (-1: every tree, summed in tree order) on the device; host pointers in and out, `out`
    // [n][n_num + n_cat][D] is overwritten.  Returns false when it was NOT computed (no HIP device, max_depth / output_dim beyond
    // the kernel's LDS budget, GBRL_HIP_SHAP_HOST=1): the caller then evaluates on the host (explain.cpp), which gives the same bits.
    // With GBRL_HIP_SHAP_DEVICE_ONLY=1 (test hook) the first two raise instead, so a result that came back was computed by k_shap.
    // Under set_profiling the phase `shap` is k_shap alone (the name the data-set calls give it too).
    bool shap_on_device(int tree_idx, const float *obs, const char *cat, int n, const float *norm, const float *base_poly,
                        const float *offset, float *out);
    // The same values from a prepared data set's bin codes (include/gbrl_hip.h, "SHAP values on a data set"): a numeric condition x > v is decided as
    // code > bin, everything else is k_shap's, so the result is shap_on_device's on the observations the codes were made from, byte for byte.
    // rows / rows_dev / m as step_prepared's (null: every row); tree_idx -1: every tree, summed in tree order.  norm / base_poly / offset: host,
    // built for max_depth.  out: float32 [m][F][D], host or device, overwritten.  There is no host evaluation behind it: a (max_depth, output_dim)
    // without a launch plan is Unsupported.  Refused before the device is touched: check_shap_prepared's list, and m * F * D >= 2^31.
    void shap_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int tree_idx, const float *norm, const float *base_poly,
                       const float *offset, float *out, bool out_dev);
    // sum_out / abs_out: host float64 [F][D], the sums over the m rows of phi and of |phi| for the whole ensemble by shap_core.h's rule (tiles of 64
    // positions, sequential float64): the bytes do not depend on chunk_rows (0: the default; else a positive multiple of 64), the matrix is never held
    // whole.  *chunk_rows_used (nullable): the chunk size the call worked with.
    void shap_importance_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, const float *norm, const float *base_poly,
                                  const float *offset, int chunk_rows, double *sum_out, double *abs_out, int *chunk_rows_used);

    void set_collective(const gbrl_hip_collective *hooks);
    // Native exchange: an RCCL communicator of this engine's own, collectives enqueued on its stream (no host sync).
    // id128 = gbrl_hip_rccl_unique_id() of rank 0, distributed by the caller.  Collective call (all ranks).
    void set_rccl(const void *id128, int world_size, int rank, bool keep_world1 = false);
    // Parity setting of this model (gbrl_hip_set_parity_mode): where the near-tie replay decides (GrowDims, engine_grow_detail.h).
    // Default: batches of up to 65 536 rows on one GPU.  Reference: every batch size, nodes of up to `max_node_rows` rows (0: every node;
    // the limit applies to batches above 65 536 rows only, smaller batches replay every flagged node).  ExactArgmax: nowhere.
    // Reference cannot hold row-sharded: Unsupported there, and set_collective / set_rccl refuse a model in that mode.
    enum class ParityMode { Default = 0, Reference = 1, ExactArgmax = 2 };
    struct Parity { ParityMode mode = ParityMode::Default; int max_node_rows = 0; };
    void set_parity(ParityMode mode, int max_node_rows);
    Parity parity() const { return parity_; }
    int device_ordinal();                 // latches the device like the first step()/predict() would
    void set_stream(hipStream_t s);       // nullptr: back to the engine's own blocking stream
    void set_profiling(int level) { profiling_ = level; }   // 0 off, 1 histogram build only (one launch in seven, every level in turn), 2 every phase
    void set_force_bisection(bool on) { force_bisection_ = on; }   // test hook: exercise the slow exact quantile path
    bool last_quantile_fallback() const { return last_quantile_fallback_; }
    const std::vector<std::pair<std::string, float>> &phase_times() const { return phases_; }

   private:
    void ensure_device();
    void sync_model_to_device();
    void rewind_values(int t);  // the values of tree t alone have changed (newton_leaves_prepared): the next sync appends them again from that tree on
    void invalidate_mirror();   // values of existing trees have changed (refit_leaves): the append-only mirror is uploaded again, the dictionary stays
    void sync_cat_dict();   // the host half of it: cat_dict_ / cat_ids_host_ follow the model (no device needed)
    // (the mirror, its dictionary and mirror_view are engine_mirror.hip's)
    int32_t *encode_categorical_batch(const char *cat, bool cat_dev, int n, int n_cat);
    // ---- the stages of a predict-family call, in the order every public call runs them (the head of engine_predict.hip has the list) ----
    // the observations as the caller handed them over: cells, or pre-encoded ids with their dictionary token (cat_ids != nullptr: cat is ignored)
    struct PredictBatch { const float *obs; bool obs_dev; const char *cat; bool cat_dev; const int32_t *cat_ids; bool ids_dev; const uint64_t *token; int n, n_num, n_cat; };
    struct StagedBatch { const float *obs; const int32_t *cat; };   // the same batch on the device: observations and dictionary ids
    struct ReadBack { void *host; const void *dev; size_t bytes; const char *what; };   // a result bound for the host (host == nullptr: it stays on the device)
    // GBRL::predict's data set checks, first-use bookkeeping of the feature counts included.  has_result: the call's result pointer is there;
    // width_limit: the call reads leaf values, which the kernels hold for up to 128 outputs
    void check_batch(const PredictBatch &b, bool has_result, bool width_limit);
    void check_dict_token(const PredictBatch &b);   // pre-encoded ids are valid only for the dictionary they were made from (host state: no device needed)
    void check_stops(const int32_t *stops, int n_stops) const;
    int check_leaves_range(int start_tree, int stop_tree) const;   // predict_leaves / leaf_counts: the resolved stop of a range the ensemble holds
    int check_refit(int start_tree, int stop_tree, const float *targets, double decay_rate, const double *loss_out) const;   // likewise (engine_refit.hip)
    StagedBatch stage_batch(const PredictBatch &b);   // device, event pool, mirror; opens the `inputs` phase: observations up, ids checked and uploaded or cells encoded
    const float *stage_targets(const float *targets, bool on_device, int n);   // [n][D] targets on the device
    kern::StagedStops stage_stops(const int32_t *stops, int n_stops);
    template <typename T>
    T *upload(DevBuf &buf, const T *host, size_t count, const char *what) {   // a host array into a grow-only device buffer, on the stream
        T *d = static_cast<T *>(buf.ensure(sizeof(T) * count));
        hip_check(hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, stream_), what);
        return d;
    }
    kern::PredictModel mirror_view();   // what the kernels read of the model and its mirror; predict() adds the routes it alone offers
    void finish(const char *launch, const char *phase, std::initializer_list<ReadBack> results);   // launch error, end of the key phase, read-backs, ONE wait, phase times
    void run_predict(const PredictBatch &b, int start_tree, int stop_tree, float *out, bool out_dev);   // predict / predict_encoded
    void run_continue(const PredictBatch &b, int start_tree, int stop_tree, const float *base, bool base_dev, float *out, bool out_dev);
    uint64_t cat_dict_token();
    void grow_tree(const detail::GrowCtx &c, std::vector<detail::HNode> &nodes, std::vector<int> &frontier, std::vector<int64_t> &acc,
                   double &leaf_scale);
    // the growth paths grow_tree chooses from (engine_grow.hip, engine_grow_levels.hip; engine_grow_detail.h has the structs)
    enum class SmallGrowth { Grown, NearTie, Unavailable };
    detail::StepTables upload_step_tables(const detail::GrowCtx &c, const detail::GrowDims &dims);
    SmallGrowth grow_small(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::StepTables &t, int blocks, detail::TreeBuilder &tb,
                           std::vector<int64_t> &acc, double &leaf_scale, const char *&why);
    void grow_levels(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::StepTables &t, detail::TreeBuilder &tb,
                     std::vector<int64_t> &acc, double &leaf_scale);
    detail::LevelWork level_workspace(const detail::GrowCtx &c, const detail::GrowDims &dims);
    void grow_levels_planned(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::StepTables &t, detail::LevelWork &w, detail::TreeBuilder &tb);
    void grow_levels_host(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::StepTables &t, detail::LevelWork &w, detail::TreeBuilder &tb,
                          detail::Stager &sta, detail::Stager &stb);
    detail::Level stage_level(const detail::GrowCtx &c, const detail::GrowDims &dims, detail::LevelWork &w, detail::TreeBuilder &tb, detail::Stager &sta, int depth,
                              std::vector<int> active);
    void level_histograms(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::LevelWork &w, const detail::Level &L);
    uint32_t score_select_level(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::StepTables &t, const detail::LevelWork &w, const detail::Level &L);
    void replay_near_ties(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::StepTables &t, const detail::LevelWork &w,
                          const std::vector<detail::HNode> &nodes, const detail::Level &L);
    void finish_leaves(const detail::GrowCtx &c, const detail::GrowDims &dims, const detail::LevelWork &w, detail::TreeBuilder &tb, detail::Stager &sta,
                       std::vector<int64_t> &acc, double &leaf_scale);
    uint32_t next_seq() { const uint32_t seq = ++level_seq_; return seq ? seq : ++level_seq_; }   // 0 is never published
    // ---- a step's categorical candidates (engine_cat_candidates.hip): the scan is enqueued before the numeric preparation and collected behind it ----
    bool enqueue_categorical_scan(const char *dcells, int N, int Fc, int B);   // false: declined at its sizes, nothing enqueued
    bool collect_categorical_candidates(const char *dcells, int N, int Fc, int B, const float *dgrads, int D, std::vector<detail::CatCandidate> &cat_cands,
                                        std::vector<int> &cat_classes);   // false: declined, the host rules decide; dgrads: raw gradients (device), for the ranking
    bool cat_rank_round(const char *dcells, int N, int Fc, const float *dgrads, int D, int n_distinct, detail::CatList &list);
    void cat_gather_sharded(detail::CatList &list, std::vector<int> &order, int &n_distinct, std::vector<char> &store);
    void sharded_categorical_ranking(const char *hcat, const float *hgrads, int N, int Fc, int D, int B, std::vector<detail::CatCandidate> &cat_cands,
                                     std::vector<uint16_t> &h_catcodes, std::vector<int> &cat_classes);
    void verify_pending_categories();   // the byte comparisons the replay deferred; a difference sets cat_clash_
    // ---- a step's numeric thresholds (engine_candidates.hip): one function per route ----
    void numeric_thresholds(const float *dobs, int N, int F, int B, long long n_global, const uint32_t *d_kt, float *d_thr, uint32_t *d_thrkeys,
                            DevBuf &root_le_buf, const uint32_t **root_le_out, int pass1_chunks = 0, uint16_t *d_codes_out = nullptr, bool *codes_written = nullptr);
    bool radix_select_applies(int B, long long n_global) const;
    detail::ThrRoute threshold_route(int N, int B, long long n_global) const;   // the route choice, written once
    void thresholds_fixed(const detail::ThrArgs &a), thresholds_uniform(const detail::ThrArgs &a), thresholds_bisection(const detail::ThrArgs &a), thresholds_sample(const detail::ThrArgs &a);
    bool thresholds_lds_sort(const detail::ThrArgs &a, uint16_t *d_codes_out);   // true: it wrote the class codes too
    const uint32_t *thresholds_radix(const detail::ThrArgs &a, DevBuf &root_le_buf, int pass1_chunks);   // returns #{keys <= threshold} (one GPU), else null
    // ---- step() in stages (engine_step.hip) ----
    bool step_pass(detail::StepInputs &in, bool host_categorical);   // one attempt at the step; false: a categorical hash clash, nothing booked
    void stage_step_inputs(detail::StepInputs &in);
    detail::CatStage categorical_stage(const detail::StepInputs &in, bool host_categorical);
    void finish_candidates_only(const detail::CatStage &cs, int Fc, const float *d_thr, size_t n_thr);
    void launch_cat_codes(const detail::StepInputs &in, const detail::CatStage &cs, uint16_t *d_codes);
    // ---- the stages step() and step_prepared() share (engine_step.hip) ----
    void read_step_hooks();                                              // the per-call test hooks that choose the selection path
    bool fused_prep_applies(int N, int F, long long n_global) const;     // kern::small_prep is tried for this shape
    void check_prepared_model(const char *what) const;                   // numeric-only, one GPU, step()'s limits: raised before the device is touched
    void check_prepared_dataset(const char *what, const PreparedDataset *ds) const;   // the data set is there and is this model's: device, n_bins, generator, width
    // step_prepared behind its argument checks and input staging: statistics, growth, append on device gradients and (nullable) device rows
    void step_prepared_run(const PreparedDataset *ds, const float *dgrads, const int32_t *d_rows, int m, const int32_t *cols = nullptr, int n_cols = 0);
    void begin_step_profile();   // a step's phase list starts here
    // ---- conditions as bin indices of ONE threshold table (engine_codes.hip): host tables appended split row by split row, their device
    // copies appended behind sync_model_to_device().  Keyed on the data set's thresholds_id: data sets that share thresholds share the tables
    // (a fit that alternates between a training and a validation set appends the new trees' rows only).  Dropped when a data set with other
    // thresholds is named or the ensemble has shrunk.
    void sync_code_bins(const PreparedDataset &ds);                      // host only: code_bins_host_ covers every split row of the model
    void check_code_range(const PreparedDataset &ds, const char *what, int start_tree, int stop_tree);   // Unsupported: an inexpressible condition the walk of the range reads
    kern::CodeTables sync_code_tables(const PreparedDataset &ds);        // device: needs sync_model_to_device()
    // numeric preparation of a batch into `pb` (phases transpose / candidates / binning); fs: the gradient statistics that step() lets the
    // fused preparation kernel compute in its launch (nullptr: want_stats = false)
    NumericPrep prepare_numeric(PrepBuffers &pb, const float *dobs, int N, int F, int Fc, long long n_global, bool prep_candidate, detail::FusedStats *fs);
    void run_grad_stats(detail::FusedStats &g, int N, long long &n_global);   // A2: statistics + quantisation (kern::small_stats when it applies)
    void grow_step_tree(const detail::StepData &d, std::vector<detail::HNode> &nodes, std::vector<int> &frontier, std::vector<int64_t> &acc, double &leaf_scale);
    int64_t *quantile_cum_device(const std::vector<int64_t> &cum, long long n_global, int B);   // device copy of the quantile target ranks (cached)
    void phase_begin(bool key = false);
    void phase_end(const char *name, bool key = false);
    void phases_resolve();
    std::pair<hipEvent_t, hipEvent_t> kernel_events(const char *name, bool key);   // event pair for one dispatch's own timestamps

    int device_ordinal_ = -1;
    bool device_ready_ = false;
    hipStream_t stream_ = nullptr;        // the stream everything is enqueued on: own_stream_ or the caller's (set_stream)
    hipStream_t own_stream_ = nullptr;
    gbrl_hip_collective coll_{};
    bool has_coll_ = false;
    Parity parity_;
    void refuse_sharding_in_reference_mode() const;
    void *rccl_comm_ = nullptr;          // non-null: the exchanges below are RCCL calls on stream_
    enum class Red { SumI64, SumF64, MaxF32, MinF32 };
    void exchange(Red op, void *dev_buf, size_t count);   // all-reduce in place; stream-ordered (RCCL) or host-synchronous (hooks)
    void allreduce_host(Red op, void *host, size_t count, DevBuf &scratch);   // the same on a host array: up, exchange, down, synchronise
    bool all_ranks_agree(bool mine, DevBuf &scratch);      // true on every rank when `mine` is true on any: every rank takes the same path
    // every rank's records (int64 words), rank after rank; more than `cap` records in all: Unsupported
    std::vector<int64_t> all_gather_records(const std::vector<int64_t> &mine, int words_per_record, size_t cap);
    // recv[0 .. count) = sum over ranks of their send[rank * count .. (rank + 1) * count)  (int64).  RCCL: ncclReduceScatter on the
    // stream (half the bytes of an all-reduce over the xGMI ring); hooks: all-reduce of the whole send buffer, then the own slice.
    void reduce_scatter_i64(int64_t *send, int64_t *recv, size_t count);
    size_t exch_bytes_ = 0, exch_calls_ = 0;   // bytes this rank hands to the transport per step() (diagnostic, reported as phases)
    static int radix_exchange_trampoline(void *self, int64_t *dev_buf, size_t count);

    // measurement
    int profiling_ = 0;
    unsigned key_calls_ = 0;   // key-kernel launches seen at profiling level 1 (every seventh carries an event pair)
    bool force_bisection_ = false, force_sample_select_ = false, force_host_categorical_ = false, force_radix_ = false, last_quantile_fallback_ = false;
    bool cat_clashed_ = false;   // a step of this model met a categorical hash clash: it stays on the host scan, whatever the hook says
    // fit(): numeric thresholds computed once from the whole data set and reused by every batch's step()
    std::vector<float> fixed_thr_;
    std::vector<detail::CatCandidate> fixed_cat_cands_;
    std::vector<int> fixed_cat_classes_;
    bool fixed_cat_valid_ = false;
    bool candidates_only_ = false;
    bool in_fit_ = false;   // predict() called from fit(): keep one accumulation chain per row in tree order (no tree-range split)
    std::vector<std::pair<std::string, float>> phases_;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool_;
    hipEvent_t ev_level_ = nullptr;   // marks the per-level result read-back (GBRL_HIP_EVENT_RESULTS=1: the copy-engine path)
    // Per-step constants of numeric-only steps (feature slots, candidate weights / reference order / slot lookup): they depend on
    // (F, n_bins, growth policy, feature weights, feature mapping) only, so they are built and uploaded once and reused while those
    // stay the same and the device staging block is still the one they were uploaded to.
    struct StepConstCache {
        bool valid = false;
        int F = 0, B = 0, oblivious = 0;
        std::vector<float> fw;
        std::vector<int32_t> rev;
        std::vector<kern::FeatureSlot> slots;
        std::vector<int32_t> cand_ref, cand_slot;
        std::vector<float> cand_w;
        std::vector<int> ref_to_internal;
        const void *dev_base = nullptr;   // device staging block that holds the uploaded copy (nullptr: not uploaded yet)
        size_t stage_bytes = 0;
    } step_const_;
    DevBuf d_rows_iota_;              // 0, 1, 2, ...: the root's row list, generated when it grows and read-only afterwards
    const void *iota_ptr_ = nullptr;
    int iota_n_ = 0;
    DevBuf d_pub_done_;               // block counter of k_resolve_splits' in-kernel publication (zero between launches)
    const void *pub_done_ptr_ = nullptr;
    const void *leafacc_clean_ptr_ = nullptr;   // leaf accumulators known to be zero (handed back clean by the last publication)
    size_t leafacc_clean_bytes_ = 0;
    PrepBuffers prep_ws_;             // step()'s numeric preparation; step_prepared(rows) gathers the subset's codes into prep_ws_.codes
    DevBuf d_sub_rows_, d_rows_mm_;   // step_prepared(rows): device copy of a host index vector, min / max of a device one
    DevBuf d_cols_plan_;              // step_prepared(cols): the gather plan (kern::gather_cols_plan); the subset's thresholds and keys go to prep_ws_
    std::vector<int32_t> cols_plan_host_, fit_cols_;   // its host copy (alive until the step has waited for the stream); fit_prepared's column draw
    uint64_t code_ds_id_ = 0;         // the thresholds id the code tables below are for (0: none)
    size_t code_splits_ = 0, code_up_splits_ = 0, code_nodes_ = 0, code_up_nodes_ = 0;   // split rows / greedy node records converted on the host, and on the device
    std::vector<int32_t> code_bins_host_, code_pack_host_, code_nodes_host_;   // bins [S][MD] (-1 unused or categorical, -2 inexpressible), cond_pack and grd_nodes with the bin as their second word
    DevBuf m_code_bins_, m_code_pack_, m_code_nodes_;
    DevBuf d_fp_pred_, d_fp_grads_, d_fp_iota_, d_fp_targets_;   // fit_prepared: held prediction [n][D], batch gradients, 0..n-1, staged targets
    DevBuf d_fp_vpred_, d_fp_vtargets_, d_fp_vpart_, d_fp_vsums_;   // its validation rows: held prediction [n_v][D], staged targets, loss partials, one sum per iteration
    DevBuf d_fp_gscratch_, d_fp_sfactor_, d_fp_eff_;   // its one-side draws: the selection's scratch (kern::goss_scratch), the kept rows' factors, the effective weights by absolute row
    DevBuf d_fp_srows_, d_fp_sgrads_, d_fp_sscratch_;   // its sampled iterations: the kept rows of the batch, their gradient rows, block counts + m
    DevBuf d_obj_weights_, d_fp_weights_, d_fp_vweights_, d_wstat_, d_wpart_, d_wsum_;   // row weights: staged vectors; kern::weight_stats' two ints, partials and sum
    DevBuf d_obj_pred_, d_obj_targets_, d_obj_grad_, d_obj_part_, d_obj_sum_, d_obj_counts_;   // objective_gradient: staged inputs, the gradient, loss partials and sum; class counts + first bad row
    DevBuf d_pi_targets_, d_pi_variants_, d_pi_part_, d_pi_sums_;   // permutation_importance_prepared: staged targets, the variant list, one launch's loss partials, one sum per variant
    DevBuf d_pd_variants_, d_pd_slots_, d_pd_part_, d_pd_sums_, d_pd_ice_;   // partial_dependence_prepared: the launched variants and their ICE slots, one launch's partials, D sums per variant, ICE rows bound for the host (released when the call ends)
    DevBuf d_met_counts_, d_met_scratch_, d_fp_vmetric_;   // eval_metric: the integer counters, the AUC pipeline's scratch; fit_prepared: the metric's counters per iteration
    struct Held;     // engine_fit_prepared.hip: a data set's rows carried through the model's trees, batch by batch
    struct FitRun;   // engine_fit_prepared.hip: the state of one fit_prepared call and the stages that work on it
    // ---- what the calls on a data set share (engine_codes.hip)
    void reset_events() { ev_used_ = 0; ev_names_.clear(); phases_.clear(); }   // a public call starts with an empty event pool and phase list
    template <typename T>
    const T *staged(DevBuf &buf, const T *x, bool on_dev, size_t count, const char *what) {   // an array that may already be on the device
        return on_dev ? x : upload(buf, x, count, what);
    }
    template <typename T>
    T *zeroed(DevBuf &buf, size_t count, const char *what) {   // count words of a grow-only device buffer, zeroed on the stream
        T *d = static_cast<T *>(buf.ensure(sizeof(T) * count));
        hip_check(hipMemsetAsync(d, 0, sizeof(T) * count, stream_), what);
        return d;
    }
    // a few words back from the device, and the wait for them; phase: a phase that ends behind the copy and before the wait
    void read_back(void *host, const void *dev, size_t bytes, const char *what, const char *phase = nullptr);
    // the rows of a data set a call works on (null: all of them), on the device and known to lie in [0, ds->n) (checked_rows)
    const int32_t *subset_rows(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m);
    int resolve_tree(const char *what, int tree) const;   // a leaves call's tree (-1: the last), refused when the model has none or not that one
    // the phase that has just ended joins the list the caller's phases are in (a step's list has been resolved already), with a marker that is not a time
    void join_tail_phase(const char *name, const char *marker, bool value);
    // class counts of device labels [n] (counts, when given: [D]); a label outside [0, D) is InvalidArgument naming the first such row
    void check_labels(const char *what, const int32_t *d_labels, int n, int D, std::vector<int32_t> *counts);
    // rows [start, start + bn) of a held prediction (one batch of it, or a part of one) advanced to every tree the model has, with the gradient
    // tail (targets, grad_out) and / or the loss tail (loss_targets, loss_part) of kern::predict_continue_codes; targets are [n][D] (softmax:
    // one int32 label per row behind the float pointers)
    // weights (nullable): device [n], one per row of the held data set, for whichever tail is on
    void advance_held(Held &h, int start, int bn, const float *targets, float *grad_out, const float *loss_targets, double *loss_part, bool generic,
                      int objective, const float *weights = nullptr, const float *d_alpha = nullptr /*device [D]: kObjQuantile's levels*/);
    // the partials of a loss tail summed into *d_sum (kern::staged_loss_finish) and, with host_sum, its 8 bytes on their way to the host: they
    // are there after the caller's wait for the stream
    void finish_loss_sum(const double *d_part, int n_part, double *d_sum, double *host_sum);
    // newton_leaves_prepared behind its argument checks and input staging (fit_prepared's loop body too): device pred / targets, indexed by the
    // position or (abs_index) by the data set row; the phase newton_leaves joins the caller's phase list
    void newton_leaves_run(const char *what, const PreparedDataset *ds, const kern::CodeRows &cr, int m, const float *d_pred, const void *d_targets, bool abs_index,
                           int objective, int t, double leaf_l2, bool generic, int64_t *sums_out, int *bits_out, float *values_out,
                           const float *d_weights = nullptr, float weight_max = 0.0f);   // (weights indexed like d_pred)
    // quantile_leaves_prepared likewise: d_alpha is the device table of the levels; the phase quantile_leaves joins the caller's phase list
    void quantile_leaves_run(const char *what, const PreparedDataset *ds, const kern::CodeRows &cr, int m, const float *d_pred, const float *d_targets,
                             bool abs_index, const float *d_alpha, int t, bool generic, float *values_out, int64_t *counts_out, int64_t *ranks_out);
    DevBuf d_lq_res_, d_lq_scratch_, d_lq_alpha_;   // its result block (keys, ranks, counts, flag), its workspace, the levels
    std::vector<uint32_t> lq_host_;                 // ... the result block read back
    // rank_gradient: staged scores, labels and offsets; the discount table; per row qid, pos, beats, ideal and DCG terms, gradient and hessian; per
    // query maxDCG, 1 / maxDCG and NDCG; loss partials and sums; the three statistics words
    DevBuf d_rk_pred_, d_rk_labels_, d_rk_off_, d_rk_disc_, d_rk_qid_, d_rk_pos_, d_rk_beats_, d_rk_ideal_, d_rk_term_, d_rk_grad_, d_rk_hess_, d_rk_maxdcg_,
        d_rk_inv_, d_rk_ndcg_, d_rk_part_, d_rk_qpart_, d_rk_sums_, d_rk_stat_;
    // a label vector with its query groups on the device (rank_prepare): 0 rank_gradient's, 1 fit_prepared's training set, 2 its validation set
    struct RankSet { DevBuf off, qid, max_dcg, inv; int n = 0, Q = 0, max_group = 0; long long pairs = 0; };
    RankSet rk_sets_[3];
    DevBuf d_fp_hess_;   // fit_prepared with a ranking objective and newton leaves: the hessian beside d_fp_grads_
    void rank_prepare(const char *what, RankSet &set, const int32_t *d_labels, const int32_t *group, int n_groups, int n, int ndcg_at);
    void rank_eval(const RankSet &set, int objective, int ndcg_at, const float *d_scores, const int32_t *d_labels, int32_t *d_pos, float *dg, float *dh,
                   bool want_loss, double *d_sum, double *host_sum, double *d_ndcg, bool timed = false /* a phase per kernel (set_profiling(2)) */);
    static double rank_loss(const RankSet &set, int objective, double sum);
    DevBuf d_newton_acc_;                         // its int64 sums [leaves][2 D + 1] and the flag word
    std::vector<unsigned long long> newton_host_;   // ... read back
    // Column sums in float64 of device rows [rows][D] and the MultiRMSE built on them, as fit() and fit_prepared() compute the bias and the loss
    // (engine_step.hip).  Its construction enqueues the memset of the zero center.
    struct ColumnStats {
        explicit ColumnStats(Engine &e);
        const std::vector<double> &sums(const float *g, int rows, const float *center);   // column sums (center null) or sums of squares about center; waits for the stream
        // sum_i factor[i] * g[i, d] in the same order (kern::column_sums_weighted); g null: the one-hot matrix of labels
        const std::vector<double> &weighted_sums(const float *g, const int32_t *labels, const float *factor, int rows);
        float rmse(const float *grads_dev, int rows);                                      // MultiRMSE, loss.cpp:42-56: sqrt(0.5 * sum g^2 / rows)
        Engine &e_;
        const int D_;
        float *d_zero_;
        double *d_stat_;
        std::vector<double> hs_;
    };
    DevBuf d_am_s_, d_near_list_, d_near_ent_, d_near_rep_, d_near_nr_, d_near_maps_, d_near_pos_, d_near_nrb_, d_near_vals_, d_near_means_, d_near_sums_, d_near_chains_, d_near_rowsort_, d_near_tiles_;   // near-tie replay (kern::near_tie_replay): runner-up per arg-max block, candidate lists, ordered row lists, replayed scores
    bool small_grow_off_ = false;     // latched after a failed launch / an abandoned grid barrier of the one-launch kernel: this engine keeps to the level loop
    long long small_grow_fallbacks_ = 0;   // trees the level loop grew after such a failure (diagnostics)
    long long near_replays_ = 0, near_bailouts_ = 0, near_in_kernel_ = 0;   // levels replayed / one-launch trees handed over (diagnostics: phases at profiling level 2)
    DevBuf d_sg_bests_, d_sg_sync_, d_sg_near_;   // one-launch growth of RL-sized steps (kern::small_grow): per-level bests of every block, barrier words
    const void *sg_sync_ptr_ = nullptr;
    std::chrono::steady_clock::time_point prof_marks_[4]{};
    std::chrono::steady_clock::time_point prof_step_entry_{};   // measurement (GBRL_HIP_SMALL_GROW_PROF)
    int prep_launches_ = 0;           // diagnostic of the last step(): 1 = kern::small_prep ran, 3 = the separate preparation launches
    uint32_t level_seq_ = 0;          // sequence number of the last published level result block (0 is never published)
    std::vector<const char *> ev_names_;
    size_t ev_used_ = 0;

    DevBuf d_pred_partial_;
    DevBuf d_pred_slots_;     // leaf slots of the two-launch chain path (kern::predict_chain)
    DevBuf d_shap_ops_, d_shap_nodes_, d_shap_values_, d_shap_poly_, d_shap_out_;
    int shap_n_ops_ = 0;
    uint64_t shap_prog_version_ = ~0ull;
    // the codes form (engine_explain.hip): a program, polynomial arrays and result buffers of its own, cached under (model.version, thresholds id)
    DevBuf d_shapc_ops_, d_shapc_nodes_, d_shapc_values_, d_shapc_poly_, d_shapc_out_, d_shapc_scratch_, d_shapc_part_, d_shapc_sums_;   // out: the host-bound matrix (released when the call ends); scratch: one chunk of the importance call (kept); part [tiles][2][F D] (released); sums [2][F D]
    int shapc_n_ops_ = 0;
    uint64_t shapc_prog_version_ = ~0ull, shapc_ds_id_ = 0;
    struct ShapPoly { const float *norm, *base, *offset; };                  // device
    struct ShapPreparedRun { const int32_t *rows; ShapPoly poly; };          // device: the row list (null: every row) and the polynomial arrays
    int upload_shap_program(int t0, int t1, const int32_t *bins /*null: the float form*/, DevBuf &ops, DevBuf &nodes, DevBuf &values);   // returns the op count
    ShapPoly upload_shap_poly(DevBuf &buf, const float *norm, const float *base_poly, const float *offset);
    // what both data-set calls refuse, in order: check_prepared_dataset's list (categorical columns and a row-sharded model among it), output_dim > 128,
    // a missing polynomial array, a model without trees, tree_idx outside it, check_row_count / check_host_rows, a shape without a launch plan, a tree
    // the thresholds cannot express (check_code_range)
    void check_shap_prepared(const char *what, const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int tree_idx, const float *norm,
                             const float *base_poly, const float *offset);
    ShapPreparedRun stage_shap_prepared(const PreparedDataset *ds, const int32_t *rows, bool rows_dev, int m, int tree_idx, const float *norm,
                                        const float *base_poly, const float *offset);
    void launch_shap_codes(const PreparedDataset *ds, const ShapPreparedRun &r, int p0, int count, float *out);
    void finish_shap_prepared(const char *launch, void *host, const void *dev, size_t bytes, const char *what);

    // ---- per-step workspace (grow-only, reused across steps) ----
    DevBuf d_obs_, d_grads_, d_qg_, d_stat_, d_partials_f64_, d_meanden_, d_maxbits_;
    DevBuf d_prefix_, d_trial_, d_counts_, d_cum_, d_minmax_;
    DevBuf d_selcnt_, d_kcls_, d_qflags_, d_splitters_, d_ccounts_, d_c2l_, d_tgt_list_, d_tgt_rank_, d_list_off_, d_qlists_;
    DevBuf d_radix_state_, d_radix_partial_, d_radix_global_, d_scales_;
    DevBuf d_catcodes_, d_rows_[2];
    DevBuf d_hist_prev_, d_am_v_, d_am_i_, d_stage_const_, d_stage_a_, d_stage_b_, d_results_;
    PinnedBuf pin_const_, pin_a_, pin_b_, pin_res_, pin_thr_, pin_acc_;
    DevBuf d_hist_partials_, d_hist_, d_hist_local_, d_hist_recv_, d_gather_, d_scores_, d_parent_;
    DevBuf d_splits_, d_cursors_, d_leafacc_, d_plan_, d_res_all_;
    PinnedBuf pin_res_all_, pin_cum_;
    long long cum_cache_n_ = -1;   // (global rows, n_bins) the device copy of the quantile target ranks was built for
    int cum_cache_b_ = -1;
    // ---- predict workspace + device mirror of the ensemble ----
    DevBuf d_pobs_, d_pcat_, d_pout_;
    DevBuf d_leaves_out_, d_leaf_counts_;   // predict_leaves: indices bound for the host; leaf_counts: the uint32 counters
    DevBuf d_refit_p_, d_refit_leaf_, d_refit_acc_, d_refit_values_, d_refit_gmax_;   // refit_leaves: running prediction, leaf per row, int64 sums, new values, max |g| per tree
    DevBuf d_staged_stops_, d_staged_targets_, d_staged_part_, d_staged_sums_;   // predict_staged / staged_loss: stops table, staged targets, loss partials and sums
    DevBuf m_tree_indices_, m_depths_, m_feature_indices_, m_feature_values_, m_values_, m_is_numerics_, m_ineq_,
        m_cat_ids_, m_bias_, m_opt_start_, m_opt_stop_, m_opt_lr_, m_cond_pack_, m_grd_nodes_, m_grd_off_, m_values_sw_, m_cond_ra_;
    DevBuf m_rate_;   // Linear schedules: rate[t][optimizer] for every tree (detail::RateTable).  Not built while every optimizer is Const.
    // The upload marks.  The mirror only ever appends: a mark says how much of a host array the device holds, sync_model_to_device() (the one
    // place that advances them, after its flush) extends the host arrays from the marks and appends [mark, current size) to the device.
    //   up_trees_          trees:      m_tree_indices_, m_cond_ra_, the greedy node records built (grd_), and with values_redo_tree_ m_values_sw_
    //   up_leaves_         leaves:     m_values_, m_ineq_
    //   up_splits_         split rows: m_depths_, m_feature_*, m_is_numerics_, m_cat_ids_, m_cond_pack_ (and cond_pack_host_ is built from it)
    //   values_redo_tree_  the first tree whose record in m_values_sw_ is stale although up_trees_ covers it (kNoRedo: none)
    //   grd_up_nodes_      greedy node records in m_grd_nodes_
    //   rate_trees_        rows of m_rate_ (0 while no schedule is Linear; detail::RateTable starts over by itself when the optimizers change)
    // Who takes them back:  rewind_values(t) -- the values of tree t alone have changed -- lowers up_leaves_ to the tree's first leaf and
    // values_redo_tree_ to t, nothing else holds a value.  invalidate_mirror() -- values of any tree may have changed -- zeroes every mark but
    // keeps the dictionary (dict_splits_, cat_dict_): ids and tokens stay valid.  A shrunken ensemble (sync_cat_dict: a mark beyond the model)
    // zeroes up_* and grd_up_nodes_ and drops the dictionary too; rate_trees_ beyond the model makes the table start over.  up_trees_ == 0 is
    // what resets grd_ and the host copies of the records.
    size_t up_trees_ = 0, up_leaves_ = 0, up_splits_ = 0;
    static constexpr size_t kNoRedo = ~static_cast<size_t>(0);
    size_t values_redo_tree_ = kNoRedo;
    size_t grd_up_nodes_ = 0;
    size_t rate_trees_ = 0;
    uint64_t mirror_version_ = ~0ull;   // the model version all of it was synchronised for
    uint64_t dict_model_version_ = ~0ull; size_t dict_splits_ = 0;   // sync_cat_dict(): the model version / split rows cat_dict_ covers
    // the host copies the marks count in, built by mirror_records.h
    detail::CatDict cat_dict_;            // the categorical strings that occur in the model's conditions: (cat feature, string) -> id >= 1
    std::vector<int32_t> cat_ids_host_, cond_pack_host_, cond_ra_host_;
    std::vector<float> values_sw_host_;   // second-generation predict: see kern::PredictModel::values_sw
    detail::GreedyNodes grd_;
    detail::RateTable rate_;
    // packed-code predict (kern::predict_pc): the ensemble's code book -- per numeric feature the sorted distinct thresholds, per
    // mentioned category a bit slot, per tree level a (word, shift, T) record -- rebuilt when the model has changed
    bool ensure_pc_book(int n_num, int n_cat);
    DevBuf m_pc_cond_, m_pc_thr_, m_pc_thr_off_, m_pc_cat_slot_, m_pc_word_cols_, d_pc_rows_;
    size_t pc_version_ = static_cast<size_t>(-1);
    int pc_f_ = -1, pc_fc_ = -1, pc_wn_ = 0, pc_nw_ = 0, pc_row_words_ = 0, pc_iters_ = 1;
    bool pc_ok_ = false;
    uint64_t dict_token_ = 0; size_t dict_token_size_ = static_cast<size_t>(-1);   // cat_dict_token(): cached per dictionary size (entries are only appended)
    DevBuf d_pcat_in_;   // pre-encoded ids handed over in host memory
    size_t dict_version_ = static_cast<size_t>(-1);   // cat_dict_.size() the device dictionary was built from
    int dict_fc_ = -1;
    DevBuf d_dict_off_, d_dict_hash_, d_dict_id_, d_dict_words_, d_pcells_;
    PinnedBuf pin_model_stage_;           // the slices sync_model_to_device appends, staged for one kern::stage_copy launch
    hipEvent_t ev_model_stage_ = nullptr; // behind that launch: the block is not refilled before it has been read
    detail::CatScan cat_;             // the device scan for a step's distinct categorical cells, and where its class codes come from
    detail::CatMemory cat_mem_;       // every distinct (feature, cell) met so far; the replay of the reference's candidate container
    bool cat_clash_ = false;          // this step's deferred comparisons found two categories of one feature under one 64-bit hash
    long long cat_clash_redos_ = 0;   // steps grown a second time on the host scan after a 64-bit hash clash (diagnostics)
    DevBuf d_fit_cells_, d_fit_cells2_;
    DevBuf d_fit_obs_, d_fit_targets_, d_fit_obs2_, d_fit_targets2_, d_fit_perm_, d_fit_preds_, d_fit_grads_, d_fit_zero_;
};

}  // namespace gbrl
