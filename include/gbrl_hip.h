/* gbrl_hip.h -- C ABI of the MI355X-native GBRL hot path (libgbrl_hip.so).
 *
 * This is the drop-in boundary for ONE path of NVlabs/gbrl: the per-step tree fit (GBRL::step) and the
 * ensemble prediction (GBRL::predict), plus the model state those two calls read and write (constructor,
 * setters/getters, .gbrl_model save/load).  Plain pointers and sizes only; no torch / pybind types.
 * Every entry point names the reference interface it replaces (paths relative to the reference repo).
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md; this repo's own binding
 * (gbrl_amd/csrc/binding.cpp -> Python module `gbrl_cpp`, class `GBRL`) is written against this header only.
 *
 * Conventions
 *   - every function that can fail returns 0 on success and a negative gbrl_hip_status otherwise; the message
 *     is available (thread-local) through gbrl_hip_last_error().  The reference throws std::runtime_error at
 *     the same places; the binding turns a non-zero status back into that exception.
 *   - `*_on_device` flags say where a caller buffer lives (0 = host memory, 1 = HIP device memory of the
 *     model's device), mirroring dataHolder<T>{ptr, deviceType} (gbrl/src/cpp/types.h:252-270).
 *   - all compute runs on the GPU.  There is NO CPU fallback: step/predict fail with GBRL_HIP_E_NO_DEVICE
 *     when no HIP device is usable.  The `device` string of the reference ("cpu" / "cuda" / "gpu") only
 *     selects where predict() results are delivered by the Python binding.
 *   - a model is not thread-safe (like the reference object, binding.cpp:448); one model <-> one device.
 */
#ifndef GBRL_HIP_H
#define GBRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBRL_HIP_ABI_VERSION 1
#define GBRL_HIP_MAX_CHAR_SIZE 128 /* MAX_CHAR_SIZE, gbrl/src/cpp/types.h:56 */

typedef struct gbrl_hip_model gbrl_hip_model; /* opaque; replaces class GBRL (gbrl/src/cpp/gbrl.h) */

typedef enum {
    GBRL_HIP_OK = 0,
    GBRL_HIP_E_INVALID = -1,   /* bad argument / incompatible dimensions  (std::runtime_error in the reference) */
    GBRL_HIP_E_NO_DEVICE = -2, /* no usable HIP device: the product has no CPU path */
    GBRL_HIP_E_HIP = -3,       /* a HIP runtime call failed */
    GBRL_HIP_E_IO = -4,        /* file open / read / write error */
    GBRL_HIP_E_UNSUPPORTED = -5 /* valid in the reference, outside this build's scope (Adam, control variates, ...) */
} gbrl_hip_status;

/* enum values follow gbrl/src/cpp/types.h:110-181 so that the serialized metadata is byte-compatible */
enum { GBRL_HIP_SCORE_L2 = 0, GBRL_HIP_SCORE_COSINE = 1 };
enum { GBRL_HIP_GEN_UNIFORM = 0, GBRL_HIP_GEN_QUANTILE = 1 };
enum { GBRL_HIP_GROW_GREEDY = 0, GBRL_HIP_GROW_OBLIVIOUS = 1 };
enum { GBRL_HIP_ALGO_SGD = 0, GBRL_HIP_ALGO_ADAM = 1 };
enum { GBRL_HIP_SCHED_CONST = 0, GBRL_HIP_SCHED_LINEAR = 1 };

/* Constructor arguments: GBRL::GBRL(...) gbrl/src/cpp/gbrl.cpp:76-114, Python defaults binding.cpp:423-440 */
typedef struct {
    int32_t input_dim, output_dim, policy_dim, max_depth, min_data_in_leaf, n_bins, par_th;
    float cv_beta;
    int32_t split_score_func; /* GBRL_HIP_SCORE_*  */
    int32_t generator_type;   /* GBRL_HIP_GEN_*    */
    int32_t use_control_variates; /* must be 0: the reference's GPU path force-disables it too (gbrl.cpp:204-207) */
    int32_t batch_size;
    int32_t grow_policy;      /* GBRL_HIP_GROW_*   */
    int32_t verbose;
    int32_t device_ordinal;   /* HIP device to run on (the reference hard-codes 0, cuda_utils.cu:59); -1 = current */
    const char *learner_name;
} gbrl_hip_config;

/* ensembleMetaData, gbrl/src/cpp/types.h:218-242 -- exactly 80 bytes, written raw into .gbrl_model files */
typedef struct {
    int32_t n_leaves, n_trees, max_trees, max_leaves, max_trees_batch, max_leaves_batch;
    int32_t input_dim, output_dim, policy_dim, max_depth, min_data_in_leaf, n_bins, par_th;
    float cv_beta;
    int32_t verbose, batch_size;
    uint8_t use_cv, split_score_func, generator_type, grow_policy;
    int32_t n_num_features, n_cat_features, iteration;
} gbrl_hip_metadata;

/* optimizerConfig, gbrl/src/cpp/types.h:186-197.  algo must be SGD.  scheduler Const: every tree's values enter predictions scaled by
 * init_lr.  Linear (scheduler.h:124-134): tree t (absolute index) is scaled by max(stop_lr, init_lr + ((t + 1) / T) * (stop_lr - init_lr)),
 * evaluated in float32; T must be positive. */
typedef struct {
    int32_t algo, scheduler;
    float init_lr, stop_lr;
    int32_t start_idx, stop_idx, T;
    float beta_1, beta_2, eps;
} gbrl_hip_optimizer;

/* ---- library / device --------------------------------------------------------------------------------- */
int gbrl_hip_abi_version(void);
/* number of usable HIP devices (0 when none); replaces GBRL::cuda_available (gbrl.cpp:542-548) */
int gbrl_hip_device_count(void);
const char *gbrl_hip_last_error(void);
/* device buffers handed to callers (predict results) -- replaces cudaMalloc/cudaFree in binding.cpp:208-219.
 * Freed buffers are recycled (a few buffers, <= 1 GiB); a recycled buffer is handed out only after a device
 * synchronisation, so a consumer kernel of its previous life cannot still be reading it. */
void *gbrl_hip_device_alloc(size_t bytes);              /* on the calling thread's current device */
void *gbrl_hip_device_alloc_on(int device, size_t bytes); /* on `device` (the buffer pool is keyed by device) */
void gbrl_hip_device_free(void *ptr);

/* ---- lifetime ----------------------------------------------------------------------------------------- */
gbrl_hip_model *gbrl_hip_create(const gbrl_hip_config *cfg);            /* GBRL::GBRL          gbrl.cpp:76-114   */
gbrl_hip_model *gbrl_hip_clone(const gbrl_hip_model *other);            /* GBRL::GBRL(GBRL&)   gbrl.cpp:125-148  */
gbrl_hip_model *gbrl_hip_load(const char *filename);                    /* GBRL::loadFromFile  gbrl.cpp:1175-1250 */
int gbrl_hip_save(gbrl_hip_model *m, const char *filename);             /* GBRL::saveToFile    gbrl.cpp:1130-1173 */
void gbrl_hip_destroy(gbrl_hip_model *m);                               /* GBRL::~GBRL         gbrl.cpp:150-165  */

/* ---- state the hot path reads ------------------------------------------------------------------------- */
int gbrl_hip_set_bias(gbrl_hip_model *m, const float *bias, int n, int on_device);               /* gbrl.cpp:213-240 */
int gbrl_hip_set_feature_weights(gbrl_hip_model *m, const float *w, int n, int on_device);       /* gbrl.cpp:242-269 */
int gbrl_hip_set_feature_mapping(gbrl_hip_model *m, const int32_t *feature_mapping,
                                 const uint8_t *mapping_numerics, int n);                        /* gbrl.cpp:271-316 */
int gbrl_hip_set_optimizer(gbrl_hip_model *m, const gbrl_hip_optimizer *opt);                    /* gbrl.cpp:452-525 */
int gbrl_hip_get_metadata(const gbrl_hip_model *m, gbrl_hip_metadata *out);                      /* binding.cpp:309-328 */
int gbrl_hip_get_bias(const gbrl_hip_model *m, float *out);                                      /* gbrl.cpp:318-330 */
int gbrl_hip_get_feature_weights(const gbrl_hip_model *m, float *out);                           /* gbrl.cpp:332-344 */
int gbrl_hip_get_feature_mapping(const gbrl_hip_model *m, int32_t *feature_mapping, uint8_t *mapping_numerics);
int gbrl_hip_num_optimizers(const gbrl_hip_model *m);
int gbrl_hip_get_optimizer(const gbrl_hip_model *m, int idx, gbrl_hip_optimizer *out);           /* binding.cpp:393-419 */
/* GBRL::get_scheduler_lrs (gbrl.cpp:527-539): out[i] = the rate optimizer i's schedule gives the NEXT tree, get_lr(n_trees) */
int gbrl_hip_get_scheduler_lrs(const gbrl_hip_model *m, float *out /*[num_optimizers]*/);
const char *gbrl_hip_learner_name(const gbrl_hip_model *m);
/* GBRL::get_ensemble_data (gbrl.cpp:1344-1356): copies of the ensembleData arrays (types.h:279-304).  Sizes:
 * T=n_trees, L=n_leaves, S = T (oblivious) or L (greedy), md=max_depth, D=output_dim, in=input_dim.  Any
 * pointer may be NULL. */
int gbrl_hip_get_ensemble(const gbrl_hip_model *m,
                          int32_t *tree_indices /*[T]*/, int32_t *depths /*[S]*/, float *values /*[L*D]*/,
                          int32_t *feature_indices /*[S*md]*/, float *feature_values /*[S*md]*/,
                          float *edge_weights /*[L*md]*/, uint8_t *is_numerics /*[S*md]*/,
                          uint8_t *inequality_directions /*[L*md]*/, char *categorical_values /*[S*md*128]*/,
                          int32_t *reverse_num_feature_mapping /*[in]*/, int32_t *reverse_cat_feature_mapping /*[in]*/);

/* ---- parity mode (new; the reference IS the reference) --------------------------------------------------------------- */
/* The contract is "tree structure bit-identical to the CPU reference".  Where the exact (float64) arg-max of a node has a runner-up inside
 * the reference's float32 summation noise, the reference's own rounding decides which candidate wins; the near-tie replay (csrc/neartie.hip)
 * re-scores such candidates in the reference's float32 operation sequence and takes its choice.  The replay costs time on large batches
 * (DESIGN.md section 3a), so WHERE it runs is a setting of the model:
 *   GBRL_HIP_PARITY_DEFAULT       replay for batches of up to 65 536 rows on one GPU, the exact arg-max above.
 *   GBRL_HIP_PARITY_REFERENCE     replay at every batch size.  max_node_rows > 0: in batches above 65 536 rows only nodes of up to that many
 *                                 rows are replayed (an oblivious level: when all of its nodes are that small), larger nodes keep the exact
 *                                 arg-max; 0: every node.  Batches of up to 65 536 rows replay every flagged node whatever the limit.
 *   GBRL_HIP_PARITY_EXACT_ARGMAX  never replay: the exact arg-max decides everywhere.
 * max_node_rows is stored with every mode and read in REFERENCE only; negative values and unknown modes fail with GBRL_HIP_E_INVALID.
 * The setting holds for step() and fit(), on every growth path.  A new model is DEFAULT.  gbrl_hip_clone carries the setting.
 * gbrl_hip_save / gbrl_hip_load do NOT: the .gbrl_model format is the reference's and stays byte-compatible, so a loaded model is DEFAULT
 * (max_node_rows 0) and the caller sets the mode again.
 * Row-sharded models cannot replay (a node's rows are spread over the ranks), they hold the exact arg-max: REFERENCE on a model with
 * collective hooks or an RCCL communicator fails with GBRL_HIP_E_UNSUPPORTED, and so do gbrl_hip_set_collective / gbrl_hip_set_rccl* on a
 * model in REFERENCE mode; DEFAULT and EXACT_ARGMAX are accepted there and both mean the exact arg-max.  In REFERENCE mode a step that
 * cannot replay fails with GBRL_HIP_E_UNSUPPORTED instead of growing another tree quietly (GBRL_HIP_DEVICE_LEVELS=1 on oblivious trees,
 * GBRL_HIP_EVENT_RESULTS=1, output_dim > 1024); the model is left unchanged.
 * Environment hooks override the setting, exactly as they behaved before it existed: GBRL_HIP_NO_NEARTIE_REPLAY=1
 * turns the replay off in every mode; GBRL_HIP_NEARTIE_MAX_ROWS=<n> turns it on for batches above 65 536 rows with limit n in every mode
 * (GBRL_HIP_NO_NEARTIE_REPLAY wins over it).  The getter reports the model's setting, not what a hook makes of it. */
typedef enum {
    GBRL_HIP_PARITY_DEFAULT = 0,
    GBRL_HIP_PARITY_REFERENCE = 1,
    GBRL_HIP_PARITY_EXACT_ARGMAX = 2
} gbrl_hip_parity_mode;
int gbrl_hip_set_parity_mode(gbrl_hip_model *m, int mode /* gbrl_hip_parity_mode */, int max_node_rows);
int gbrl_hip_get_parity_mode(const gbrl_hip_model *m, int *mode, int *max_node_rows);   /* either pointer may be NULL */

/* ---- THE HOT PATH ------------------------------------------------------------------------------------- */
/* GBRL::step (gbrl.cpp:939-981) == Fitter::step_cpu semantics (fitter.cpp:50-115), computed on the GPU:
 * fits ONE tree to `grads` and appends it to the ensemble.
 *   obs      float32 [n_samples, n_num_features] row-major, or NULL when n_num_features == 0
 *   cat_obs  char    [n_samples, n_cat_features, 128] (NUL-padded strings), or NULL
 *   grads    float32 [n_samples, output_dim] row-major
 * Buffers are borrowed for the duration of the call only. */
int gbrl_hip_step(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs,
                  int cat_on_device, const float *grads, int grads_on_device, int n_samples,
                  int n_num_features, int n_cat_features);

/* GBRL::fit (gbrl.cpp:983-1104) == Fitter::fit_cpu semantics (fitter.cpp:117-261), MultiRMSE loss (loss.cpp:42-56), computed
 * on the GPU: bias = column means of `targets`; split candidates from the WHOLE data set once; then `iterations` boosting
 * rounds over consecutive batches of metadata.batch_size rows (predict over trees [0, i) -> gradients pred - target -> one
 * tree); *loss_out = sqrt(0.5 * sum (pred - target)^2 / n_samples) over the whole data set afterwards.  shuffle != 0 fits
 * a randomly permuted copy (seeded from std::random_device like the reference).  */
int gbrl_hip_fit(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                 const float *targets, int targets_on_device, int n_samples, int n_num_features, int n_cat_features,
                 int iterations, int shuffle, float *loss_out);

/* GBRL::predict (gbrl.cpp:369-422) == Predictor::predict_cpu semantics (predictor.cpp:122-265) + SGDOptimizer::step
 * (optimizer.cpp:110-118): out[i,:] = bias - sum_t lr_k * leaf_value(i, t) over trees [start_tree, stop_tree)
 * (stop_tree == 0 means n_trees).  `out` is float32 [n_samples, output_dim], host or device per out_on_device. */
int gbrl_hip_predict(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs,
                     int cat_on_device, int n_samples, int n_num_features, int n_cat_features,
                     int start_tree, int stop_tree, float *out, int out_on_device);

/* Extension (no counterpart in the reference, which re-compares the 128-byte cells of every row inside every predict call,
 * predictor.cpp:231-265 / 188-229): a serving loop that predicts the SAME categorical batch repeatedly, or produces its categorical columns
 * from a small vocabulary, encodes them once.  gbrl_hip_encode_categorical writes int32 ids[n_samples, n_cat_features] (0 = a category no
 * condition of the model mentions) and a token identifying the model's category dictionary; gbrl_hip_predict_encoded is gbrl_hip_predict
 * with those ids in place of the cells and fails with GBRL_HIP_E_INVALID when the token is not the model's current one (a later tree
 * mentioned a new category, or the ids belong to another model): encode again.  Same results as gbrl_hip_predict, bit for bit. */
int gbrl_hip_encode_categorical(gbrl_hip_model *m, const char *cat_obs, int cat_on_device, int n_samples, int n_cat_features,
                                int32_t *ids_out, int ids_on_device, uint64_t *dictionary_token);
int gbrl_hip_predict_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                             uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features,
                             int start_tree, int stop_tree, float *out, int out_on_device);

/* Extension (no counterpart in the reference, whose predict can only start from the bias): a training loop that keeps a batch resident and
 * adds one tree per step holds the ensemble's output on that batch and applies only the trees grown since, instead of walking the whole
 * ensemble again.  `base` is float32 [n_samples, output_dim], the caller's prediction over the trees [0, start_tree) -- for start_tree == 0
 * the tiled bias.  out[r][j] is base[r][j] carried through the trees t = start_tree .. stop_tree - 1 in order: for every optimizer o with
 * start_idx <= j < stop_idx, p = fma(-lr_o(t), leaf_value(r, t)[j], p), lr_o(t) the optimizer's scheduled rate at the ABSOLUTE tree index
 * (Const and Linear).  An output that no optimizer owns keeps its base value, and the bias is never added: it is already in `base`.  The
 * call never splits the range over partial sums, at any batch size or range length, so continuing gbrl_hip_predict's tree-order chain over
 * [0, start_tree) gives the chain over [0, stop_tree) bit for bit.  stop_tree == 0 means n_trees; start_tree == stop_tree returns `base`
 * unchanged; start_tree < 0, start_tree > stop_tree (after resolving 0) or stop_tree > n_trees fail with GBRL_HIP_E_INVALID (a silent no-op
 * in a cache would be a stale prediction); output_dim > 128 is refused as in gbrl_hip_predict.  `out` may be `base` (in place: the expected
 * use).  gbrl_hip_predict_continue_encoded takes the ids and token of gbrl_hip_encode_categorical in place of the cells; a stale token fails
 * as in gbrl_hip_predict_encoded. */
int gbrl_hip_predict_continue(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                              int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree,
                              const float *base, int base_on_device, float *out, int out_on_device);
int gbrl_hip_predict_continue_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                                      uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features,
                                      int start_tree, int stop_tree, const float *base, int base_on_device, float *out, int out_on_device);

/* Extension (no counterpart in the reference): every prefix of the ensemble in ONE walk -- the prediction, or the MultiRMSE loss on a held-out
 * set, after every k trees; the curve that answers "how many trees to keep".  `stops` is a HOST array of n_stops > 0 tree counts k, strictly
 * ascending, 0 <= k <= n_trees.  k == 0 is a legal stage and means the bias alone: unlike stop_tree of gbrl_hip_predict, 0 NEVER means "all
 * trees" here.  Stage s is, bit for bit, what gbrl_hip_predict_continue(base = tiled bias, start_tree = 0, stop_tree = stops[s]) returns: one
 * chain per (row, output) in tree order, rates at the absolute tree index (Const and Linear), an output that no optimizer owns keeps the bias
 * bits, and the walk is never split over tree ranges, at any batch size.  The rows are read once, whatever n_stops is.
 *   gbrl_hip_predict_staged: `out` is float32 [n_stops, n_samples, output_dim], host or device per out_on_device.
 *   gbrl_hip_staged_loss:    `targets` is float32 [n_samples, output_dim], host or device; loss_out is a HOST array of n_stops doubles,
 *                            loss_out[s] = sqrt(0.5 * S / n_samples) in float64, S = the float64 sum of (double)g * (double)g over all rows and
 *                            outputs, g = fl32(prediction - target) -- MultiRMSE as gbrl_hip_fit defines it.  The sum has a fixed reduction
 *                            order and uses no floating-point atomics: two identical calls return identical bytes.
 * Reported with GBRL_HIP_E_INVALID before the device is touched: n_stops <= 0 or stops NULL; a stop that is negative, above n_trees or not above
 * its predecessor; targets / loss_out NULL; the data set errors of gbrl_hip_predict.  output_dim > 128 is refused as in gbrl_hip_predict.
 * Row-sharded models need no exchange: each rank evaluates its own rows. */
int gbrl_hip_predict_staged(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                            int n_samples, int n_num_features, int n_cat_features, const int32_t *stops, int n_stops,
                            float *out, int out_on_device);
int gbrl_hip_staged_loss(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                         const float *targets, int targets_on_device, int n_samples, int n_num_features, int n_cat_features,
                         const int32_t *stops, int n_stops, double *loss_out);

/* Extension (sklearn's apply, XGBoost's and LightGBM's pred_leaf, CatBoost's calc_leaf_indexes): WHERE a row lands.  For a row and a tree t of
 * [start_tree, stop_tree) the answer is the GLOBAL leaf index: the row of `values` in the ensemble data; minus tree_indices[t] it is the index
 * within the tree.
 *   oblivious trees: tree_indices[t] + sum over d of pass(condition d of tree t) << (depth of t - 1 - d); a numeric condition passes when
 *                    x[feature] > threshold, a categorical one when the cell equals its category; a tree of depth 0 gives tree_indices[t].
 *   greedy trees:    the first leaf in storage order from tree_indices[t] on whose conditions all hold, each tested against its inequality
 *                    direction.  As in the reference's walk, a leaf of depth 0 never passes (the search then runs on into the following trees)
 *                    and a search that runs off the ensemble gives -1; a well-formed tree with at least one split does neither.
 * Range: stop_tree == 0 means n_trees; after that 0 <= start_tree < stop_tree <= n_trees is required.  Reported with GBRL_HIP_E_INVALID before
 * the device is touched: any other range, a model without trees, the data set errors of gbrl_hip_predict, a stale dictionary token.  No leaf
 * value is read, so there is NO output_dim limit.  Row-sharded models need no exchange: each rank answers for its own rows.
 *   gbrl_hip_predict_leaves[_encoded]: `out` is int32 [n_samples, stop_tree - start_tree], row-major, host or device per out_on_device.
 *                    n_samples * (stop_tree - start_tree) >= 2^31 is refused with GBRL_HIP_E_UNSUPPORTED, also before the device is touched:
 *                    slice the tree range.
 *   gbrl_hip_leaf_counts[_encoded]: out_host is a HOST array of n_leaves int64, indexed by global leaf over the WHOLE ensemble: entry l is the
 *                    number of rows of this batch that reach leaf l; leaves of trees outside the range are 0.  Reduced on the device with
 *                    integer atomics only (the index matrix is never materialised): two identical calls return identical bytes.  The counters
 *                    of at most gbrl_hip_leaf_counts_chunk() leaves are held on chip per launch; a longer range is processed in runs of whole
 *                    trees, and the rows are read once per run. */
int gbrl_hip_predict_leaves(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                            int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree,
                            int32_t *out, int out_on_device);
int gbrl_hip_predict_leaves_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                                    uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features,
                                    int start_tree, int stop_tree, int32_t *out, int out_on_device);
int gbrl_hip_leaf_counts(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                         int n_samples, int n_num_features, int n_cat_features, int start_tree, int stop_tree, int64_t *out_host);
int gbrl_hip_leaf_counts_encoded(gbrl_hip_model *m, const float *obs, int obs_on_device, const int32_t *cat_ids, int ids_on_device,
                                 uint64_t dictionary_token, int n_samples, int n_num_features, int n_cat_features,
                                 int start_tree, int stop_tree, int64_t *out_host);
int gbrl_hip_leaf_counts_chunk(void);   /* leaf counters one launch of leaf_counts holds on chip (diagnostic; no device needed) */

/* Extension (LightGBM's Booster.refit, XGBoost's process_type=update with updater=refresh): the leaf VALUES of the trees [start_tree, stop_tree)
 * are fitted again on this batch; the structure stays.  `values` and `tree_indices` below are the arrays of the ensemble data.
 *   P = the float32 prediction gbrl_hip_predict_continue(tiled bias, 0, start_tree) gives on these rows (start_tree == 0: the tiled bias).
 *   For t = start_tree .. stop_tree - 1, in order:
 *     g[r][j] = fl32(P[r][j] - targets[r][j]) for ALL outputs: the MultiRMSE gradient of gbrl_hip_fit.  gmax = max |g|, a NaN carried as +inf.
 *     lbits = the step's rule for its exact leaf sums with n = n_samples of this call: min(60, floor(log2(4.0e18 / (n * gmax))) - 1), 40 when
 *     gmax == 0.  Per global leaf l of tree t, routed exactly as gbrl_hip_predict_leaves defines: S[l][j] = the exact int64 sum of
 *     llrint((double)g * 2^lbits) (nearest even) and cnt[l] = the rows that reach l -- integer atomics only: two calls on equal models return
 *     identical bytes.  mean = ((double)S / 2^lbits) / (double)cnt, the expression a step stores.  New value: (float)mean when decay_rate == 0,
 *     else (float)(decay_rate * (double)old + (1 - decay_rate) * mean) with two rounded float64 products and one rounded float64 sum (no fused
 *     multiply-add).  A leaf with cnt == 0 and any leaf of depth 0 keep their value (an oblivious tree of depth 0 is one such leaf: every row
 *     reaches it, and P is advanced with the kept value).  A row whose greedy search leaves tree t (index -1 or outside [tree_indices[t],
 *     tree_indices[t + 1]): a hand-edited file) joins no sum of that tree and keeps its P.
 *     P[r][j] = fmaf(-lr_o(t), new value[leaf][j], P[r][j]) for every optimizer o that owns j, lr_o(t) the rate at the absolute tree index
 *     (Const and Linear); an output nobody owns keeps P -- the bits of gbrl_hip_predict_continue's chain.
 * Only `values` of the trees in the range change.  The structure, n_trees, iteration, bias, optimizers, the category dictionary and its token
 * stay, and so do the trees outside the range: the trees from stop_tree on were fitted against the OLD prefix and are stale with respect to the
 * new one (refit up to n_trees, or grow them again).  *loss_out (host) = bit for bit what gbrl_hip_staged_loss(obs, cat_obs, targets,
 * stops = {stop_tree}) returns right after.  `targets` is float32 [n_samples, output_dim], host or device.
 * Range: stop_tree == 0 means n_trees; after that 0 <= start_tree < stop_tree <= n_trees is required.  Reported before the device is touched,
 * with GBRL_HIP_E_INVALID: a model without trees, any other range, targets or loss_out NULL, decay_rate outside [0, 1] or NaN, the data set
 * errors of gbrl_hip_predict; with GBRL_HIP_E_UNSUPPORTED: output_dim > 128, and a model with collective hooks or an RCCL communicator (the
 * sums would need an exchange per tree: row-sharded refit is out of scope), and a GREEDY tree of depth 0 among the trees [start_tree - 1,
 * stop_tree): its leaf never passes, so the prediction walks on and applies a leaf of the next tree at this tree's rate -- a value the refit has
 * not computed yet, so the chain above cannot be followed (a stump further in front only touches unchanged trees and is fine).  A run in which
 * some gmax, or max |g| of the final P, is not finite (non-finite targets, an overflowing prediction) fails with GBRL_HIP_E_INVALID.  After ANY failure the model is unchanged.  The whole range is one enqueue and one wait. */
int gbrl_hip_refit_leaves(gbrl_hip_model *m, const float *obs, int obs_on_device, const char *cat_obs, int cat_on_device,
                          const float *targets, int targets_on_device, int n_samples, int n_num_features, int n_cat_features,
                          int start_tree, int stop_tree, double decay_rate, double *loss_out);

/* ---- prepared data sets (new: LightGBM's Dataset, XGBoost's QuantileDMatrix) -------------------------------------------- */
/* A step turns the observation matrix into ordered keys, split thresholds and class codes before it looks at a gradient.  A prepared data set is
 * that work done ONCE for a batch of numeric observations: several epochs over one rollout buffer, an actor and a critic on the same observations,
 * or a supervised loop then step on it with new gradients each time.
 *   gbrl_hip_dataset_create(m, obs, obs_on_device, n, n_num)  runs exactly what gbrl_hip_step runs for numeric columns, on the same code paths
 *     (key transpose; uniform thresholds, the LDS sort, the radix multi-select, the sample-splitter path and its fallbacks; class codes; the
 *     fused preparation of RL-sized batches), into buffers the data set owns, and waits for the stream: `obs` is not needed afterwards.  It
 *     records n, F = n_num, the model's n_bins and generator_type and the device.  The model is not changed.  NULL on failure
 *     (gbrl_hip_last_error, gbrl_hip_dataset_last_status).
 *   gbrl_hip_step_prepared(m, ds, grads, grads_on_device, rows, rows_on_device, n_rows)  gradient statistics, growth, append -- no transpose, no
 *     candidates, no binning.  Legal for ANY model on the data set's device whose n_bins and generator_type equal the data set's and whose
 *     input_dim == F; it only reads the data set, so several models may share one.  It latches n_num_features = F, n_cat_features = 0 at
 *     iteration 0 and honours the model's parity mode, as gbrl_hip_step does.
 *     rows == NULL: n_rows must be n, grads is float32 [n, output_dim], and the model ends up BYTE FOR BYTE as gbrl_hip_step(obs, NULL, grads)
 *     would leave it (ensemble arrays, metadata, the saved file).
 *     rows != NULL: int32 [n_rows], host or device, duplicates allowed (bootstrap), every entry in [0, n); grads is [n_rows, output_dim] in the
 *     order of rows.  The tree is grown on those rows with THE DATA SET'S thresholds -- LightGBM's Dataset.subset, and what gbrl_hip_fit does
 *     with the candidates of the whole data set -- not with the quantiles of the subset.  The growth path is chosen by n_rows as a step on
 *     n_rows rows would choose it.  rows = 0, 1, ..., n - 1 gives the bytes of rows == NULL.  An out-of-range index is found before anything
 *     reads through it (a host vector on the host, a device vector by a min / max kernel, read back): GBRL_HIP_E_INVALID, no tree is grown.
 *   gbrl_hip_dataset_thresholds  out[F * n_bins], host.   gbrl_hip_dataset_codes  out uint16 [G][n_rows][16], host, G = ceil(F / 16): the
 *     group-major class codes (code of feature f and row r at [f / 16][r][f % 16] = #{k : threshold[f][k] < obs[r][f]}); rows == NULL: every
 *     row (n_rows is ignored), else the gathered records of rows.  Diagnostics: they run on the null stream of the data set's device.
 * Refused before the device is touched -- GBRL_HIP_E_UNSUPPORTED: a model with categorical columns (n_cat_features > 0: categorical candidates
 * depend on the step's gradients), a model with collective hooks or an RCCL communicator (the thresholds would need the exchange), a data set
 * from another device, and the limits of gbrl_hip_step (max_depth, n_bins, output_dim) with its messages; GBRL_HIP_E_INVALID: n_bins,
 * generator_type or F differing from the model's, grads NULL or n_rows not n without rows, n_rows <= 0, a NULL or destroyed data set.
 * After ANY failure the model is unchanged.  A data set may outlive the model that made it. */
typedef struct gbrl_hip_dataset gbrl_hip_dataset;
typedef struct {
    int32_t n_rows, n_features, n_bins, generator_type, device, code_groups;
    uint64_t nbytes;   /* device bytes held + the host copy of the thresholds */
} gbrl_hip_dataset_desc;
gbrl_hip_dataset *gbrl_hip_dataset_create(gbrl_hip_model *m, const float *obs, int obs_on_device, int n_samples, int n_num_features);
int gbrl_hip_dataset_last_status(void);   /* status of the calling thread's last gbrl_hip_dataset_create */
void gbrl_hip_dataset_destroy(gbrl_hip_dataset *ds);
int gbrl_hip_dataset_info(const gbrl_hip_dataset *ds, gbrl_hip_dataset_desc *out);
int gbrl_hip_dataset_thresholds(const gbrl_hip_dataset *ds, float *out /*[F*B]*/);
int gbrl_hip_dataset_codes(const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, uint16_t *out /*[G][n_rows][16], host*/);
int gbrl_hip_step_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *grads, int grads_on_device, const int32_t *rows,
                           int rows_on_device, int n_rows);

/* ---- the walk over a data set's bin codes (new): continue and fit without the observations ------------------------------------------ */
/* code(r, f) = #{b : thr[f][b] < obs[r][f]} (-0.0 == +0.0; NaN below every threshold).  For a numeric condition x[f] > v whose v equals some
 * thr[f][b] let bin = #{b : thr[f][b] < v}; then x > v <=> code > bin: if x > v, every threshold below v and v itself are below x
 * (code >= bin + 1); if x <= v, only thresholds below v can be below x (code <= bin).  Duplicated thresholds and any order are fine; NaN has
 * code 0 and never passes, as x > v does.  The rule does NOT hold for a v that is not one of feature f's thresholds: such a model is refused.
 *   gbrl_hip_condition_bins(m, thresholds[F * B], F, B, out)  host only.  out has the length and indexing of feature_values
 *     (gbrl_hip_get_ensemble); a used numeric slot (d < depths[split row]) gets its bin, every other slot -1.  F or B that are not the model's
 *     numeric feature count and n_bins: GBRL_HIP_E_INVALID.  A used numeric condition whose value is not among its feature's thresholds (float
 *     ==; a NaN value never is): GBRL_HIP_E_UNSUPPORTED, the message names the tree and the condition.
 *   gbrl_hip_predict_continue_prepared(m, ds, rows, rows_on_device, n_rows, base, base_on_device, start_tree, stop_tree, out)
 *     out[j] = base[j] carried through the trees [start_tree, stop_tree) for data set row rows[j] (rows == NULL: row j, n_rows must be n) --
 *     BIT FOR BIT gbrl_hip_predict_continue on the observations the data set was made from, which need not exist any more.  base / out
 *     float32 [n_rows, output_dim], `out` where `base` is (host or device); out may be base (updated in place).  Ranges as gbrl_hip_predict_continue (stop 0 =
 *     n_trees, start == stop: out = base), rows as gbrl_hip_step_prepared.  Refused before the device is touched: what gbrl_hip_step_prepared
 *     refuses about the model and the data set, output_dim > 128, a bad range, and (GBRL_HIP_E_UNSUPPORTED) a tree of the range with a
 *     condition the codes cannot express -- for a greedy model also the trees a trailing one-leaf tree of the range lets the walk run into.
 *     The model is never changed.
 *   gbrl_hip_fit_prepared(m, ds, targets, targets_on_device, iterations, loss_out)  gbrl_hip_fit(shuffle = 0) on the data set's rows with
 *     nothing recomputed: the running prediction of every row is held and advanced by the trees grown since its batch was last visited (one
 *     launch, which also writes the MultiRMSE gradient), then gbrl_hip_step_prepared's body grows the tree.  targets float32 [n, output_dim].
 *     Batches are gbrl_hip_fit's: contiguous ranges of batch_size rows in row order, wrapping to row 0; there is no shuffle (permute before
 *     gbrl_hip_dataset_create).  A model without trees gets bias = column means of the targets and ends up BYTE FOR BYTE as gbrl_hip_fit
 *     leaves it, with the same loss.  A model WITH trees keeps its bias and continues from all of them -- unlike gbrl_hip_fit, whose iteration
 *     i predicts from the trees [0, i) only and which resets the bias -- and every existing tree must be expressible on the data set
 *     (GBRL_HIP_E_UNSUPPORTED before anything changes).  Argument errors (the data set checks of gbrl_hip_step_prepared, iterations < 0, NULL
 *     targets, batch_size <= 0) leave the model unchanged; a failure in iteration i leaves the i trees already grown, as gbrl_hip_fit does.
 *
 * Data sets that share thresholds (new: LightGBM's Dataset(reference=train)).  A data set's codes only mean something against its own
 * thresholds, so a held-out batch binned by gbrl_hip_dataset_create gets quantiles of its own and a model grown on the training set is refused
 * on it.  A BOUND data set puts new rows on thresholds that already exist.
 *   gbrl_hip_dataset_create_like(m, reference, obs, obs_on_device, n)  obs float32 [n, F of the reference].  The result holds the codes of obs
 *     under the reference's thresholds -- code(r, f) = #{b : thr[f][b] < obs[r][f]} by the rule above, computed on the ordered keys against the
 *     reference's threshold keys in ONE pass over obs (no transpose, no selection); rows outside the reference's range get 0 or n_bins; records
 *     [G][n][16] u16 with the padding slots zero -- and its own copies of the thresholds, their keys and the host thresholds: the reference may
 *     be destroyed afterwards.  gbrl_hip_dataset_thresholds returns the reference's bytes; nbytes counts the codes and the threshold copies
 *     (a bound data set holds no keys, no feature-major codes and no root table).  It is a full data set: gbrl_hip_dataset_codes,
 *     gbrl_hip_predict_continue_prepared, gbrl_hip_step_prepared and gbrl_hip_fit_prepared work on it; a step on it grows with the
 *     reference's thresholds, byte for byte as a subset step (rows != NULL) on the same records does.  Refused before the device is touched
 *     (GBRL_HIP_E_INVALID): a NULL or destroyed reference, n <= 0, NULL obs; and everything gbrl_hip_step_prepared refuses about (model,
 *     reference).  NULL on failure, status as gbrl_hip_dataset_create.  The model is never changed.
 *   gbrl_hip_dataset_thresholds_id(ds)  a data set made without a reference gets a fresh id; a bound one inherits its reference's, through any
 *     chain.  0 for a NULL or destroyed data set.  The model's code tables (the bins of its conditions) are keyed on this id: calls that
 *     alternate between data sets that share thresholds append the new trees' rows only.
 *
 * Validation and early stopping.
 *   gbrl_hip_fit_prepared_valid(m, ds, targets, .., iterations, valid_ds, valid_targets, .., early_stopping_rounds, min_delta, loss_out,
 *     valid_loss_out, iterations_done, best_n_trees)  gbrl_hip_fit_prepared watching valid_ds, which must share ds's thresholds id (it may be
 *     ds itself).  Let T0 be the tree count at entry (a model without trees: after the bias has been set).  valid_loss_out[k], k = 0 ..
 *     *iterations_done (room for iterations + 1 doubles), is the MultiRMSE of the first T0 + k trees on the validation rows: BIT FOR BIT
 *     gbrl_hip_staged_loss(.., stops = {T0 + k}) on the matrix valid_ds was binned from (sqrt(0.5 * S / n_v) in float64, S from one partial per
 *     64 consecutive rows).  The validation prediction is held on the device and advanced after EVERY iteration, whatever batch_size is, by one
 *     launch that also writes the loss partials.  Rule: best = index of the minimum so far, from k = 0; entry k improves iff valid_loss[k] <
 *     valid_loss[best] - min_delta (a NaN never improves); with early_stopping_rounds = R > 0 the loop ends after iteration k when k - best >=
 *     R; R = 0 records only.  All trees grown stay (there is no truncation); *best_n_trees = T0 + best is the stop_tree to predict with.  The
 *     model after *iterations_done iterations is BYTE FOR BYTE what gbrl_hip_fit_prepared(m, ds, targets, *iterations_done) leaves and
 *     *loss_out is its loss.  Refused before anything changes (GBRL_HIP_E_INVALID): a valid_ds with another thresholds id (create it with
 *     gbrl_hip_dataset_create_like), NULL valid_targets, early_stopping_rounds < 0, min_delta negative or NaN, NULL valid_loss_out; and what
 *     gbrl_hip_fit_prepared refuses.
 *   gbrl_hip_early_stop_scan(curve, n, rounds, min_delta, stop_after, best)  the rule above on a curve of n >= 1 entries, host only (the loop
 *     itself calls it): *stop_after = the first k with k - best >= rounds (rounds > 0), else n - 1; *best = the best index at that point.
 *
 * Row subsampling (new: stochastic gradient boosting -- LightGBM's bagging_fraction, XGBoost's and scikit-learn's subsample).  The sampler is
 * a pure function of (seed, draw, row), in unsigned 64-bit arithmetic that wraps:
 *     x = (uint64(draw) << 32) | uint32(row);  z = x + (seed + 1) * 0x9E3779B97F4A7C15;
 *     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31;  u = z >> 40   (24 bits)
 *     row is kept  <=>  u < (uint32) floor(subsample * 2^24)        subsample in [2^-24, 1]; 1.0 keeps every row
 * row is the ABSOLUTE row index in the data set, draw >= 0 is the caller's to choose.  The sample of the rows [row0, row0 + n) is the ascending
 * list of the kept indices: no replacement, the same list on the host and on the device, independent of how a range is cut.
 *   gbrl_hip_sample_rows_host(row0, n, subsample, seed, draw, out, count)  the rule itself on the host: out[0 .. *count) (room for n), no device.
 *   gbrl_hip_dataset_sample_rows(ds, row0, n, subsample, seed, draw, out, out_on_device, count)  the same list from the device kernels, on the
 *     data set's device and the null stream: a count launch, a one-block scan of the block counts and a write launch that places every kept
 *     row at its rank (no atomics: two calls give the same bytes).  out has room for n int32, on the host or on the data set's device; *count
 *     may be 0.  The result is a legal `rows` of gbrl_hip_step_prepared and gbrl_hip_predict_continue_prepared when *count > 0.
 *     Both calls refuse (GBRL_HIP_E_INVALID): row0 < 0, n <= 0, draw < 0, a subsample that is NaN or outside [2^-24, 1], NULL out or count, a
 *     range that ends above row 2^31 - 1; the data set call also a NULL or destroyed data set and a range outside [0, n_rows).
 *   gbrl_hip_fit_prepared_sampled(m, ds, targets, .., iterations, valid_ds, valid_targets, .., early_stopping_rounds, min_delta, subsample, seed,
 *     loss_out, valid_loss_out, iterations_done, best_n_trees)  gbrl_hip_fit_prepared_valid growing every tree on a sample of its batch.  With
 *     valid_ds == NULL the validation arguments must be NULL / 0 and it is gbrl_hip_fit_prepared (*best_n_trees is not written).  With
 *     subsample == 1.0 it runs the unsampled loop itself: no sampler launch, no gather, the same bytes, loss and phases, whatever seed is.
 *     Otherwise iteration i, once the held prediction and the gradient of its batch [start, start + bn) are up to date, draws the rows of the
 *     batch with draw = the tree count BEFORE the step (so a fit that is continued continues the sequence), gathers their gradient rows in the
 *     pass that writes the indices, reads the count back (4 bytes) and grows the tree as gbrl_hip_step_prepared(rows) does, with the data set's
 *     thresholds.  A draw that keeps no row of the batch takes the whole batch, as the unsampled iteration does.  A fresh draw per tree (there
 *     is no bagging_freq), never with replacement.  Batches, validation, the stopping rule and the returned loss (on ALL rows of ds) are the
 *     unsampled loop's.  Refused before anything changes (GBRL_HIP_E_INVALID): a bad subsample, and what the two calls above refuse.
 *   gbrl_hip_sample_gather(row0, n, subsample, seed, draw, grads, output_dim, rows_out, grads_out, count)  test access to the launch sequence of
 *     a sampled iteration, on the calling thread's current device and the null stream: grads float32 [n, output_dim] (row r - row0 for row r),
 *     rows_out int32 [n] and grads_out [n, output_dim] are DEVICE buffers; grads_out[j] = grads[rows_out[j] - row0] (16-byte accesses when
 *     output_dim % 4 == 0 and both matrices are 16-byte aligned, 4-byte accesses otherwise).  grads and grads_out may both be NULL.
 *   gbrl_hip_sample_rows_geometry(rows_per_block, scan_width)  the rows one block of the sampler owns and the block counts one slice of its scan
 *     takes (diagnostic; no device needed): the sizes at which the kernels take another path.
 *
 * One-side sampling (new: gradient-based one-side sampling, GOSS -- LightGBM's data_sample_strategy = "goss").  Of the rows [row0, row0 + n) with
 * gradient rows G float32 [n, D] it keeps the rows with the largest gradients and a hash draw of the rest, whose gradients it amplifies so that the
 * histogram sums stay unbiased.  One definition for the host and the device (csrc/sample_core.h), with top_rate = a and other_rate = b:
 *     score   s_r = 0; for d = 0 .. D-1: s_r = fl32(s_r + fl32(g_rd * g_rd))     float32, a separate multiply and add (never contracted)
 *     key     bits(s_r) & 0x7FFFFFFF          non-negative floats order like their bits; an infinity or a NaN ranks by its bits
 *     top     k = floor(a * n) in double; tau = the k-th largest key, exactly.  A row is TOP iff its key is above tau, or equals tau and the row is
 *             among the first k - #{key > tau} such rows in row order: exactly k top rows whatever the ties (on the first tree of a softmax fit every
 *             row of a class has the same gradient).  k == 0: no top rows; tau is then reported as 0x80000000, above every key.
 *     other   a row that is not top is kept iff u(seed ^ 0x676F737372657374, draw, row) < min(2^24, floor(p * 2^24)), p = b / (1 - a) in double; u is
 *             the row sampler's 24-bit hash, the constant ("gossrest") a stream of its own beside the row and column samplers'.  A Bernoulli draw
 *             like subsample's, NOT LightGBM's sequential draw of an exact count: the number of other rows varies around b * n.
 *     amp     fl32((1 - a) / b), the quotient in double.  A kept other row's gradient entries become fl32(amp * g) (the weight rule, one float32
 *             multiply); a top row's entries are copied, so no bit of them changes.
 *     sample  the ascending list of the kept ABSOLUTE rows, their factor (1 or amp) and their gathered gradient rows with the factor applied.
 *   Refused by every call below (GBRL_HIP_E_INVALID, before anything is enqueued): a NaN rate, a outside [0, 1), b outside (0, 1], a + b > 1 (in
 *     double), p < 2^-24, and what gbrl_hip_sample_rows_host refuses about the range and the draw; NULL gradients or outputs, D outside [1, 512].
 *   gbrl_hip_goss_rows_host(grads, output_dim, row0, n, top_rate, other_rate, seed, draw, rows_out, factor_out, grads_out, count)  the rule on the
 *     host, no device: rows_out int32 / factor_out float32 [n] get the *count kept rows, grads_out (may be NULL) [n, output_dim] their gradient rows.
 *   gbrl_hip_dataset_sample_goss(ds, grads, output_dim, row0, n, top_rate, other_rate, seed, draw, rows_out, factor_out, grads_out, on_device, count,
 *     n_top, tau_bits)  the same bytes from the device kernels, on the data set's device and the null stream; grads and the three outputs (room for n
 *     rows each) are all on the host or all on that device.  One pass computes scores and keys and counts their first digit; an MSD radix count over
 *     the 32-bit keys (8 bits a pass, integer counts only) finds tau and the ties to take and leaves them in device memory; the tie counts of the
 *     sampler's blocks are scanned; then the row sampler's count / scan / write passes run with the keep rule above -- a kept row's position is its
 *     rank, no atomic hands out a position, two calls give the same bytes.  *n_top = k, *tau_bits = tau (either may be NULL).  Also refused: a NULL
 *     or destroyed data set, a range outside [0, n_rows).
 *   gbrl_hip_fit_prepared_goss(.., weights, .., goss_top, goss_other, loss_out, ..)  gbrl_hip_fit_prepared_weighted plus the two rates; the older
 *     calls are this one with goss_other == 0, which enqueues nothing new.  With goss_other > 0 the one-side draw takes the place of the subsample
 *     draw: over the batch [start, start + bn), draw = the tree count BEFORE the step, on the gradient as the held prediction's launch left it (with
 *     weights the scores are those of fl32(w * g), as in LightGBM).  tau never visits the host; the only wait is the 4-byte read-back of the count.
 *     A draw that keeps no row takes the whole batch unamplified.  newton: the sums run over the kept rows with the effective weights e_r =
 *     fl32(w_r * factor_r) (w_r = 1 without weights) and weight_max = fl32(wmax * amp).  colsample, validation, metrics, warm starts and batch_size
 *     < n work as with subsample.  The model is byte for byte the loop objective_gradient -> sample_goss -> step_prepared(rows) ->
 *     newton_leaves_prepared_weighted(rows, e, weight_max) -> predict_continue_prepared.  Also refused before anything changes: goss with subsample
 *     < 1; fl32(wmax * amp) > 65536 (wmax = 1 without weights), once the weights are known and before any tree is grown.  There is no warm-up of
 *     1 / learning_rate unsampled iterations, and GOSS does not reach fit() or step().
 *     What it does NOT do: like a row weight, the factor is a gradient multiplier.  The histogram SUMS are unbiased, but a gradient leaf stores
 *     the mean of the amplified gradients over the KEPT rows (the row counts are unchanged), about 1 / (top_rate + other_rate) times the batch
 *     mean: with leaf_update = gradient a GOSS fit steps that much further per tree (lower the learning rate accordingly).  A Newton leaf stores
 *     sum e g / (sum e h + leaf_l2), which the amplification leaves unbiased, as in LightGBM.
 *
 * Column subsampling (new: the other half of stochastic gradient boosting -- LightGBM's feature_fraction, XGBoost's colsample_bytree,
 * scikit-learn's max_features per tree).  A weight of 0 (gbrl_hip_set_feature_weights) only removes a column's candidates from the arg-max; a
 * column subset skips the column's histogram.  The column rule is a definition, on the host, with the row sampler's 24-bit hash u(seed, draw, x):
 *     k   = max(1, floor(colsample * F + 0.5))                  in double; colsample in (0, 1], NaN refused; 1.0 keeps every column
 *     u_f = u(seed ^ 0x636F6C73616D706C, draw, f)               f = 0 .. F - 1
 *     the kept columns are the k smallest pairs (u_f, f), returned ascending in f            (always exactly k columns)
 *   gbrl_hip_sample_cols_host(n_features, colsample, seed, draw, out, count)  the rule: out[0 .. *count) (room for n_features), no device.  Refused
 *     (GBRL_HIP_E_INVALID): n_features < 1, draw < 0, a colsample that is NaN or outside (0, 1], NULL out or count.
 *   gbrl_hip_step_prepared_cols(m, ds, grads, grads_on_device, rows, rows_on_device, n_rows, cols, n_cols)  gbrl_hip_step_prepared growing on the
 *     columns cols only: a HOST int32 vector, strictly ascending, entries in [0, n_features), 1 <= n_cols <= n_features; anything else is refused
 *     (GBRL_HIP_E_INVALID) before anything changes.  The 32-byte code records are re-packed into ceil(n_cols / 16) groups -- rows, when given, in the
 *     same pass -- with the thresholds of those columns, and every growth path runs on n_cols features.  The model is what a model of input_dim
 *     n_cols with feature weights w[cols] grows on a data set of obs[:, cols], except that its conditions name the data set's columns (feature
 *     index cols[f']): ascending order keeps the tie rule (the lowest candidate index wins), and the candidate weight of column c is what the
 *     full step uses for feature c.  The model still latches n_num_features = n_features.  cols naming every column is gbrl_hip_step_prepared:
 *     no gather, the same bytes and phases.  Phase `gather_cols` (gbrl_hip_last_phase_times); `gather_codes` stays the row-only gather.
 *   gbrl_hip_dataset_codes_cols(ds, rows, rows_on_device, n_rows, cols, n_cols, out)  gbrl_hip_dataset_codes for a column subset: out
 *     [ceil(n_cols / 16)][m][16], out[g][j][i] = the code of column cols[16 g + i] and row rows[j] (rows NULL: every row), padding slots 0.
 *   gbrl_hip_fit_prepared_colsampled(.., subsample, colsample, seed, ..)  gbrl_hip_fit_prepared_sampled plus colsample; the older fit_prepared calls
 *     are this call with colsample == 1.0, which runs their code itself whatever seed is.  Otherwise iteration i draws its columns with the rule
 *     above at draw = the tree count BEFORE the step and the row sampler's seed, and grows as gbrl_hip_step_prepared_cols does (on the sampled
 *     rows when subsample < 1: one pass over the codes).  A draw of all columns (n_features == 1, or a fraction that rounds to it) is the step
 *     without cols.  The held prediction, validation, the stopping rule and the loss see all rows and all columns; trees carry data set
 *     feature indices and thresholds.  Refused before anything changes: a bad colsample, and what gbrl_hip_fit_prepared_sampled refuses.
 *   gbrl_hip_gather_cols_geometry(rows_per_tile, max_staged_groups)  the rows one block of the column gather owns, and the source groups it
 *     stages at a time: a subset that touches more is walked in chunks by the same kernel (diagnostic; no device needed).
 *
 * Classification objectives (new: fit_prepared beyond MultiRMSE).  The trees and the outputs are what they were -- D raw scores, p moves by
 * -lr * value along the mean gradient of a leaf -- only the gradient rule g = dL/dp and the loss change.  Every float32 step below is ONE
 * definition shared by the host and the device (csrc/objective_core.h): the same bits on either.
 *   obj_exp(t), t <= 0: k = rint(t log2 e); r = t - k ln2 in two parts (fmaf); exp(r) = 1 + (r + r^2 P(r)), P of degree 5 in fmaf; times 2^k through
 *     the exponent bits.  No libm, no fast intrinsic, no contraction.  t < -104 gives +0.  The value p 2^k is within 2^-22 relative of exp(t) on
 *     all of [-104, 0]; the rules below use it rounded once to float32 (obj_exp_f32: subnormal below t = -87.34), written obj_exp for short.
 *   GBRL_HIP_OBJ_LOGISTIC, output_dim >= 1, targets float32 [n, D]: e = obj_exp(-|p|); s = p >= 0 ? 1 / (1 + e) : e / (1 + e) (correctly rounded
 *     division); g = fl32(s - y).  Row loss, float64 from the float32 p: sum_d [max(p, 0) - y p + log1p(exp(-|p|))].
 *   GBRL_HIP_OBJ_SOFTMAX, output_dim >= 2, targets int32 [n], labels in [0, D): m = max_c p_c; t_c = fl32(p_c - m) (0 where p_c == m, so that a
 *     score of +inf is the maximum and not inf - inf); e_c = obj_exp(t_c); S = float32 sum of e_c, c ascending; q_c = e_c / S;
 *     g_c = fl32(q_c - [c == y]).  Row loss, float64: log(sum_c exp((double)p_c - m)) + m - p_y.
 *   GBRL_HIP_OBJ_RMSE: g = fl32(p - y) and the MultiRMSE expression, as ever.
 *   The float64 row losses are reduced as MultiRMSE's are (one partial per 64 rows, a fixed tree: no floating-point atomics).  The loss of a set
 *   is sum / n in float64 -- not a square root -- for the two new objectives.
 *   gbrl_hip_fit_prepared_objective(.., seed, objective, ..)  gbrl_hip_fit_prepared_colsampled plus the objective; the two targets are float32
 *     [n, D] (rmse, logistic) or int32 [n] (softmax).  The older calls are this one with GBRL_HIP_OBJ_RMSE, which runs their code itself.  A
 *     fresh model (n_trees == 0) gets, computed on the host in double: logistic bias_d = (float)log(c / (1 - c)), c = clamp(mean_d(y), 1 / 2n,
 *     1 - 1 / 2n); softmax bias_c = (float)log(max(n_c, 0.5) / n), n_c the rows of class c, counted on the device with integer atomics.
 *     The launch that advances the held prediction writes the objective's gradient; the validation launch its loss partials;
 *     valid_loss_out[k] = sum / n_valid; *loss_out = (float)(sum / n) over all rows.  Batches, sampling, warm starts and the stopping rule are
 *     untouched.  Refused before anything changes (GBRL_HIP_E_INVALID): an unknown objective, softmax with output_dim < 2, a label outside
 *     [0, D) in either set (the message names the first one found), and what gbrl_hip_fit_prepared_colsampled refuses.
 *   gbrl_hip_objective_gradient(m, pred, pred_on_device, targets, targets_on_device, n, objective, grad_out, loss_out)  the same device
 *     functions on a prediction matrix [n, output_dim], on the model's device and stream: grad_out [n, D] (where pred is: a device buffer iff
 *     pred_on_device) and / or *loss_out (host; sum / n, or the MultiRMSE expression for rmse).  Either output may be NULL, not both.
 *   gbrl_hip_objective_gradient_host(pred, targets, n, D, objective, grad_out)  the gradient rule with no device: the same bits.
 *   gbrl_hip_objective_exp_host(t, n, out, out_f32)  out[i] = obj_exp(t[i]), the unrounded value p 2^k as a double, and / or out_f32[i] = that
 *     value rounded once to float32 (obj_exp_f32: the e of the rules above), on the host (diagnostic: what the accuracy test sweeps); t[i] <= 0. */
enum { GBRL_HIP_OBJ_RMSE = 0, GBRL_HIP_OBJ_LOGISTIC = 1, GBRL_HIP_OBJ_SOFTMAX = 2 };
int gbrl_hip_fit_prepared_objective(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                    const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                    double min_delta, double subsample, double colsample, uint64_t seed, int objective, float *loss_out,
                                    double *valid_loss_out /*[iterations + 1]*/, int *iterations_done, int *best_n_trees);
int gbrl_hip_objective_gradient(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device, int n, int objective,
                                float *grad_out /*[n, output_dim]*/, double *loss_out);
int gbrl_hip_objective_gradient_host(const float *pred, const void *targets, int n, int D, int objective, float *grad_out /*[n, D]*/);
int gbrl_hip_objective_exp_host(const float *t, int n, double *out /*[n] or NULL*/, float *out_f32 /*[n] or NULL*/);
/* Classifier metrics (new: what a fitted classifier is watched and stopped on, beyond its mean log loss).  Both are INTEGERS before they are
 * numbers (csrc/metric_core.h, shared by the host rule and the kernels): the counts of the device, of the host rule and of a brute force are
 * equal or wrong -- there is no tolerance -- and every floating-point step is taken on the host from the integers: the same bits.
 *   GBRL_HIP_METRIC_ERROR, GBRL_HIP_OBJ_SOFTMAX: row r is wrong iff argmax_c p[r][c] != label[r], the arg-max being the lowest index among
 *     equal maxima, compared as floats.  E = wrong rows; value = (double)E / n.  counts [1] = E.
 *   GBRL_HIP_METRIC_ERROR, GBRL_HIP_OBJ_LOGISTIC: cell (r, d) is wrong iff (p[r][d] > 0) != (y[r][d] > 0.5) -- a score of exactly 0 predicts
 *     the negative class, a target of exactly 0.5 is negative.  E_d = wrong cells of column d; value = (double)(sum_d E_d) / (n D).
 *     counts [D] = E_d.
 *   GBRL_HIP_METRIC_AUC, GBRL_HIP_OBJ_LOGISTIC, per output column d: positives are the rows with y[r][d] > 0.5 (P_d of them), the other
 *     N_d rows are negatives.  Scores compare through one order-preserving key: -0.0 is first made +0.0; then u = bits(p) and
 *     key = u ^ (u >> 31 ? 0xffffffff : 0x80000000).  A NaN is therefore ordered by its bits: defined, and meaningless.
 *     2U_d = sum over positives i of (#{negatives j : key_j < key_i} + #{negatives j : key_j <= key_i}), a uint64 (ties count half);
 *     AUC_d = (double)(2U_d) / (2.0 * (double)P_d * (double)N_d); value = (sum_d AUC_d, d ascending, in double) / D.
 *     counts [D][3] = (2U_d, P_d, N_d).  On the device: the D score columns are sorted by key in four passes of a segmented radix sort,
 *     the negatives are prefix-counted along every sorted column, and every positive adds the prefix at the two ends of its run of equal
 *     keys; integer atomics only.
 *   Refused, GBRL_HIP_E_INVALID: an unknown metric; a metric with GBRL_HIP_OBJ_RMSE; a column with P_d == 0 or N_d == 0 (auc: the message names
 *     the column); a label outside [0, D).  GBRL_HIP_E_UNSUPPORTED: auc with softmax (a multi-class AUC is a separate decision); auc on
 *     n * D >= 2^31 - 2048 cells; output_dim > 128.
 *   Out of scope: multi-class AUC, metrics for rmse (MAE and the like), a model truncated at best_n_trees, row-sharded models.
 *   gbrl_hip_eval_metric(m, pred, pred_on_device, targets, targets_on_device, n, objective, metric, value_out, counts_out)  the metric of a
 *     prediction matrix [n, output_dim] (targets as for the objective) on the model's device and stream.  value_out and counts_out (host)
 *     may each be NULL, not both.
 *   gbrl_hip_eval_metric_host(pred, targets, n, D, objective, metric, value_out, counts_out)  the definition itself, by std::sort on the
 *     host: no device.  It shares the key and the final division with the device path and nothing else.
 *   gbrl_hip_fit_prepared_metric(.., objective, metric, loss_out, valid_loss_out, valid_metric_out, ..)  gbrl_hip_fit_prepared_objective plus
 *     the metric; the older calls are this one with GBRL_HIP_METRIC_NONE.  With a metric, valid_metric_out[k], k = 0 .. *iterations_done, is
 *     gbrl_hip_eval_metric_host of the validation rows' prediction after k iterations, and the stopping rule and *best_n_trees follow that
 *     curve in place of the loss curve: the error as it is, the AUC negated.  valid_loss_out is recorded as ever.  The metric only reads the
 *     held validation prediction: the model is byte for byte what the call without it leaves after the same number of iterations.
 *     Refused before anything changes: a metric without a validation set, the refusals above (a single-class column of valid_targets
 *     included), a NULL valid_metric_out with a metric. */
enum { GBRL_HIP_METRIC_NONE = 0, GBRL_HIP_METRIC_ERROR = 1, GBRL_HIP_METRIC_AUC = 2 };
int gbrl_hip_fit_prepared_metric(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                 const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                 double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, float *loss_out,
                                 double *valid_loss_out /*[iterations + 1]*/, double *valid_metric_out /*[iterations + 1]*/, int *iterations_done,
                                 int *best_n_trees);
int gbrl_hip_eval_metric(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device, int n, int objective,
                         int metric, double *value_out, int64_t *counts_out);
int gbrl_hip_eval_metric_host(const float *pred, const void *targets, int n, int D, int objective, int metric, double *value_out, int64_t *counts_out);
/* Newton leaf values (new: the second-order step a classifier's leaves take in scikit-learn, XGBoost and LightGBM).  A tree is grown on the
 * gradient g = dL/dp as ever; with GBRL_HIP_LEAF_NEWTON every leaf then stores v = (sum g) / (sum h + leaf_l2) over the rows the tree was grown
 * on instead of the mean of g, h = d2L/dp2 (softmax: the diagonal).  Predictions move by -rate * v, the sign convention is unchanged.
 * csrc/newton_core.h defines all of it once for the host and the kernels:
 *   hessian   logistic: e = exp32(-|p|), den = 1 + e as in the gradient; h = fl32(fl32(1 / den) * fl32(e / den)), both quotients correctly
 *             rounded -- no 1 - s cancels, h(p) == h(-p) bit for bit, h(0) = 0.25.  softmax: q_c exactly as the gradient computes it,
 *             h_c = fl32(q_c * fl32(1 - q_c)).  The gradient is gbrl_hip_objective_gradient_host's, bit for bit.
 *   sums      bits = min(40, 62 - bit_length(m)) for m summed rows; q(x) = llrint((double)x * 2^bits) for g and h alike; per leaf the int64
 *             Sg[D], Sh[D] and cnt.  |g| <= 1 and h <= 0.25: no sum reaches 2^62.  Integer adds on the device: every run, and both kernel
 *             families, give the same bytes.
 *   value     on the host in double: G = Sg / 2^bits, H = Sh / 2^bits, den = H + leaf_l2, v = (float)(G / den).  A leaf keeps the value it
 *             has when cnt == 0, when its depth is 0, or when !(den > 0).
 *   gbrl_hip_newton_leaves_prepared(m, ds, rows, rows_on_device, n_rows, pred, pred_on_device, targets, targets_on_device, objective, tree,
 *     leaf_l2, sums_out, bits_out, values_out)  the rule applied to ONE tree (tree == -1: the last) over the data set rows rows[0 .. n_rows)
 *     (NULL: every row, n_rows == the data set's).  pred [n_rows, output_dim] is the caller's prediction over the trees [0, tree) and, like
 *     targets ([n_rows, output_dim] float32, or int32 [n_rows] labels for softmax), is indexed by position.  sums_out (host, may be NULL)
 *     int64 [leaves, 2 output_dim + 1] = (Sg, Sh, cnt) per leaf of the tree; *bits_out (may be NULL); values_out (host, may be NULL) float32
 *     [leaves, output_dim], what the model holds afterwards.  Only that tree's values change; only its slice of the device mirror is sent
 *     again.  Refused before anything changes: what gbrl_hip_predict_continue_prepared refuses about the model, the data set and rows;
 *     output_dim > 128; GBRL_HIP_OBJ_RMSE (GBRL_HIP_E_INVALID: its Newton step is the gradient mean the step stores); a leaf_l2 that is
 *     negative, NaN or infinite; a tree outside the model; a label outside [0, output_dim).  Found by the kernel and refused with the model
 *     unchanged (GBRL_HIP_E_INVALID): a logistic target outside [0, 1] (a NaN counts), a prediction that is not finite.
 *   gbrl_hip_objective_hessian_host(pred, n, D, objective, hess_out)  the hessian rule on the host, no device (rmse: 1).
 *   gbrl_hip_newton_values_host(sums, n_leaves, D, bits, old_values, depths, leaf_l2, values_out)  the value rule on the host, no device:
 *     sums int64 [n_leaves, 2 D + 1], old_values float32 [n_leaves, D], depths int32 [n_leaves].
 *   gbrl_hip_newton_sum_bits(m)  the bits of the quantum for m rows.
 *   gbrl_hip_fit_prepared_leaf(.., objective, metric, leaf_update, leaf_l2, ..)  gbrl_hip_fit_prepared_metric plus the leaf rule; the older
 *     calls are this one with GBRL_HIP_LEAF_GRADIENT and leaf_l2 = 1.  GBRL_HIP_LEAF_NEWTON: right after every step the new tree's leaves get
 *     gbrl_hip_newton_leaves_prepared's values from the rows the tree was grown on (the batch; the kept rows of a sampled iteration, the whole
 *     batch when the draw kept none) at the held prediction; the held predictions, the validation curve and the returned loss see them.  The
 *     model is byte for byte the loop objective_gradient -> step_prepared -> newton_leaves_prepared -> predict_continue_prepared written by
 *     hand.  GBRL_HIP_LEAF_GRADIENT enqueues nothing new.  Refused before anything changes (GBRL_HIP_E_INVALID): an unknown leaf_update,
 *     newton with GBRL_HIP_OBJ_RMSE, a bad leaf_l2, and with newton and logistic a training target outside [0, 1].
 *   Out of scope: Newton values in fit(), step() and refit_leaves, hessian-weighted split scores, min_child_weight, the full softmax hessian,
 *     row-sharded models. */
enum { GBRL_HIP_LEAF_GRADIENT = 0, GBRL_HIP_LEAF_NEWTON = 1 };
int gbrl_hip_newton_leaves_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const float *pred,
                                    int pred_on_device, const void *targets, int targets_on_device, int objective, int tree, double leaf_l2,
                                    int64_t *sums_out /*[leaves, 2 output_dim + 1]*/, int *bits_out, float *values_out /*[leaves, output_dim]*/);
int gbrl_hip_objective_hessian_host(const float *pred, int n, int D, int objective, float *hess_out /*[n, D]*/);
int gbrl_hip_newton_values_host(const int64_t *sums, int n_leaves, int D, int bits, const float *old_values, const int32_t *depths, double leaf_l2,
                                float *values_out /*[n_leaves, D]*/);
int gbrl_hip_newton_sum_bits(int64_t m);
int gbrl_hip_fit_prepared_leaf(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                               const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                               double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update,
                               double leaf_l2, float *loss_out, double *valid_loss_out /*[iterations + 1]*/,
                               double *valid_metric_out /*[iterations + 1]*/, int *iterations_done, int *best_n_trees);
/* Row weights (new: LightGBM's weight, XGBoost's and scikit-learn's sample_weight, for fit_prepared and its public pieces).  weights is float32
 * [n], one per data set row; every entry finite and in [0, 65536] (GBRL_HIP_WEIGHT_MAX); W = sum_r (double)w_r, reduced in float64 in a fixed
 * order (two calls give the same bits), must be > 0 where a loss or a bias is taken.  csrc/objective_core.h and csrc/newton_core.h define the
 * rule once for the host and the kernels, contraction off:
 *   gradient  g_w = fl32(w * g), g bit for bit the unweighted gradient (rmse: fl32(p - y)).  The tree is grown on g_w.  w == 1 changes no bit.
 *   hessian   h_w = fl32(w * h).
 *   loss      sum_r (double)w_r * L_r in place of sum_r L_r and W in place of the row count, the formulas otherwise unchanged (rmse:
 *             sqrt(0.5 * sum / W)).  L_r is the float64 row loss as before; the product is one float64 multiply in front of the wave butterfly;
 *             the partials and the finishing sum keep their fixed order.
 *   bias      of a fresh model.  rmse: sum_r w_r y_rd / W per column; logistic: the log odds of that mean, the clamp 0.5 / n kept; softmax:
 *             log(max(W_c, 0.5 * W / n) / W), W_c the weight of class c.  The sums are the column sums' own reduction with the weight as a per-row
 *             factor (the product of two float32 is exact in float64): all-ones weights give the unweighted bias bits.
 *   newton    Sg += q(g_w), Sh += q(h_w), cnt counts rows; bits = min(40, 62 - bit_length(m) - e), e the smallest integer >= 0 with weight_max <=
 *             2^e: |g_w| <= 2^e, so |sum| < 2^62 still, and e = 0 is the unweighted rule.  weight_max is an INPUT of the rule: fit_prepared uses
 *             the maximum over the training weights of the whole data set; gbrl_hip_newton_leaves_prepared_weighted takes it (negative: the
 *             maximum of the weights given), so that a caller's loop over sampled rows reproduces the fit's bits.  The value rule is unchanged.
 *   What weights do NOT do.  Split scores see weighted gradients, but their row counts (L2's sum^2 / count, min_data_in_leaf) are unchanged.  A
 *             gradient leaf stores the mean of w g over its rows: weights act as gradient multipliers, and weights with mean 1 keep the step
 *             size.  A Newton leaf stores the properly weighted ratio sum w g / (sum w h + leaf_l2).  A zero-weight row still counts as a row of
 *             its leaf: to drop rows use rows / subsample.  Hessian- or weight-aware split scores, min_child_weight, weighted metrics, weights
 *             in fit(), step() and refit_leaves, and row-sharded models are out of scope.
 *   gbrl_hip_fit_prepared_weighted(.., leaf_update, leaf_l2, weights, weights_on_device, valid_weights, valid_weights_on_device, loss_out, ..,
 *     best_n_trees, weight_max_out)  gbrl_hip_fit_prepared_leaf plus the training weights [n] and the validation weights [valid rows] (each
 *     may be NULL); the older calls are this one with both NULL and enqueue the kernels and arguments they always did.  The weight rides in the
 *     launches that advance the held predictions and sum the Newton leaves as one more float per row; a weighted rmse run takes its training
 *     loss from the held prediction (gbrl_hip_objective_gradient_weighted's loss, bit for bit), not from the column sums of the gradient.
 *     valid_weights weigh valid_loss_out only.  *weight_max_out (may be NULL): the largest training weight, 0 without weights.  The model is
 *     byte for byte the loop objective_gradient_weighted -> step_prepared -> newton_leaves_prepared_weighted(weight_max) ->
 *     predict_continue_prepared.  Refused before anything changes (GBRL_HIP_E_INVALID): an entry of either vector that is NaN, negative,
 *     infinite or above 65536 (the message names the first such row), W == 0, valid_weights without valid_ds; (GBRL_HIP_E_UNSUPPORTED):
 *     valid_weights with a metric -- the metrics are exact integer counts of rows.  Training weights with a metric are fine.
 *   gbrl_hip_objective_gradient_weighted(m, pred, .., targets, .., weights, weights_on_device, n, objective, grad_out, loss_out)
 *     gbrl_hip_objective_gradient with weights [n] (NULL: that call): grad_out = g_w, *loss_out the weighted loss.  Refused: a bad entry, W == 0.
 *   gbrl_hip_newton_leaves_prepared_weighted(.., leaf_l2, weights, weights_on_device, weight_max, sums_out, bits_out, values_out)
 *     gbrl_hip_newton_leaves_prepared with weights [n_rows], indexed by position.  Refused before anything changes: a bad entry; a weight_max
 *     below the largest weight given, above 65536 or NaN; a weight_max >= 0 without weights.  (No W is taken: all-zero weights leave every leaf
 *     with its regularised value 0 / leaf_l2.)
 *   gbrl_hip_objective_gradient_host_weighted / gbrl_hip_objective_hessian_host_weighted(.., weights, ..)  the two rules on the host with weights
 *     [n] (NULL: the unweighted call); a bad entry is refused.  gbrl_hip_newton_sum_bits_weighted(m, weight_max): the bits, or GBRL_HIP_E_INVALID
 *     for a weight_max that is NaN, negative or above 65536. */
#define GBRL_HIP_WEIGHT_MAX 65536.0f
int gbrl_hip_fit_prepared_weighted(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                   const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                   double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update,
                                   double leaf_l2, const float *weights /*[n]*/, int weights_on_device, const float *valid_weights /*[valid rows]*/,
                                   int valid_weights_on_device, float *loss_out, double *valid_loss_out /*[iterations + 1]*/,
                                   double *valid_metric_out /*[iterations + 1]*/, int *iterations_done, int *best_n_trees, float *weight_max_out);
int gbrl_hip_objective_gradient_weighted(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device,
                                         const float *weights /*[n]*/, int weights_on_device, int n, int objective, float *grad_out /*[n, output_dim]*/,
                                         double *loss_out);
int gbrl_hip_newton_leaves_prepared_weighted(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows,
                                             const float *pred, int pred_on_device, const void *targets, int targets_on_device, int objective, int tree,
                                             double leaf_l2, const float *weights /*[n_rows]*/, int weights_on_device, float weight_max,
                                             int64_t *sums_out /*[leaves, 2 output_dim + 1]*/, int *bits_out, float *values_out /*[leaves, output_dim]*/);
int gbrl_hip_objective_gradient_host_weighted(const float *pred, const void *targets, const float *weights /*[n]*/, int n, int D, int objective,
                                              float *grad_out /*[n, D]*/);
int gbrl_hip_objective_hessian_host_weighted(const float *pred, const float *weights /*[n]*/, int n, int D, int objective, float *hess_out /*[n, D]*/);
int gbrl_hip_newton_sum_bits_weighted(int64_t m, float weight_max);
int gbrl_hip_goss_rows_host(const float *grads /*[n, output_dim]*/, int output_dim, int row0, int n, double top_rate, double other_rate, uint64_t seed, int draw,
                            int32_t *rows_out /*[n]*/, float *factor_out /*[n]*/, float *grads_out /*[n, output_dim], may be NULL*/, int *count);
int gbrl_hip_dataset_sample_goss(const gbrl_hip_dataset *ds, const float *grads /*[n, output_dim]*/, int output_dim, int row0, int n, double top_rate,
                                 double other_rate, uint64_t seed, int draw, int32_t *rows_out /*[n]*/, float *factor_out /*[n]*/,
                                 float *grads_out /*[n, output_dim]*/, int on_device, int *count, int *n_top, uint32_t *tau_bits);
int gbrl_hip_fit_prepared_goss(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                               const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                               double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update,
                               double leaf_l2, const float *weights /*[n]*/, int weights_on_device, const float *valid_weights /*[valid rows]*/,
                               int valid_weights_on_device, double goss_top, double goss_other, float *loss_out,
                               double *valid_loss_out /*[iterations + 1]*/, double *valid_metric_out /*[iterations + 1]*/, int *iterations_done,
                               int *best_n_trees, float *weight_max_out);
/* Quantile regression (new: LightGBM's objective="quantile", scikit-learn's loss="quantile", XGBoost's reg:quantileerror).  csrc/quantile_core.h
 * defines all of it once for the host and the kernels; like the AUC and the Newton sums the result is integers before it is a number, and every
 * selected value is one of the inputs, bit for bit.
 *   levels      alpha float32 [output_dim], one per output, every entry finite and strictly inside (0, 1); anything else is GBRL_HIP_E_INVALID naming
 *               the output.
 *   GBRL_HIP_OBJ_QUANTILE, output_dim >= 1, targets float32 [n, D]: x = fl32(p - y) (the bits of the rmse gradient); g = x > 0 ? fl32(1 - a_d) :
 *               (x < 0 ? -a_d : 0).  Row loss in float64 from the float32 inputs: u = (double)y - (double)p, sum_d (u >= 0 ? a_d u : (a_d - 1) u); loss and
 *               valid_loss are the mean row loss, reduced in the fixed order of the other objectives.  g is dL/dp.
 *   rank        a leaf of m >= 1 rows: k = clamp(ceil(a_d m), 1, m), the product EXACT (a_d = M 2^-s, M < 2^24, m < 2^31: 64-bit integers and a shift; a
 *               shift that leaves the word gives 1).  A double product can round across an integer and is not the rule.
 *   leaf value  GBRL_HIP_LEAF_QUANTILE: v[leaf][d] = the k-th LARGEST x among the rows of the leaf (-0 counts as +0), no arithmetic on it.  Predictions
 *               move by -rate v; -v is the k-th smallest residual y - p: NumPy's quantile(method="inverted_cdf"), a minimiser of the leaf's pinball sum
 *               -- where a gradient leaf, the mean of values in [-a, 1 - a], moves a fit by at most the learning rate per tree.  A leaf without rows or
 *               of depth 0 keeps the value the step gave it.
 *   bias        of a fresh model: the same rule on one leaf of every row at p = 0: bias_d = the k-th smallest y_d, k from n.
 *   gbrl_hip_fit_prepared_quantile(.., goss_top, goss_other, alpha, loss_out, ..)  gbrl_hip_fit_prepared_goss plus alpha (host [D]); the older entries are
 *     this one with NULL and enqueue exactly what they did.  GBRL_HIP_LEAF_QUANTILE: right after every step the new tree's leaves get
 *     gbrl_hip_quantile_leaves_prepared's values from the rows the tree was grown on (the batch; the kept rows of a subsampled iteration), one enqueue
 *     and one read-back, only that tree's values sent again: the model is byte for byte the loop objective_gradient -> step_prepared ->
 *     quantile_leaves_prepared -> predict_continue_prepared written by hand.  Refused before anything changes: GBRL_HIP_OBJ_QUANTILE without alpha, alpha
 *     with another objective, a bad level, GBRL_HIP_LEAF_QUANTILE with another objective, GBRL_HIP_LEAF_NEWTON with GBRL_HIP_OBJ_QUANTILE (the hessian
 *     is zero), a metric with it, a training target that is not finite (a fresh model or a warm start); (GBRL_HIP_E_UNSUPPORTED) weights or valid_weights with it, goss with
 *     GBRL_HIP_LEAF_QUANTILE (both would need a weighted quantile; goss with gradient leaves works as with any objective).
 *   gbrl_hip_quantile_leaves_prepared(m, ds, rows, rows_on_device, n_rows, pred, .., targets, .., alpha, tree, values_out, counts_out, ranks_out)  the
 *     leaves of ONE tree (-1: the last) from the data set rows `rows` (NULL: all of them); pred and targets [n_rows, D] are indexed by position.  Two
 *     kernel paths (an MSD radix select per (leaf, output) for trees of up to max_select_leaves leaves; a sort by key and leaf id beyond, and behind
 *     GBRL_HIP_CONTINUE_GENERIC=1) return the same bytes.  values_out [leaves, D] what the model now holds, counts_out int64 [leaves], ranks_out int64
 *     [leaves, D] (0 for an empty leaf); each may be NULL.  Refused before anything changes: whatever gbrl_hip_newton_leaves_prepared refuses about the
 *     model, the data set, rows, the tree and output_dim, and a bad level; after the launch, the model unchanged: a prediction, a target or a residual
 *     that is not finite.
 *   gbrl_hip_leaf_quantile_host(x [m, D], leaves [m], m, D, n_leaves, alpha, values_out, counts_out, ranks_out)  the rule with no device (an entry of
 *     leaves outside [0, n_leaves) joins no leaf; an empty leaf has the value 0).  gbrl_hip_quantile_rank(m, a, rank_out)  the rank function.
 *   gbrl_hip_leaf_quantile_geometry(max_select_leaves, rows_per_chunk)  the largest tree of the select path and the rows one block of its count pass
 *     takes at a time, for tests that straddle them.
 *   gbrl_hip_objective_gradient_quantile / gbrl_hip_objective_gradient_host_quantile(.., alpha, ..)  the objective calls with the levels (NULL: those
 *     calls); the same bits on both sides.
 *   Out of scope: weighted and interpolated quantiles, Huber and L1 as objectives of their own, quantile leaves in fit(), step() and refit_leaves,
 *     crossing-quantile repair. */
enum { GBRL_HIP_OBJ_QUANTILE = 3 };
enum { GBRL_HIP_LEAF_QUANTILE = 2 };
int gbrl_hip_fit_prepared_quantile(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                                   const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                   double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update,
                                   double leaf_l2, const float *weights /*[n]*/, int weights_on_device, const float *valid_weights /*[valid rows]*/,
                                   int valid_weights_on_device, double goss_top, double goss_other, const float *alpha /*host [output_dim], may be NULL*/,
                                   float *loss_out, double *valid_loss_out /*[iterations + 1]*/, double *valid_metric_out /*[iterations + 1]*/,
                                   int *iterations_done, int *best_n_trees, float *weight_max_out);
int gbrl_hip_quantile_leaves_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const float *pred,
                                      int pred_on_device, const float *targets, int targets_on_device, const float *alpha /*host [output_dim]*/, int tree,
                                      float *values_out /*[leaves, D]*/, int64_t *counts_out /*[leaves]*/, int64_t *ranks_out /*[leaves, D]*/);
int gbrl_hip_leaf_quantile_host(const float *x /*[m, D]*/, const int32_t *leaves /*[m]*/, int m, int D, int n_leaves, const float *alpha /*[D]*/,
                                float *values_out /*[n_leaves, D]*/, int64_t *counts_out /*[n_leaves]*/, int64_t *ranks_out /*[n_leaves, D]*/);
int gbrl_hip_quantile_rank(int64_t m, float a, int64_t *rank_out);
void gbrl_hip_leaf_quantile_geometry(int *max_select_leaves, int *rows_per_chunk);
int gbrl_hip_objective_gradient_quantile(gbrl_hip_model *m, const float *pred, int pred_on_device, const void *targets, int targets_on_device,
                                         const float *alpha /*host [output_dim]*/, int n, int objective, float *grad_out, double *loss_out);
int gbrl_hip_objective_gradient_host_quantile(const float *pred, const void *targets, const float *alpha /*[D]*/, int n, int D, int objective,
                                              float *grad_out /*[n, D]*/);
/* Ranking objectives on query groups (new: LightGBM's lambdarank with group=, XGBoost's rank:pairwise and rank:ndcg; a query of two rows with labels
 * (1, 0) under the pairwise objective is the Bradley-Terry step -log sigmoid(s_0 - s_1) of reward modelling).  csrc/rank_core.h defines all of it once
 * for the host and the kernels (csrc/rank.hip); a ranking gradient is a sum over the other rows of the row's query, so these objectives have calls of
 * their own and every call without query groups refuses their codes.
 *   inputs      scores float32 [n] of a model with output_dim == 1; labels int32 [n], every entry in [0, 30]; group int32 [Q] in host memory, the sizes
 *               of consecutive row runs, each in [1, 1024] (gbrl_hip_rank_geometry), summing to n.
 *   position    pos(i) = #{j in the query of i: s_j > s_i, or s_j == s_i and j < i}: 0-based, the float compare (-0 == +0).
 *   discounts   disc[t] = 1 / log2(t + 2), t in [0, 1024), float64: ONE table built on the host (gbrl_hip_rank_discounts) that host rule and kernels both
 *               read.  ndcg_at = K > 0: disc[t] counts as 0 for t >= K; 0: no truncation.  gain(l) = 2^l - 1, exact.
 *   ideal DCG   the query's labels in descending order: maxDCG_q = sum_t gain(l_(t)) * disc[t], t ascending, every product and sum rounded on its own;
 *               inv_q = maxDCG_q > 0 ? 1 / maxDCG_q : 0.
 *   pairs       rows i, j of one query with l_i > l_j: delta = fl32(s_i - s_j), rho = sig(-delta), eta = fl32(sig(delta) * sig(-delta)): the logistic
 *               gradient and hessian bits (gbrl_hip_objective_gradient_host at (-delta, 0), gbrl_hip_objective_hessian_host at delta).
 *   weight      GBRL_HIP_OBJ_PAIRWISE: omega = 1.  GBRL_HIP_OBJ_LAMBDARANK: omega = (|gain(l_i) - gain(l_j)| * |disc[pos i] - disc[pos j]|) * inv_q, two
 *               products in that order; a pair with omega == 0 (both rows beyond K) is skipped.
 *   sums        lam = (double)rho * omega, kap = (double)eta * omega; row i (the better one): g -= lam, h += kap; row j: g += lam, h += kap.  Every row
 *               keeps its own two float64 sums from +0.0, partners in ascending row order, each rounded once to float32 at the end.  No atomics: the
 *               bits do not depend on the launch geometry.  g is dL/dp.
 *   ndcg        DCG_q = sum over the query's rows, ascending, of gain(l) * disc[pos]; ndcg_q = maxDCG_q > 0 ? DCG_q * inv_q : 1: bit-exact between host
 *               and device.
 *   loss        lambdarank: 1 - (sum_q ndcg_q) / Q.  pairwise: the mean over the P label-ordered pairs of the logistic row loss at (p = delta, y = 1),
 *               a device-only float64 expression like the logistic loss (0 when P == 0).  Both in the fixed reduction order of the other losses: two
 *               calls give the same bits.
 *   gbrl_hip_rank_gradient(m, pred, pred_on_device, labels, labels_on_device, group, n_groups, n, objective, ndcg_at, grad_out, hess_out, loss_out,
 *     ndcg_out, positions_out, pairs_out)  on the model's device.  grad_out, hess_out [n] float32 and positions_out [n] int32 are where pred is;
 *     ndcg_out float64 [n_groups], loss_out and pairs_out (P, an exact count) are host; each may be NULL.  Refused, GBRL_HIP_E_INVALID, before a kernel
 *     runs: output_dim != 1, another objective, no group, a size outside [1, 1024] (the first such query is named), sizes that do not sum to n,
 *     ndcg_at < 0, ndcg_at > 0 with pairwise; after the label pass: a label outside [0, 30] (the first such row is named); after the launch: a score
 *     that is not finite.  The model is never changed.
 *   gbrl_hip_rank_gradient_host(pred, labels, group, n_groups, n, objective, ndcg_at, ..)  the rule with no device: the same bytes; loss_out must be NULL
 *     for pairwise.  gbrl_hip_rank_discounts(out [1024])  the table.  gbrl_hip_rank_geometry(max_query, max_label)  the caps.
 *   Not LightGBM's lambdarank: no sigmoid parameter (it is 1), no lambdarank_norm, no position-bias terms, no label_gain table.
 *   Out of scope: queries above 1024 rows, output_dim > 1, query or row weights, the ranking objectives inside gbrl_hip_fit_prepared* and
 *     subsample, goss and weights with a ranking objective, ranking in fit(), step() and refit_leaves, MAP and XE-NDCG.
 *   gbrl_hip_fit_prepared_rank(.., alpha, group, n_groups, ndcg_at, valid_group, valid_n_groups, loss_out, ..)  gbrl_hip_fit_prepared_quantile plus the query
 *     sizes of the two sets; the older entries are this one with NULL and enqueue exactly what they did.  targets and valid_targets are the int32 labels.
 *     Per iteration: the held prediction advanced with no fused gradient (gbrl_hip_predict_continue_prepared's launch), the rank kernels into the gradient
 *     (and the hessian for GBRL_HIP_LEAF_NEWTON), the step, the Newton sums from those two buffers (bits = newton_sum_bits(n, largest query), since |g| and h
 *     are below the query size), the validation loss by the same kernels.  A fresh model's bias is 0 (both losses are invariant to a shift).  The model is
 *     byte for byte the loop predict_continue_prepared -> rank_gradient -> step_prepared -> newton_leaves_prepared_rank written by hand; loss_out is the
 *     rule's loss of every row, valid_loss_out[k] gbrl_hip_rank_gradient's loss of the validation prediction after k trees (lower is better: the stopping
 *     rule is unchanged).  Refused before anything changes, GBRL_HIP_E_INVALID: output_dim != 1, no group, group / valid_group / ndcg_at with another
 *     objective, a size outside [1, 1024] (the query is named), sizes that do not sum to the rows, a label outside [0, 30] (the row is named),
 *     batch_size < n (a batch must hold whole queries), subsample < 1, goss, weights or valid_weights, alpha, a metric, GBRL_HIP_LEAF_QUANTILE, a validation
 *     set without valid_group, ndcg_at < 0 or with pairwise, pairwise on a training set without a pair (P == 0).  Found by the kernel during the
 *     iterations: a prediction that is not finite (the model keeps the trees grown so far).
 *   gbrl_hip_newton_leaves_prepared_rank(m, ds, pred, .., labels, .., group, n_groups, objective, ndcg_at, tree, leaf_l2, sums_out, bits_out, values_out)
 *     gbrl_hip_newton_leaves_prepared for a ranking objective, over every row of the data set (a row list would cut queries apart). */
enum { GBRL_HIP_OBJ_PAIRWISE = 4, GBRL_HIP_OBJ_LAMBDARANK = 5 };
int gbrl_hip_rank_gradient(gbrl_hip_model *m, const float *pred, int pred_on_device, const int32_t *labels, int labels_on_device, const int32_t *group /*host*/,
                           int n_groups, int n, int objective, int ndcg_at, float *grad_out /*[n]*/, float *hess_out /*[n]*/, double *loss_out,
                           double *ndcg_out /*host [n_groups]*/, int32_t *positions_out /*[n]*/, int64_t *pairs_out);
int gbrl_hip_rank_gradient_host(const float *pred, const int32_t *labels, const int32_t *group, int n_groups, int n, int objective, int ndcg_at,
                                float *grad_out /*[n]*/, float *hess_out /*[n]*/, double *loss_out, double *ndcg_out /*[n_groups]*/,
                                int32_t *positions_out /*[n]*/, int64_t *pairs_out);
int gbrl_hip_rank_discounts(double *out /*[max_query]*/);
int gbrl_hip_fit_prepared_rank(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int iterations,
                               const gbrl_hip_dataset *valid_ds, const void *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                               double min_delta, double subsample, double colsample, uint64_t seed, int objective, int metric, int leaf_update, double leaf_l2,
                               const float *weights /*[n]*/, int weights_on_device, const float *valid_weights /*[valid rows]*/, int valid_weights_on_device,
                               double goss_top, double goss_other, const float *alpha /*host [output_dim], may be NULL*/,
                               const int32_t *group /*host [n_groups], may be NULL*/, int n_groups, int ndcg_at,
                               const int32_t *valid_group /*host [valid_n_groups], may be NULL*/, int valid_n_groups, float *loss_out,
                               double *valid_loss_out /*[iterations + 1]*/, double *valid_metric_out /*[iterations + 1]*/, int *iterations_done,
                               int *best_n_trees, float *weight_max_out);
int gbrl_hip_newton_leaves_prepared_rank(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *pred, int pred_on_device, const int32_t *labels,
                                         int labels_on_device, const int32_t *group /*host*/, int n_groups, int objective, int ndcg_at, int tree, double leaf_l2,
                                         int64_t *sums_out /*[leaves, 3]*/, int *bits_out, float *values_out /*[leaves, 1]*/);
void gbrl_hip_rank_geometry(int *max_query, int *max_label);
/* Feature importance (new: scikit-learn's feature_importances_ and inspection.permutation_importance, LightGBM's feature_importance, XGBoost's
 * get_score).  Two counts from the host copy of the model and the permutation importance of a data set's columns on the device.
 *   permutation   csrc/perm_core.h defines it once for the host and the kernels (csrc/perm_loss.hip): pi = perm(n, seed, col, repeat) is a bijection of
 *                 [0, n), computed element by element with no state -- a cycle-walking balanced Feistel network of four rounds over 2 * h bits,
 *                 h = ceil(max(2, bit_length(n - 1)) / 2), with the row sampler's hash as round function on a stream of its own ("permutat"); the
 *                 header's opening comment has every constant.  Row i of the variant (col, repeat) reads column col from row pi(i).
 *   gbrl_hip_permutation_host(n, seed, col, repeat, out [n])  the rule with no device.  Refused: n < 1, col < 0, repeat < 0, NULL out.
 *   gbrl_hip_permutation_importance_prepared(m, ds, targets, targets_on_device, objective, alpha, n_repeats, seed, cols, n_cols, n_trees, baseline_out,
 *     loss_out)  on the model's device.  *baseline_out = the loss of the trees [0, n_trees) (n_trees == -1: all) on the data set's rows, walked from the
 *     bias, in the units of valid_loss_out of gbrl_hip_fit_prepared_* for the objective (rmse: sqrt(0.5 sum / n); otherwise sum / n); loss_out (host
 *     float64 [n_cols][n_repeats]) = the same loss with column cols[c] shuffled by perm(n, seed, cols[c], r): bit for bit the validation loss of a
 *     zero-iteration gbrl_hip_fit_prepared_* call on a data set made from the shuffled observations with ds as its reference (binning is per cell).
 *     No variant is materialised: one launch walks up to 64 variants (gbrl_hip_permutation_geometry) over a row tile staged once, patches one 2-byte
 *     code per row on chip, and stores one float64 partial per 64 rows; the partials are summed in the loss paths' fixed order.  cols: host int32,
 *     strictly ascending entries in [0, n_features); NULL: every column.  objective: GBRL_HIP_OBJ_RMSE / LOGISTIC / SOFTMAX / QUANTILE with targets
 *     (host or device) and alpha (host [output_dim], quantile only) as gbrl_hip_fit_prepared_quantile takes them.  A column that no condition of the
 *     walked trees tests is not launched: its entries are the baseline's bits.  Refused before the device is touched, GBRL_HIP_E_INVALID: n_repeats
 *     < 1, cols that break the rule, n_trees outside [1, n_trees of the model] and not -1, NULL targets or outputs, a model without trees, the
 *     ranking objectives (their loss needs query groups), alpha without quantile or quantile without alpha; and whatever
 *     gbrl_hip_predict_continue_prepared refuses about the model and the data set (GBRL_HIP_E_UNSUPPORTED for a tree the thresholds cannot express,
 *     the tree is named).  After the label pass: a softmax label outside [0, output_dim).  Model and data set are left byte for byte as they were.
 *   gbrl_hip_feature_importance(m, kind, leaf_counts, out [input_dim])  no device.  A decision is a level of an oblivious tree (once, not once per node)
 *     or a distinct internal node of a greedy tree (conditions are stored per leaf: path prefixes are deduplicated).  GBRL_HIP_IMPORTANCE_SPLIT:
 *     out[f] = decisions that test feature f.  GBRL_HIP_IMPORTANCE_COVER: out[f] = sum over leaves of leaf_counts[leaf] * (conditions on the leaf's path
 *     that test f), leaf_counts the int64 [n_leaves] vector of gbrl_hip_leaf_counts: the rows that reach every decision on f.  The feature axis is
 *     gbrl_hip_ensemble_shap's: a condition counts at its raw feature index, a categorical one WITHOUT the n_num_features offset, feature_mapping not
 *     applied.  Every value is an integer in float64.  Refused: an unknown kind, cover without leaf_counts, a negative count.
 *   Out of scope: weights, the ranking objectives, categorical columns and row-sharded models (the data-set family has neither), gain importance (the
 *     file format stores no split gain), permuting groups of columns together. */
enum { GBRL_HIP_IMPORTANCE_SPLIT = 0, GBRL_HIP_IMPORTANCE_COVER = 1 };
int gbrl_hip_permutation_host(int n, uint64_t seed, int col, int repeat, int32_t *out /*[n]*/);
int gbrl_hip_permutation_importance_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const void *targets, int targets_on_device, int objective,
                                             const float *alpha /*host [output_dim], may be NULL*/, int n_repeats, uint64_t seed,
                                             const int32_t *cols /*host [n_cols], may be NULL*/, int n_cols, int n_trees, double *baseline_out,
                                             double *loss_out /*host [n_cols][n_repeats]*/);
void gbrl_hip_permutation_geometry(int *launch_variants, int *tile_rows);
int gbrl_hip_feature_importance(const gbrl_hip_model *m, int kind, const int64_t *leaf_counts /*[n_leaves], may be NULL for split*/, double *out /*[input_dim]*/);
/* Partial dependence and ICE curves on a data set, one and two columns (new: scikit-learn's inspection.partial_dependence).  csrc/pd_core.h has the
 * host rules, csrc/pd_rows.hip the kernels.
 *   breaks     A tree ensemble on binned data is a step function of each column.  bins(c) = the sorted distinct bins (gbrl_hip_condition_bins' rule for
 *              the thresholds) of the numeric conditions on column c that the walk of the trees [0, n_trees) reads -- the conditions
 *              gbrl_hip_permutation_importance_prepared counts a used column by, a greedy range's run-on trees included.  codes(c) = [0] + [b + 1 for b
 *              in bins(c)], ascending, k + 1 entries; segment j is the code range [codes[j], codes[j + 1] - 1], the last one runs to n_bins; every code
 *              of a segment answers every walked condition on c alike, so its first code stands for it; in x, segment j >= 1 begins just above
 *              thresholds[c][codes[j] - 1].  A column the walk never tests: [0].
 *   gbrl_hip_partial_dependence_codes(m, thresholds, n_features, n_bins, col, n_trees, out, count)  the rule with no device: out (room for n_bins + 1
 *     entries) = codes(col), *count = k + 1.  n_trees == -1: all.  Only the walked conditions on col are converted.  Refused: NULL thresholds, out or
 *     count, n_features / n_bins that are not the model's, col outside [0, n_features), a model without trees, n_trees outside [1, n_trees of the model]
 *     (GBRL_HIP_E_INVALID); a walked condition on col whose value is not among its thresholds (GBRL_HIP_E_UNSUPPORTED, the tree is named).
 *   gbrl_hip_partial_dependence_prepared(m, ds, variants, n_variants, rows, rows_on_device, n_rows, n_trees, sums_out, ice_out, ice_on_device)  on the
 *     model's device.  variants: host int32 [n_variants][4] = {col0, code0, col1, code1}; col1 == -1: one column; col0 == -1 (col1 then -1 too): the data
 *     set as it is, the baseline.  A variant holds its columns at the constant codes (any code in [0, n_bins]) for every row and leaves every other
 *     column as the row has it.  rows: host or device int32 [n_rows], duplicates allowed, every entry in [0, rows of ds) (gbrl_hip_step_prepared's);
 *     NULL: every row, n_rows == rows of ds.  For each variant the trees [0, n_trees) are walked from the bias: ice_out (may be NULL; host or device
 *     float32 [n_variants][n_rows][output_dim]) = the rows, bit for bit gbrl_hip_predict_continue_prepared from a tiled bias over [0, n_trees) on a data
 *     set that really holds those codes; sums_out (host float64 [n_variants][output_dim]) = the sum over the rows of (double)p[r][d] in a FIXED order:
 *     one partial per 64 consecutive positions of the row list (the loss paths' wave butterfly), finished by the loss paths' finishing kernel.  Two
 *     calls give the same bytes.  The partial dependence is sums_out / n_rows.  No variant is materialised: a launch stages a row tile once, writes up to
 *     two 2-byte codes per row on chip for each of its variants and puts them back; the float64 partials of a launch (8 * variants * output_dim *
 *     ceil(n_rows / 64) bytes) are kept under a fixed budget by cutting the variants per launch (gbrl_hip_partial_dependence_geometry).  A column of a
 *     variant that no walked condition tests is dropped; a variant left without a column is not launched and reports the baseline's bits, as does every
 *     variant of a model in which no optimizer owns an output.  Refused before the device is touched, GBRL_HIP_E_INVALID unless noted: what
 *     gbrl_hip_predict_continue_prepared refuses about the model, the data set and rows (GBRL_HIP_E_UNSUPPORTED: output_dim > 128, a tree the thresholds
 *     cannot express, which is named), a model without trees, n_trees outside [1, n_trees of the model] and not -1, NULL variants or sums_out,
 *     n_variants < 1, a column outside [0, n_features) and not -1, col0 == col1, col1 without col0, a code outside [0, n_bins], more than 2^20 launched
 *     variants, and with ice_out n_variants * n_rows * output_dim >= 2^31 (GBRL_HIP_E_UNSUPPORTED: pass rows).  Model and data set are left byte for
 *     byte as they were.
 *   gbrl_hip_partial_dependence_cells(col0, codes0, n0, col1, codes1, n1, out)  the cells of one entry as variants, no device: col1 < 0: {col0, codes0[i],
 *     -1, 0} for every i; otherwise the row-major product, {col0, codes0[i], col1, codes1[j]} at out[(i * n1 + j) * 4] -- the order of the Python
 *     result's cell axes.  out holds n0 * max(n1, 1) variants.  Refused: col0 < 0, col1 == col0, missing codes, NULL out.
 *   gbrl_hip_partial_dependence_geometry(n_rows, output_dim, ...)  rows per partial (64), the variants one launch takes at that shape (1..64), the most
 *     any launch takes (64), the scratch budget in bytes (64 MiB).
 *   Out of scope: categorical columns and row-sharded models (the data-set family has neither), user grids, weighted means, centred and derivative ICE. */
int gbrl_hip_partial_dependence_codes(const gbrl_hip_model *m, const float *thresholds /*[F*B]*/, int n_features, int n_bins, int col, int n_trees,
                                      int32_t *out /*[n_bins + 1]*/, int *count);
int gbrl_hip_partial_dependence_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *variants /*host [n_variants][4]*/, int n_variants,
                                         const int32_t *rows /*may be NULL*/, int rows_on_device, int n_rows, int n_trees, double *sums_out /*host [n_variants][output_dim]*/,
                                         float *ice_out /*[n_variants][n_rows][output_dim], may be NULL*/, int ice_on_device);
int gbrl_hip_partial_dependence_cells(int col0, const int32_t *codes0, int n0, int col1, const int32_t *codes1 /*may be NULL when col1 < 0*/, int n1,
                                      int32_t *out /*[n0 * max(n1, 1)][4]*/);
void gbrl_hip_partial_dependence_geometry(int n_rows, int output_dim, int *rows_per_partial, int *launch_variants, int *max_launch_variants,
                                          uint64_t *scratch_budget_bytes);
/* SHAP values on a data set: the matrix and its mean |SHAP| reduction (new: LightGBM's pred_contrib on a Dataset).  csrc/shap_core.h has the host rules,
 * csrc/shap.hip the kernels.
 *   decisions  A numeric condition x[f] > v is evaluated as code(row, f) > bin, bin by gbrl_hip_condition_bins' rule for the data set's thresholds (keyed
 *              on the thresholds id like every other data-set call).  Everything else is gbrl_hip_ensemble_shap's device evaluation, rounding for
 *              rounding: the program, the edge weights, the arithmetic and its order.  x > v <=> code > bin for every float (NaN, infinities and signed
 *              zeros included), so the values equal gbrl_hip_ensemble_shap / gbrl_hip_tree_shap on the observations the codes were made from, byte
 *              for byte.
 *   reduction  Positions p = 0 .. n_rows - 1 of the row list fall into tiles t = p / 64.  For each (feature, output) a tile's partial is the sequential
 *              float64 sum, from 0.0, ascending in p, of (double)phi[p][f][d]; a second partial does the same with fabs of the float32.  The total is the
 *              sequential ascending sum of the tile partials from 0.0 (no fused multiply-add anywhere: there is no product).  The result does not depend on
 *              chunk_rows, on rows == NULL against 0 .. n - 1, or on how many launches ran.  A NaN in a column propagates into that column's two totals.
 *   gbrl_hip_shap_prepared(m, ds, rows, rows_on_device, n_rows, tree_idx, norm_values, base_poly, offset, out, out_on_device)  on the model's device.
 *     rows: host or device int32 [n_rows], duplicates allowed, every entry in [0, rows of ds) (gbrl_hip_step_prepared's); NULL: every row, n_rows == rows
 *     of ds.  tree_idx == -1: every tree, summed in tree order; else that tree alone.  norm_values [(max_depth + 1)][max_depth], base_poly [max_depth],
 *     offset [max_depth][max_depth]: host, as gbrl_hip_ensemble_shap takes them.  out: host or device float32 [n_rows][n_features][output_dim], overwritten.
 *   gbrl_hip_shap_importance_prepared(m, ds, rows, rows_on_device, n_rows, norm_values, base_poly, offset, chunk_rows, sum_out, abs_out, chunk_rows_used)
 *     sum_out / abs_out: host float64 [n_features][output_dim], the reduction of the whole ensemble's values over the rows; mean |SHAP| is abs_out /
 *     n_rows.  The matrix is never held whole: chunk_rows positions at a time are evaluated into a float32 scratch [chunk_rows][n_features][output_dim]
 *     (never more rows than n_rows rounded up to a tile), every chunk is reduced to its tile partials [tiles][2][n_features * output_dim], one finishing
 *     launch adds them and 2 * n_features * output_dim doubles are read back.  chunk_rows: a positive multiple of 64; 0: the largest multiple of 64 whose
 *     scratch stays within 64 MiB (partial dependence's budget), and at least 64.  *chunk_rows_used (may be NULL): the value the call worked with.
 *   Both are refused before the device is touched, GBRL_HIP_E_INVALID unless noted: what gbrl_hip_predict_continue_prepared refuses about the model, the
 *     data set and rows (GBRL_HIP_E_UNSUPPORTED: a row-sharded model, a model with categorical columns, output_dim > 128, a tree the thresholds cannot
 *     express, which is named); a NULL polynomial array or result; a model without trees; tree_idx outside [0, n_trees) and not -1; a (max_depth,
 *     output_dim) the kernel has no launch plan for (GBRL_HIP_E_UNSUPPORTED, both are named: the codes live on the device, there is no host evaluation to
 *     hand over to; gbrl_hip_shap_plan tells); chunk_rows negative or no multiple of 64; for gbrl_hip_shap_prepared n_rows * n_features * output_dim >=
 *     2^31 (GBRL_HIP_E_UNSUPPORTED: pass rows, or use the importance call).  Model and data set are left byte for byte as they were.
 *   gbrl_hip_shap_sums_host(phi, n_rows, n_cols, sum_out, abs_out)  the reduction rule with no device: phi host float32 [n_rows][n_cols], both results
 *     float64 [n_cols].
 *   gbrl_hip_shap_geometry(n_features, output_dim, ...)  rows per tile (64), the default chunk_rows at that shape, the scratch budget in bytes (64 MiB).
 *   Out of scope: categorical columns, interaction values, weighted means, a tree range other than all trees or one tree. */
int gbrl_hip_shap_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows /*may be NULL*/, int rows_on_device, int n_rows, int tree_idx /*-1: all*/,
                           const float *norm_values, const float *base_poly, const float *offset, float *out /*[n_rows][n_features][output_dim]*/, int out_on_device);
int gbrl_hip_shap_importance_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows /*may be NULL*/, int rows_on_device, int n_rows,
                                      const float *norm_values, const float *base_poly, const float *offset, int chunk_rows /*0: default*/,
                                      double *sum_out /*host [n_features][output_dim]*/, double *abs_out /*likewise*/, int *chunk_rows_used /*may be NULL*/);
int gbrl_hip_shap_sums_host(const float *phi /*host [n_rows][n_cols]*/, int64_t n_rows, int64_t n_cols, double *sum_out /*[n_cols]*/, double *abs_out /*[n_cols]*/);
void gbrl_hip_shap_geometry(int n_features, int output_dim, int *tile_rows, int *default_chunk_rows, uint64_t *budget_bytes);
int gbrl_hip_sample_rows_host(int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out /*[n]*/, int *count);
int gbrl_hip_dataset_sample_rows(const gbrl_hip_dataset *ds, int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out /*[n]*/,
                                 int out_on_device, int *count);
int gbrl_hip_fit_prepared_sampled(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                                  const gbrl_hip_dataset *valid_ds, const float *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                  double min_delta, double subsample, uint64_t seed, float *loss_out, double *valid_loss_out /*[iterations + 1]*/,
                                  int *iterations_done, int *best_n_trees);
int gbrl_hip_sample_gather(int row0, int n, double subsample, uint64_t seed, int draw, const float *grads, int output_dim, int32_t *rows_out,
                           float *grads_out, int *count);
void gbrl_hip_sample_rows_geometry(int *rows_per_block, int *scan_width);
int gbrl_hip_sample_cols_host(int n_features, double colsample, uint64_t seed, int draw, int32_t *out /*[n_features]*/, int *count);
int gbrl_hip_step_prepared_cols(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *grads, int grads_on_device, const int32_t *rows,
                                int rows_on_device, int n_rows, const int32_t *cols /*host*/, int n_cols);
int gbrl_hip_dataset_codes_cols(const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows, const int32_t *cols /*host*/, int n_cols,
                                uint16_t *out /*[ceil(n_cols / 16)][m][16]*/);
int gbrl_hip_fit_prepared_colsampled(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                                     const gbrl_hip_dataset *valid_ds, const float *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                     double min_delta, double subsample, double colsample, uint64_t seed, float *loss_out,
                                     double *valid_loss_out /*[iterations + 1]*/, int *iterations_done, int *best_n_trees);
void gbrl_hip_gather_cols_geometry(int *rows_per_tile, int *max_staged_groups);
int gbrl_hip_condition_bins(const gbrl_hip_model *m, const float *thresholds /*[F*B]*/, int n_features, int n_bins, int32_t *out);
gbrl_hip_dataset *gbrl_hip_dataset_create_like(gbrl_hip_model *m, const gbrl_hip_dataset *reference, const float *obs, int obs_on_device, int n_samples);
uint64_t gbrl_hip_dataset_thresholds_id(const gbrl_hip_dataset *ds);
int gbrl_hip_fit_prepared_valid(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                                const gbrl_hip_dataset *valid_ds, const float *valid_targets, int valid_targets_on_device, int early_stopping_rounds,
                                double min_delta, float *loss_out, double *valid_loss_out /*[iterations + 1]*/, int *iterations_done, int *best_n_trees);
int gbrl_hip_early_stop_scan(const double *curve, int n, int rounds, double min_delta, int *stop_after, int *best);
int gbrl_hip_predict_continue_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const int32_t *rows, int rows_on_device, int n_rows,
                                       const float *base, int base_on_device, int start_tree, int stop_tree, float *out);
int gbrl_hip_fit_prepared(gbrl_hip_model *m, const gbrl_hip_dataset *ds, const float *targets, int targets_on_device, int iterations,
                          float *loss_out);

/* ---- row-sharded multi-GPU (new; the reference is single-GPU) ------------------------------------------ */
/* One process per GPU, each holding a contiguous block of rows.  When hooks are installed, step() calls them at
 * its exchange points so that every rank grows the identical tree; predict() needs no exchange.  Buffers are
 * DEVICE pointers; the hook must return only after the reduced result is visible on the HIP null stream
 * ordering used by the model.  sum hooks are exact (integers), so the trees of 2/4/8-GPU runs are
 * bit-identical to each other.  Against a ONE-GPU model they are bit-identical when that model holds the exact arg-max too:
 * always for batches above 65 536 rows in GBRL_HIP_PARITY_DEFAULT, and for batches of up to 65 536 rows only against a one-GPU
 * model in GBRL_HIP_PARITY_EXACT_ARGMAX (the one-GPU default replays near-ties there, a row-sharded run cannot).  Install NULL
 * hooks to go back to single-GPU.  Refused (GBRL_HIP_E_UNSUPPORTED) on a model in GBRL_HIP_PARITY_REFERENCE, see above. */
typedef struct {
    void *ctx;
    int world_size, rank;
    int (*allreduce_sum_i64)(void *ctx, int64_t *dev_buf, size_t count);
    int (*allreduce_sum_f64)(void *ctx, double *dev_buf, size_t count);
    int (*allreduce_max_f32)(void *ctx, float *dev_buf, size_t count);
    int (*allreduce_min_f32)(void *ctx, float *dev_buf, size_t count);
} gbrl_hip_collective;
int gbrl_hip_set_collective(gbrl_hip_model *m, const gbrl_hip_collective *hooks);

/* Native exchange (preferred on multi-GPU nodes): the model creates its own RCCL communicator and enqueues every all-reduce
 * on its stream -- no host synchronisation at the exchange points.  RCCL is bound at run time (the librccl.so the process
 * already loaded, e.g. PyTorch's, else the system one).  Rank 0 calls gbrl_hip_rccl_unique_id and hands the 128 bytes to the
 * other ranks by any means (torch.distributed.broadcast in gbrl_amd/dist.py); then EVERY rank calls gbrl_hip_set_rccl
 * (a collective call: it returns when all ranks have joined).  Replaces hooks installed earlier; installing hooks later
 * destroys the communicator. */
int gbrl_hip_rccl_available(void);   /* 1 when an RCCL library could be bound in this process */
int gbrl_hip_rccl_unique_id(void *id128);
int gbrl_hip_set_rccl(gbrl_hip_model *m, const void *id128, int world_size, int rank);
/* The same with flags.  GBRL_HIP_RCCL_KEEP_WORLD1: keep the row-sharded code path (every exchange enqueued on the stream) at world size 1,
 * which gbrl_hip_set_rccl drops as "nothing to exchange" -- what bench.py's `collective` leg measures (the fixed cost of that path before a
 * byte crosses xGMI).  No reference counterpart (the reference has no collective). */
#define GBRL_HIP_RCCL_KEEP_WORLD1 1u
int gbrl_hip_set_rccl_flags(gbrl_hip_model *m, const void *id128, int world_size, int rank, unsigned flags);

/* ---- measurement -------------------------------------------------------------------------------------- */
/* ---- inspection, served from the host copy of the ensemble ---------------------- */
/* Linear TreeSHAP of one tree / of the whole ensemble: GBRL::tree_shap gbrl.cpp:1269-1303, GBRL::ensemble_shap gbrl.cpp:1305-1342,
 * algorithm shap.cpp:38-364.  Evaluated on the HIP device when one is usable (same bits as the host evaluation, which serves
 * machines without a GPU).  HOST pointers only (the reference's binding accepts NumPy arrays only, binding.cpp:985-1117).
 * obs [n_samples][n_num_features] f32, cat_obs [n_samples][n_cat_features][128] bytes (either may be NULL when the model has no
 * such features); norm_values [(max_depth+1)][max_depth], base_poly [max_depth], offset [max_depth][max_depth] as built by
 * gbrl/common/utils.py:317-371.  out [n_samples][n_num_features + n_cat_features][output_dim] is OVERWRITTEN
 * (left untouched by gbrl_hip_ensemble_shap when the ensemble has no trees: the feature counts are unknown until the first step). */
int gbrl_hip_tree_shap(const gbrl_hip_model *m, int tree_idx, const float *obs, const char *cat_obs, int n_samples,
                       const float *norm_values, const float *base_poly, const float *offset, float *out);
int gbrl_hip_ensemble_shap(const gbrl_hip_model *m, const float *obs, const char *cat_obs, int n_samples,
                           const float *norm_values, const float *base_poly, const float *offset, float *out);
/* GBRL::exportModel gbrl.cpp:1106-1128 (text: export_ensemble_data types.cpp:409-679).  export_format "float"|"fxp8"|"fxp16",
 * export_type "full"|"compact"; NULL strings mean the binding's defaults ("", "float", "full", "").  Oblivious models only. */
int gbrl_hip_export(const gbrl_hip_model *m, const char *filename, const char *modelname, const char *export_format,
                    const char *export_type, const char *prefix);
/* GBRL::print_tree gbrl.cpp:1357-1391 (tree_idx -1 = last tree) and GBRL::print_ensemble_metadata gbrl.cpp:1254-1267: the same
 * text, written to stdout.  device_name is what get_device() reports ("cpu" | "cuda"). */
int gbrl_hip_print_tree(const gbrl_hip_model *m, int tree_idx);
int gbrl_hip_print_ensemble_metadata(const gbrl_hip_model *m, const char *device_name);
/* GBRL::plot_tree gbrl.cpp:1409-1547 needs Graphviz, which this image does not have: always GBRL_HIP_E_UNSUPPORTED with the
 * message of the reference's own no-Graphviz build ("GBRL compiled without Graphviz! Cannot plot model"). */
int gbrl_hip_plot_tree(const gbrl_hip_model *m, int tree_idx, const char *filename);
/* what get_ensemble_data()["alloc_data_size"] shows in the reference: the size of the exact-size copy it hands out
 * (copy_ensemble_data types.cpp:322-384, binding.cpp:382) */
size_t gbrl_hip_alloc_data_size(const gbrl_hip_model *m);

/* Per-phase GPU time of the LAST step()/predict() call, measured with HIP events on the model's stream.
 * names/ms hold up to `cap` entries; returns the number of phases. */
int gbrl_hip_last_phase_times(const gbrl_hip_model *m, const char **names, float *ms, int cap);
/* level 0 (default): no events.  1: only the dominant kernel's launches (histogram build in step(), the traversal kernel in
 * predict()) are timed -- step(): the dispatch's own begin/end timestamps (hipExtLaunchKernelGGL events), free for a timed region.  2: every phase is bracketed
 * (diagnostic: each record costs a few microseconds of stream bubble, ~60 records per step). */
int gbrl_hip_set_profiling(gbrl_hip_model *m, int level);
/* Diagnostics (tests): the near-tie replay kernel (csrc/neartie.hip) on ONE node given explicitly -- the float32 score the reference's
 * TreeNode::splitScoreCosine / splitScoreL2 (node.cpp:187-251, 321-376) gives the split {rows with goes_right} | {the others} of the rows
 * with in_node set, and the node's parent score (scoreCosine / scoreL2, split_candidate_generator.cpp:262-320).  Host pointers: grads
 * [n_rows][output_dim]; in_node, goes_right [n_rows] bytes; meanden nullable [2 * output_dim] (L2: column means | std + 1e-8f, the
 * standardisation applied to grads before scoring); out_scores[2] = split score | parent score.  n_rows <= 65536. */
int gbrl_hip_replay_scores(const float *grads, const uint8_t *in_node, const uint8_t *goes_right, int n_rows, int output_dim,
                           const float *meanden, int cosine, int min_data_in_leaf, float *out_scores);

/* Diagnostics for the tests: sequential float32 sums -- s = start; for every element in order: s = (float)(s + x) -- of `n_chains` arrays stored
 * back to back in `x` (`lens[i]` elements each), evaluated by the parallel block-summary kernels of seqsum.hip; the results must equal the plain
 * loop bit for bit.  Host pointers; starts nullable (zeros); n_slow_blocks nullable: how many 256-element blocks took the serial fallback.
 * No reference counterpart (the reference IS the plain loop: node.cpp:336-352). */
int gbrl_hip_seq_sums(const float *x, const uint32_t *lens, const float *starts, int n_chains, float *out, uint32_t *n_slow_blocks);
/* Diagnostics for the tests: the same sums evaluated on the CPU by the arithmetic the kernels are compiled from (csrc/seqsum_core.h), walking
 * every chain as the kernels do -- exponent predicted from the fp64 prefix of the 256-element block sums plus the start, summaries composed
 * from single elements, 16 blocks under one exponent tried first, then block by block, then element by element.  No HIP call: it runs without
 * a device.  Arguments as above; n_fast_blocks nullable: how many blocks a summary applied (n_slow_blocks + n_fast_blocks = all blocks).
 * Nothing in the product calls it. */
int gbrl_hip_seq_sums_model(const float *x, const uint32_t *lens, const float *starts, int n_chains, float *out, uint32_t *n_slow_blocks,
                            uint32_t *n_fast_blocks);

/* Diagnostics for the tests: the ranking statistics of a batch's categorical cells as the device computes them when the batch holds more
 * distinct (feature, cell) pairs than n_cat * n_bins (cat_rank.hip).  Host pointers: cells [n][n_cat][128] bytes, grads [n][output_dim].
 * Per distinct pair, in no particular order: its feature, the first row that carries it, the number of rows that carry it and the float32
 * sum of those rows' squared gradient norms in ascending row order from 0.0f -- the operands of the reference's mean
 * (split_candidate_generator.cpp:119-137), bit for bit.  The four outputs hold `cap` entries; *n_distinct receives the number written.
 * GBRL_HIP_E_INVALID when cap is too small (then *n_distinct is left at -1). */
int gbrl_hip_cat_rank_stats(const char *cells, int n, int n_cat, const float *grads, int output_dim, int cap, int32_t *feature,
                            int32_t *first_row, int32_t *count, float *total, int *n_distinct);

/* Diagnostics for the tests: the launch plan of the device TreeSHAP kernel (csrc/shap.hip, kern::shap_block_threads) for a model with this
 * max_depth and output_dim.  *threads = threads per block (256 while the two coefficient stacks of every thread fit the LDS, then 128, then
 * 64), *samples_per_block = threads / output_dim; both 0 when the kernel declines the shape (the stacks fit no block size, or one sample's
 * outputs do not fit the block): tree_shap / ensemble_shap then evaluate on the host.  No HIP call: it runs without a device. */
int gbrl_hip_shap_plan(int max_depth, int output_dim, int *threads, int *samples_per_block);

/* Diagnostics for the tests: what a step with `n_classes` classes per feature (n_bins + 1, or the largest categorical class count + 1) and
 * `output_dim` outputs on `n_rows` rows does in its split-score histogram build (csrc/step_hist_build.hip).  fg_in = 0: fg is the engine's own
 * choice of features per block (kern::hist_feature_group); 1, 2, 4, 8 or 16: used as given.  The rest is the answer of the one rule every
 * launch goes through (hist_route), hooks GBRL_HIP_HIST_GENERIC and GBRL_HIP_HIST_PIPE read as a real call reads them:
 *   kind   0 the run-time-D kernel, 1 k_hist_build<D> (compile-time D), 2 k_hist_build_wide<2, H>, 3 k_hist_build_quad<R>
 *   param  kind 1: D;  kind 2: H = ceil((D + 1) / 2);  kind 3: R = ceil((D + 1) / 4);  kind 0: 0
 *   pipe   kind 1 only: the software-pipelined main loop
 *   direct_ok     a block may store its node's int64 histogram itself (every node one chunk)
 *   countless_ok  a build that leaves the count field out exists (the root's counts then come from root_le)
 *   hist_lds_bytes  the LDS tile of one block, n_classes * (output_dim + 1) * fg * 4; a step needs it to be at most 160 KiB - 512
 * No HIP call: it runs without a device.  Nothing in the product calls it. */
typedef struct gbrl_hip_hist_plan_t {
    int fg, kind, param, pipe, direct_ok, countless_ok;
    size_t hist_lds_bytes;
} gbrl_hip_hist_plan_t;
int gbrl_hip_hist_plan(int n_classes, int output_dim, int n_rows, int fg_in, gbrl_hip_hist_plan_t *plan);

/* Diagnostics for the tests: ONE histogram build on arrays given explicitly, and the reduce behind it -- the kernels of csrc/step_hist_build.hip
 * and csrc/step_hist_reduce.hip exactly as a step launches them.  Host pointers.  With Fp = n_feature_slots rounded up to a multiple of fg:
 *   codes   uint16 [ceil(Fp / 16)][n_rows][16]   the class of every (row, feature slot); every value below n_classes, padding included
 *   qg      int32  [n_rows][output_dim]          the quantised gradients
 *   rows    int32  [m]                           the row list (row indices, repeats allowed)
 *   chunks  int32  [n_chunks][3]                 (node, start, len): rows[start .. start + len) belong to `node`.  Nodes ascending; a node without
 *                                                rows has no entry (mode 0).  Entries with len = 0 may follow the last entry that has rows.
 *   mode    0: every chunk's int32 partial sums, then hist_reduce.  1: HistDirect -- entry i is ALL of node i (len 0 included, n_chunks = n_nodes)
 *              and the build stores the histograms; only where the plan says direct_ok.
 *   count_rows  0: the build without the count field (only where the plan says countless_ok)
 *   root_le     nullable uint32 [root_F][root_B], #{keys <= threshold}: the count of class c of a feature below root_F becomes
 *               le[c] - le[c-1] (class root_B: root_n - le[root_B-1]); only where the plan says countless_ok
 *   chunks_per_slot   below 48: one thread per element sums a node's chunks; from 48: four
 *   scatter_fs  > 0: hist is the send layout [ceil(Fp / fs)][n_nodes][fs][n_classes][output_dim + 1] of a reduce-scatter by feature
 *   slot_map    nullable int32 [n_nodes]: node k's histogram goes to slot slot_map[k] (distinct)
 *   hist        int64 [hist_elems]: [slots][Fp][n_classes][output_dim + 1] (field output_dim = the count), slots >= n_nodes or what slot_map
 *               names -- or the scatter layout.  Copied to the device before the kernels run and back afterwards: a cell that no kernel stored
 *               keeps the caller's value.  The partial sums start from a non-zero pattern.
 * Out, of the kernel that ran: kind, param, pipe (as gbrl_hip_hist_plan), counted (1: it accumulates the count field); and wrote_direct.
 * n_nodes <= 65535.
 * Everything is checked on the host before the first HIP call -- codes, row indices, chunk ranges, fg, the LDS tile, the modes against the plan,
 * slot_map, hist_elems against the layout: GBRL_HIP_E_INVALID, and no device is touched.  Nothing in the product calls it. */
typedef struct gbrl_hip_hist_probe_t {
    const uint16_t *codes;
    const int32_t *qg, *rows, *chunks;
    const uint32_t *root_le;
    const int32_t *slot_map;
    int64_t *hist;
    long long hist_elems, root_n;
    int n_rows, output_dim, m, n_chunks, n_nodes, n_feature_slots, fg, n_classes, mode, count_rows, root_F, root_B, chunks_per_slot, scatter_fs;
    int kind, param, pipe, counted, wrote_direct;
} gbrl_hip_hist_probe_t;
int gbrl_hip_hist_probe(gbrl_hip_hist_probe_t *args);

/* Diagnostics for the tests: what a tree level does with its histograms -- the kernels of csrc/step_score.hip through the launchers a step uses
 * (score_candidates, argmax, resolve_splits; the pinned publish path is not driven).  Host pointers.  With W = output_dim + 1:
 *   hist        int64 [n_hist_nodes][Fp][n_classes][W]   the level's histograms, IN and OUT (a derived node's slice is written back)
 *   hist_prev   nullable int64 [n_prev_nodes][Fp][n_classes][W]; sub_par / sub_sib nullable int32 [n_nodes]: sub_par[k] >= 0 makes node k
 *               hist_prev[sub_par[k]] - hist[sub_sib[k]] (sub_sib[k] < 0: the parent alone)
 *   hist_global nullable int64 [n_nodes][Fp][n_classes][W]: resolve_splits counts a second pair from it
 *   slots       int32 [n_table_slots][4] = (is_cat, n_cand, cand_base, 0);  thr float [n_table_slots][B];  thr_keys nullable uint32, the same shape
 *   path_len    int32 [n_nodes];  path_slot, path_bin int32 and path_val float [n_nodes][32]
 *   cand_w float, cand_ref, ref_to_internal, cand_slot int32 [n_cand];  is_root int32 [n_nodes];  seg_start nullable int32 [n_nodes]
 *   inv_scale = 2^-sbits;  slot0, n_slots: the slots launched;  keep_derived as score_candidates takes it
 * What runs:
 *   do_score   0: nothing;  1: scores mode -> scores, parent, cand_nr (nullable);  2: the fused greedy form -> parent, part_v, part_i and,
 *              where given, part_s, part_n, all [n_nodes][n_slots]
 *   do_argmax  1 (with do_score 0 or 1): k_argmax_stage1 in the oblivious form on `scores` -> part_v, part_i, part_s (nullable) [n_parts]
 *   do_resolve 1: resolve_splits on part_* (as left by the steps above, or as given) -> best_idx, best_score [max_front], counts4 int64
 *              [4][max_front], splits int32 [n_nodes][8] (NodeSplit), cursors int32 [n_nodes][2].  near != 0: the NearDetect fields
 *              (part_s, part_n, near_rel, parent, is_root, cosine, near_rows).  keep_derived = 0 hands it hist_prev, sub_par and sub_sib.
 *   n_parts    entries per node of part_*: n_slots after do_score 2, ceil(n_cand / 256) after do_argmax, free otherwise
 * Every array named as an output (and hist) goes to the device holding the caller's values and comes back afterwards: a cell no kernel
 * stored keeps them.  Everything a kernel will index is checked on the host first -- null arrays, sizes, the LDS tile
 * (n_classes + 2) * W * 8 <= 150 KiB, every slot's candidates inside [0, n_cand) and its classes inside n_classes, sub_par / sub_sib, path_len <= 32,
 * cand_ref a permutation, ref_to_internal and cand_slot, the launch window, given part_i: GBRL_HIP_E_INVALID with a text that names the
 * reason, and no device is touched.  Nothing in the product calls it. */
typedef struct gbrl_hip_score_probe_t {
    int64_t *hist;
    const int64_t *hist_prev, *hist_global;
    const int32_t *sub_par, *sub_sib, *slots;
    const float *thr;
    const uint32_t *thr_keys;
    const int32_t *path_len, *path_slot, *path_bin;
    const float *path_val, *cand_w;
    const int32_t *cand_ref, *ref_to_internal, *cand_slot, *is_root, *seg_start;
    float *scores, *parent, *part_v, *part_s, *best_score;
    int32_t *cand_nr, *part_i, *part_n, *best_idx, *splits, *cursors;
    int64_t *counts4;
    long long near_rows;
    float near_rel;
    int n_hist_nodes, n_prev_nodes, n_nodes, Fp, n_classes, output_dim, n_table_slots, B, n_cand, sbits, min_data, cosine, slot0, n_slots, keep_derived;
    int do_score, do_argmax, do_resolve, n_parts, oblivious, near, max_front;
} gbrl_hip_score_probe_t;
int gbrl_hip_score_probe(gbrl_hip_score_probe_t *args);

/* Diagnostics for the tests: ONE launch of a row kernel of csrc/step_partition.hip on host arrays.  op 0: partition_rows, 1: count_right,
 * 2: leaf_sums.
 *   rows     int32 [m] row indices (repeats allowed);  chunks int32 [n_chunks][3] = (slot, start, len), len <= 4096 for op 0
 *   codes    uint16 [ceil(n_feature_slots / 16)][n_rows][16] (ops 0, 1);  kt nullable uint32 [n_feature_slots][n_rows]: numeric splits read the keys
 *   splits   int32 [n_slots][8] (NodeSplit: do_split, fslot, bin, is_cat, seg_start, n_left, thr_key, 0) (ops 0, 1)
 *   grads    float [n_rows][output_dim], scaled by 2^lbits (op 2)
 *   rows_out int32 [m] and cursors int32 [n_slots][2] (op 0);  acc int64 [n_slots] (op 1: rows going right) or [n_slots][output_dim + 1] (op 2)
 * rows_out, cursors and acc go to the device holding the caller's values -- the kernels ADD to cursors and acc -- and come back afterwards.
 * Checked on the host first: null arrays, sizes, row indices, chunks inside the row list, every split's slot; for op 0 also that the segments
 * of the splitting nodes lie inside the list and apart, that their cursors start at 0, and that every n_left is the count the host itself
 * finds (a destination would leave the segment otherwise): GBRL_HIP_E_INVALID, and no device is touched.  Nothing in the product calls it. */
typedef struct gbrl_hip_rows_probe_t {
    const int32_t *rows, *chunks, *splits;
    const uint16_t *codes;
    const uint32_t *kt;
    const float *grads;
    int32_t *rows_out, *cursors;
    int64_t *acc;
    int op, n_rows, m, n_chunks, n_slots, n_feature_slots, output_dim, lbits;
} gbrl_hip_rows_probe_t;
int gbrl_hip_rows_probe(gbrl_hip_rows_probe_t *args);

/* ---- device / stream contract (new; the reference pins everything to device 0 and the null stream, cuda_types.cu:32-106) -- */
/* The device the model computes on: the ordinal given at creation, or -- for -1 -- the calling thread's current device at the
 * first call that needs it (it is latched by this call too).  -1 when no HIP device is usable.  A caller that hands out
 * predict results as device buffers must allocate them on THIS device (gbrl_hip_device_alloc_on) and label them with it. */
int gbrl_hip_device_ordinal(gbrl_hip_model *m);
/* Stream ordering.  By default the model owns a BLOCKING stream: its work is ordered with the legacy null stream only, so a
 * caller that runs on a non-default (or per-thread default) stream must either synchronise that stream around step()/predict()
 * or hand it over here: with a non-null `hip_stream` (a hipStream_t of the model's device) every kernel, copy and collective
 * of this model is enqueued on it -- inputs produced on that stream and outputs consumed on it need no further
 * synchronisation.  step()/predict() still return after their own work has completed (they read results back).  NULL
 * restores the model's own stream. */
int gbrl_hip_set_stream(gbrl_hip_model *m, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GBRL_HIP_H */
