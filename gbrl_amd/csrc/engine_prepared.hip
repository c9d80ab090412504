// engine_prepared.hip -- a batch binned once and stepped on many times (see engine.h, PreparedDataset):
//   Engine::prepare_dataset   the numeric preparation of step() (Engine::prepare_numeric, engine_step.hip: key transpose, thresholds, class codes,
//                             the fused kern::small_prep with want_stats = false) into buffers the data set owns
//   Engine::prepare_dataset_like   a data set bound to another one's thresholds: kern::bin_like on the new rows, copies of the thresholds
//   Engine::step_prepared     gradient statistics (Engine::run_grad_stats), the GrowCtx from the data set, grow_tree, append_tree -- no transpose,
//                             no candidates, no binning.  A row subset gathers the subset's 32-byte code records (kern::gather_code_records) into
//                             the engine's workspace and grows on them with the DATA SET'S thresholds; keys, feature-major codes and the root's
//                             count table are handed over as null there (legal inputs of every growth path: the partition then reads the
//                             codes, the root histogram counts its rows).
//                             A column subset (cols) gathers the subset's columns of those records -- rows and columns in one pass,
//                             kern::gather_code_columns -- and the subset's thresholds and keys, grows on F' = n_cols features with the full
//                             step's candidate weights and rewrites the conditions' feature indices through cols before the tree is appended.
//   PreparedDataset::codes_to_host   the codes on the host, all rows or a gathered subset of rows and / or columns
//   Engine::sample_rows_host / sample_rows / sample_gather   the row sampler of sample_core.h: the rule on the host, kern::sample_rows on a data
//                             set's row range, and with the gathered rows of a matrix (what fit_prepared's sampled iterations enqueue)
//   Engine::goss_rows_host / sample_goss   one-side sampling of sample_core.h: the rule on the host, kern::sample_goss on a data set's row range
// None of the growth kernels is touched: integer histograms do not depend on which of the optional buffers a path reads.
#include "engine_step_detail.h"
#include "sample_core.h"

#include <limits>
#include <memory>

namespace gbrl {

// numeric-only, one GPU: categorical candidates depend on the step's gradients, sharded thresholds need the exchange
void Engine::check_prepared_model(const char *what) const {
    const gbrl_hip_metadata &md = model.meta;
    if (has_coll_ || rccl_comm_ != nullptr)
        throw Unsupported(std::string(what) + ": not available on a model with a communicator or collective hooks (the thresholds of a row-sharded batch need the exchange)");
    if (md.iteration > 0 && md.n_cat_features > 0)
        throw Unsupported(std::string(what) + ": not available on a model with categorical columns (their split candidates depend on the step's gradients)");
}

namespace {
uint64_t next_dataset_id() {
    static std::atomic<uint64_t> next_id{1};
    return next_id.fetch_add(1, std::memory_order_relaxed);
}
}  // namespace

// A data set bound to `ref`'s thresholds: the codes of obs under them (kern::bin_like), own copies of the thresholds, their keys and the host
// thresholds.  No keys, no feature-major codes, no root table: the growth paths take them as null (step_prepared_run).
PreparedDataset *Engine::prepare_dataset_like(const PreparedDataset *ref, const float *obs, bool obs_dev, int n) {
    check_prepared_dataset("prepare_dataset", ref);
    if (n <= 0 || obs == nullptr) throw InvalidArgument("Cannot call prepare_dataset without obs!");
    ensure_device();
    ev_used_ = 0;
    ev_names_.clear();
    hipStream_t s = stream_;
    const int N = n, F = ref->F, B = ref->n_bins;
    std::unique_ptr<PreparedDataset> ds(new PreparedDataset());
    ds->n = N; ds->F = F; ds->n_bins = B; ds->generator_type = ref->generator_type; ds->device = device_ordinal_;
    ds->id = next_dataset_id();
    ds->thresholds_id = ref->thresholds_id;
    ds->h_thr = ref->h_thr;
    phase_begin();
    const float *dobs = obs;
    if (!obs_dev) {
        dobs = static_cast<float *>(d_obs_.ensure(sizeof(float) * static_cast<size_t>(N) * F));
        hip_check(hipMemcpyAsync(const_cast<float *>(dobs), obs, sizeof(float) * static_cast<size_t>(N) * F, hipMemcpyHostToDevice, s), "H2D obs");
    }
    const size_t n_thr = static_cast<size_t>(F) * B;
    float *d_thr = static_cast<float *>(ds->buf.thr.ensure(sizeof(float) * n_thr));
    uint32_t *d_thrkeys = static_cast<uint32_t *>(ds->buf.thrkeys.ensure(sizeof(uint32_t) * n_thr));
    hip_check(hipMemcpyAsync(d_thr, ref->prep.d_thr, sizeof(float) * n_thr, hipMemcpyDeviceToDevice, s), "D2D thr");
    hip_check(hipMemcpyAsync(d_thrkeys, ref->prep.d_thrkeys, sizeof(uint32_t) * n_thr, hipMemcpyDeviceToDevice, s), "D2D thr keys");
    phase_end("inputs"); phase_begin(/*key=*/true);
    const size_t G = static_cast<size_t>(ds->code_groups());
    uint16_t *d_codes = static_cast<uint16_t *>(ds->buf.codes.ensure(sizeof(uint16_t) * G * N * kern::kCodeGroup));
    kern::bin_like(dobs, N, F, d_thrkeys, B, d_codes, s);
    hip_check(hipGetLastError(), "bin_like launch");
    phase_end("bin_like", /*key=*/true);
    hip_check(hipStreamSynchronize(s), "sync");   // the caller's obs and the reference are not needed from here on
    phases_resolve();
    ds->prep.d_thr = d_thr; ds->prep.d_thrkeys = d_thrkeys; ds->prep.d_codes = d_codes;
    return ds.release();
}

PreparedDataset *Engine::prepare_dataset(const float *obs, bool obs_dev, int n, int n_num) {
    const gbrl_hip_metadata &md = model.meta;
    check_prepared_model("prepare_dataset");
    if (md.iteration > 0 && n_num != md.n_num_features) throw InvalidArgument("Incompatible dataset");
    if (n_num != md.input_dim) throw InvalidArgument("Total number of features != correct input dim");
    if (n <= 0 || n_num <= 0 || obs == nullptr) throw InvalidArgument("Cannot call prepare_dataset without obs!");
    if (md.max_depth > kern::kMaxPath) throw Unsupported("max_depth > 32 is not supported");
    if (md.n_bins < 1 || md.n_bins > 65534) throw Unsupported("n_bins must be in [1, 65534]");
    if ((n_num + kern::kCodeGroup - 1) / kern::kCodeGroup > 65535) throw Unsupported("prepare_dataset: more than 65535 groups of 16 features");
    ensure_device();
    prof_step_entry_ = std::chrono::steady_clock::now();
    ev_used_ = 0;
    ev_names_.clear();
    exch_bytes_ = 0;
    exch_calls_ = 0;
    read_step_hooks();
    hipStream_t s = stream_;
    const int N = n, F = n_num, B = md.n_bins;
    std::unique_ptr<PreparedDataset> ds(new PreparedDataset());
    ds->n = N; ds->F = F; ds->n_bins = B; ds->generator_type = md.generator_type; ds->device = device_ordinal_;
    ds->id = ds->thresholds_id = next_dataset_id();
    phase_begin();
    const float *dobs = obs;
    if (!obs_dev) {
        dobs = static_cast<float *>(d_obs_.ensure(sizeof(float) * N * F));
        hip_check(hipMemcpyAsync(const_cast<float *>(dobs), obs, sizeof(float) * N * F, hipMemcpyHostToDevice, s), "H2D obs");
    }
    phase_end("inputs");
    prof_marks_[0] = std::chrono::steady_clock::now();
    ds->prep = prepare_numeric(ds->buf, dobs, N, F, 0, N, fused_prep_applies(N, F, N), nullptr);
    ds->h_thr.resize(static_cast<size_t>(F) * B);
    hip_check(hipMemcpyAsync(ds->h_thr.data(), ds->prep.d_thr, sizeof(float) * ds->h_thr.size(), hipMemcpyDeviceToHost, s), "D2H thr");
    hip_check(hipStreamSynchronize(s), "sync");   // the caller's obs is not needed from here on
    hip_check(hipGetLastError(), "prepare_dataset kernels");
    phases_resolve();
    return ds.release();
}

namespace detail {
const int32_t *checked_rows(DevBuf &copy, DevBuf &mm_buf, const int32_t *rows, bool rows_dev, int m, int n, hipStream_t s) {
    if (!rows_dev) {
        int32_t *d = static_cast<int32_t *>(copy.ensure(sizeof(int32_t) * static_cast<size_t>(m)));
        hip_check(hipMemcpyAsync(d, rows, sizeof(int32_t) * static_cast<size_t>(m), hipMemcpyHostToDevice, s), "H2D rows");
        return d;
    }
    int32_t *d_mm = static_cast<int32_t *>(mm_buf.ensure(2 * sizeof(int32_t)));
    kern::rows_minmax(rows, m, d_mm, s);
    int32_t mm[2] = {0, 0};
    hip_check(hipMemcpyAsync(mm, d_mm, sizeof(mm), hipMemcpyDeviceToHost, s), "D2H rows min/max");
    hip_check(hipStreamSynchronize(s), "sync");
    const int lo = mm[0], hi = ~mm[1];
    if (lo < 0 || hi >= n)
        throw InvalidArgument("rows: index " + std::to_string(lo < 0 ? lo : hi) + " is outside [0, " + std::to_string(n) + ")");
    return rows;
}
void check_row_count(const char *what, const char *noun, const int32_t *rows, int m, int n, const char *verb) {
    if (m <= 0) throw InvalidArgument(std::string(what) + ": no rows (m must be positive)");
    if (rows == nullptr && m != n)
        throw InvalidArgument(std::string(what) + ": " + noun + " has " + std::to_string(m) + " rows, the data set " + std::to_string(n) + " (pass rows to " + verb + " a subset)");
}
void check_host_rows(const int32_t *rows, int m, int n) {
    for (int j = 0; j < m; ++j)
        if (rows[j] < 0 || rows[j] >= n)
            throw InvalidArgument("rows: index " + std::to_string(rows[j]) + " (entry " + std::to_string(j) + ") is outside [0, " + std::to_string(n) + ")");
}
}  // namespace detail

// the data set is there and is this model's (step_prepared's checks; `what` prefixes the messages)
void Engine::check_prepared_dataset(const char *what, const PreparedDataset *ds) const {
    const gbrl_hip_metadata &md = model.meta;
    const std::string w(what);
    if (ds == nullptr) throw InvalidArgument(w + ": null data set");
    check_prepared_model(what);
    {
        int dev = device_ordinal_;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = -1;   // (an unlatched model runs on the calling thread's current device)
        if (dev >= 0 && dev != ds->device)
            throw Unsupported(w + ": the data set lives on device " + std::to_string(ds->device) + ", the model on device " + std::to_string(dev));
    }
    if (ds->n_bins != md.n_bins) throw InvalidArgument(w + ": the data set was binned with n_bins = " + std::to_string(ds->n_bins) + ", the model has " + std::to_string(md.n_bins));
    if (ds->generator_type != md.generator_type) throw InvalidArgument(w + ": the data set's generator_type differs from the model's");
    if (ds->F != md.input_dim) throw InvalidArgument("Total number of features != correct input dim");
    if (md.iteration > 0 && ds->F != md.n_num_features) throw InvalidArgument("Incompatible dataset");
}

void Engine::begin_step_profile() {
    prof_step_entry_ = std::chrono::steady_clock::now();
    ev_used_ = 0;
    ev_names_.clear();
    exch_bytes_ = 0;
    exch_calls_ = 0;
}

void Engine::check_cols(const char *what, const int32_t *cols, int n_cols, int F) {
    const std::string w(what);
    if (n_cols < 1 || n_cols > F) throw InvalidArgument(w + ": cols must name between 1 and " + std::to_string(F) + " columns, got " + std::to_string(n_cols));
    for (int i = 0; i < n_cols; ++i) {
        if (cols[i] < 0 || cols[i] >= F)
            throw InvalidArgument(w + ": cols: index " + std::to_string(cols[i]) + " (entry " + std::to_string(i) + ") is outside [0, " + std::to_string(F) + ")");
        if (i > 0 && cols[i] <= cols[i - 1])
            throw InvalidArgument(w + ": cols must be strictly ascending (entry " + std::to_string(i) + " is " + std::to_string(cols[i]) + " after " + std::to_string(cols[i - 1]) + ")");
    }
}

void Engine::step_prepared(const PreparedDataset *ds, const float *grads, bool grads_dev, const int32_t *rows, bool rows_dev, int m, const int32_t *cols, int n_cols) {
    gbrl_hip_metadata &md = model.meta;
    check_prepared_dataset("step_prepared", ds);
    if (grads == nullptr) throw InvalidArgument("Cannot call step without grads!");
    check_row_count("step_prepared", "grads", rows, m, ds->n, "step on");
    if (md.max_depth > kern::kMaxPath) throw Unsupported("max_depth > 32 is not supported");
    if (md.n_bins < 1 || md.n_bins > 65534) throw Unsupported("n_bins must be in [1, 65534]");
    if (md.output_dim > 512) throw Unsupported("output_dim > 512");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, ds->n);
    if (cols != nullptr) {
        check_cols("step_prepared", cols, n_cols, ds->F);
        if (n_cols == ds->F) cols = nullptr;   // every column, in order: the call without cols
    }
    ensure_device();
    begin_step_profile();
    hipStream_t s = stream_;
    const int N = m, D = md.output_dim;
    // ---- inputs on the device ---------------------------------------------------------------------------------
    phase_begin();
    const float *dgrads = grads;
    if (!grads_dev) {
        dgrads = static_cast<float *>(d_grads_.ensure(sizeof(float) * N * D));
        hip_check(hipMemcpyAsync(const_cast<float *>(dgrads), grads, sizeof(float) * N * D, hipMemcpyHostToDevice, s), "H2D grads");
    }
    const int32_t *d_rows = subset_rows(ds, rows, rows_dev, m);
    phase_end("inputs");
    step_prepared_run(ds, dgrads, d_rows, m, cols, n_cols);
}

// One boosting step on device inputs that have been checked (fit_prepared's loop body too): the phase list is the caller's (begin_step_profile).
// cols (host, checked, a proper subset; null: every column): the step grows on those columns.
void Engine::step_prepared_run(const PreparedDataset *ds, const float *dgrads, const int32_t *d_rows, int m, const int32_t *cols, int n_cols) {
    gbrl_hip_metadata &md = model.meta;
    // GBRL::step, gbrl.cpp:946-958 (the latch is taken back when the step fails: the model is unchanged after any failure)
    const int32_t keep_num = md.n_num_features, keep_cat = md.n_cat_features;
    if (md.iteration == 0) { md.n_num_features = ds->F; md.n_cat_features = 0; }
    try {
        hipStream_t s = stream_;
        const int N = m, F = cols ? n_cols : ds->F, D = md.output_dim;
        const bool cosine = md.split_score_func == GBRL_HIP_SCORE_COSINE;
        long long n_global = N;
        prof_marks_[0] = std::chrono::steady_clock::now();
        // ---- 1. gradient statistics and quantisation (A2) ----------------------------------------------------------
        phase_begin();
        float *d_meanden = static_cast<float *>(d_meanden_.ensure(sizeof(float) * 2 * D));
        double *d_stat = static_cast<double *>(d_stat_.ensure(sizeof(double) * 4 * D));
        kern::StepScales *d_scales = static_cast<kern::StepScales *>(d_scales_.ensure(sizeof(kern::StepScales)));
        int32_t *d_qg = static_cast<int32_t *>(d_qg_.ensure(sizeof(int32_t) * static_cast<size_t>(N) * D));
        const bool no_small_stats = [] { const char *e = hooks::raw(hooks::NO_SMALL_STATS); return e && e[0] == '1'; }();   /* read per call: the tests flip it */
        FusedStats gs{dgrads, D, cosine, d_stat, d_meanden, d_scales, d_qg, chunk_rows_of(n_global), !no_small_stats};
        run_grad_stats(gs, N, n_global);
        phase_end("grad_stats");
        // ---- the subset's code records (the thresholds stay the data set's) ---------------------------------------
        NumericPrep np = ds->prep;
        if (cols) {
            // rows and columns in one pass over the codes; the subset's rows of the threshold table and of its keys beside them
            phase_begin();
            const kern::GatherColsPlan plan = kern::gather_cols_plan(cols, n_cols, cols_plan_host_);
            const int32_t *d_plan = upload(d_cols_plan_, cols_plan_host_.data(), plan.n_words, "H2D column plan");
            const size_t n_thr = static_cast<size_t>(n_cols) * ds->n_bins;
            uint16_t *sub = static_cast<uint16_t *>(prep_ws_.codes.ensure(sizeof(uint16_t) * static_cast<size_t>(plan.n_out_groups) * N * kern::kCodeGroup));
            float *thr = static_cast<float *>(prep_ws_.thr.ensure(sizeof(float) * n_thr));
            uint32_t *thrkeys = static_cast<uint32_t *>(prep_ws_.thrkeys.ensure(sizeof(uint32_t) * n_thr));
            kern::gather_code_columns(ds->prep.d_codes, ds->n, d_rows, N, d_plan, plan, sub, s);
            kern::gather_threshold_rows(ds->prep.d_thr, ds->prep.d_thrkeys, ds->n_bins, d_plan, plan, thr, thrkeys, s);
            phase_end("gather_cols");
            np = NumericPrep{};
            np.d_codes = sub; np.d_thr = thr; np.d_thrkeys = thrkeys;
        } else if (d_rows) {
            phase_begin();
            const int G = ds->code_groups();
            uint16_t *sub = static_cast<uint16_t *>(prep_ws_.codes.ensure(sizeof(uint16_t) * static_cast<size_t>(G) * N * kern::kCodeGroup));
            kern::gather_code_records(ds->prep.d_codes, ds->n, G, d_rows, N, sub, s);
            phase_end("gather_codes");
            np.d_codes = sub;
            np.d_kt = nullptr; np.d_codes_fm = nullptr; np.root_le = nullptr;
        }
        prof_marks_[1] = prof_marks_[2] = std::chrono::steady_clock::now();
        prep_launches_ = 0;
        // ---- feature slots, candidate order, weights, growth, leaf sums ------------------------------------------
        const std::vector<CatCandidate> cat_cands;
        const std::vector<int> cat_classes;
        StepData sd{};
        sd.N = N; sd.F = F; sd.Fc = 0; sd.n_global = n_global; sd.chunk_rows = gs.chunk_rows; sd.prep = np; sd.stats = &gs;
        sd.cat_cands = &cat_cands; sd.cat_classes = &cat_classes; sd.cols = cols;
        std::vector<HNode> nodes;
        std::vector<int> frontier;
        std::vector<int64_t> acc;
        double leaf_scale = 1.0;
        grow_step_tree(sd, nodes, frontier, acc, leaf_scale);
        hip_check(hipGetLastError(), "step kernels");
        if (cols)   // the tree names the data set's columns
            for (HNode &nd : nodes)
                for (HCond &c : nd.path) c.feat_idx = cols[c.feat_idx];
        append_tree(model, nodes, frontier, acc, leaf_scale, cat_cands);
        phases_resolve();
    } catch (...) {
        if (md.iteration == 0) { md.n_num_features = keep_num; md.n_cat_features = keep_cat; }
        throw;
    }
}

namespace {
struct DeviceScope {   // a data set's device for one call, the caller's afterwards
    int prev = -1;
    explicit DeviceScope(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; hip_check(hipSetDevice(dev), "hipSetDevice"); }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace

void PreparedDataset::codes_to_host(const int32_t *rows, bool rows_dev, int m, uint16_t *out, const int32_t *cols, int n_cols) const {
    if (out == nullptr) throw InvalidArgument("dataset_codes: no place for the codes");
    if (rows == nullptr) m = n;
    if (m <= 0) throw InvalidArgument("dataset_codes: no rows (m must be positive)");
    if (rows != nullptr && !rows_dev) check_host_rows(rows, m, n);
    if (cols != nullptr) Engine::check_cols("dataset_codes", cols, n_cols, F);
    DeviceScope scope(device);
    hipStream_t s = nullptr;
    const int G = cols ? (n_cols + kern::kCodeGroup - 1) / kern::kCodeGroup : code_groups();
    const size_t bytes = sizeof(uint16_t) * static_cast<size_t>(G) * m * kern::kCodeGroup;
    const uint16_t *src = prep.d_codes;
    DevBuf sub, rows_copy, mm, plan_buf;
    std::vector<int32_t> plan_words;   // (alive until the wait below)
    if (cols != nullptr) {
        const int32_t *d_rows = rows ? checked_rows(rows_copy, mm, rows, rows_dev, m, n, s) : nullptr;
        const kern::GatherColsPlan plan = kern::gather_cols_plan(cols, n_cols, plan_words);
        int32_t *d_plan = static_cast<int32_t *>(plan_buf.ensure(sizeof(int32_t) * plan.n_words));
        hip_check(hipMemcpyAsync(d_plan, plan_words.data(), sizeof(int32_t) * plan.n_words, hipMemcpyHostToDevice, s), "H2D column plan");
        uint16_t *dst = static_cast<uint16_t *>(sub.ensure(bytes));
        kern::gather_code_columns(prep.d_codes, n, d_rows, m, d_plan, plan, dst, s);
        hip_check(hipGetLastError(), "gather_code_columns launch");
        src = dst;
    } else if (rows != nullptr) {
        const int32_t *d_rows = checked_rows(rows_copy, mm, rows, rows_dev, m, n, s);
        uint16_t *dst = static_cast<uint16_t *>(sub.ensure(bytes));
        kern::gather_code_records(prep.d_codes, n, G, d_rows, m, dst, s);
        hip_check(hipGetLastError(), "gather_code_records launch");
        src = dst;
    }
    hip_check(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, s), "D2H codes");
    hip_check(hipStreamSynchronize(s), "sync");
}

// ---- the row sampler (sample_core.h) on a row range: the host rule, the device kernels on a data set, the fused gather of fit_prepared's loop
void Engine::check_subsample(const char *what, double subsample) {
    if (!kern::sample_fraction_ok(subsample))
        throw InvalidArgument(std::string(what) + ": subsample must be in [2^-24, 1] (and not NaN), got " + std::to_string(subsample));
}

namespace {
void check_sample_range(const char *what, int row0, int n, double subsample, int draw, const void *out, const int *count) {
    const std::string w(what);
    if (out == nullptr || count == nullptr) throw InvalidArgument(w + ": null output");
    if (row0 < 0) throw InvalidArgument(w + ": row0 must be >= 0");
    if (n <= 0) throw InvalidArgument(w + ": no rows (n must be positive)");
    if (draw < 0) throw InvalidArgument(w + ": draw must be >= 0");
    Engine::check_subsample(what, subsample);
    if (row0 > std::numeric_limits<int32_t>::max() - (n - 1)) throw InvalidArgument(w + ": the range ends above row 2^31 - 1");
}
}  // namespace

void Engine::check_colsample(const char *what, double colsample) {
    if (!kern::sample_cols_fraction_ok(colsample))
        throw InvalidArgument(std::string(what) + ": colsample must be in (0, 1] (and not NaN), got " + std::to_string(colsample));
}

void Engine::sample_cols_host(int F, double colsample, uint64_t seed, int draw, int32_t *out, int *count) {
    if (out == nullptr || count == nullptr) throw InvalidArgument("sample_cols_host: null output");
    if (F < 1) throw InvalidArgument("sample_cols_host: no columns (F must be positive)");
    if (draw < 0) throw InvalidArgument("sample_cols_host: draw must be >= 0");
    check_colsample("sample_cols_host", colsample);
    std::vector<int32_t> cols;
    kern::sample_cols(F, colsample, seed, draw, cols);
    std::copy(cols.begin(), cols.end(), out);
    *count = static_cast<int>(cols.size());
}

void Engine::sample_rows_host(int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out, int *count) {
    check_sample_range("sample_rows_host", row0, n, subsample, draw, out, count);
    const uint32_t thr = kern::sample_threshold(subsample);
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t row = static_cast<uint32_t>(row0) + static_cast<uint32_t>(i);
        if (kern::sample_keeps(seed, draw, row, thr)) out[m++] = static_cast<int32_t>(row);
    }
    *count = m;
}

void Engine::sample_gather(int row0, int n, double subsample, uint64_t seed, int draw, const float *G, int D, int32_t *rows_out, float *G_out, int *count) {
    check_sample_range("sample_gather", row0, n, subsample, draw, rows_out, count);
    if ((G == nullptr) != (G_out == nullptr)) throw InvalidArgument("sample_gather: G and G_out go together");
    if (G != nullptr && (D < 1 || D > 512)) throw InvalidArgument("sample_gather: D must be in [1, 512]");
    hipStream_t s = nullptr;
    DevBuf scratch;
    int32_t *d_scratch = static_cast<int32_t *>(scratch.ensure(sizeof(int32_t) * (static_cast<size_t>(kern::sample_rows_blocks(n)) + 1)));
    kern::sample_rows(row0, n, kern::sample_threshold(subsample), seed, draw, G, D, rows_out, G_out, d_scratch, s);
    hip_check(hipGetLastError(), "sample_rows launch");
    int32_t m = 0;
    hip_check(hipMemcpyAsync(&m, d_scratch, sizeof(m), hipMemcpyDeviceToHost, s), "D2H sample count");
    hip_check(hipStreamSynchronize(s), "sync");
    *count = m;
}

// ---- one-side sampling (sample_core.h): the checks, the rule on the host, the device kernels on a data set's rows
void Engine::check_goss(const char *what, double a, double b) {
    if (!kern::goss_rates_ok(a, b))
        throw InvalidArgument(std::string(what) + ": goss needs top_rate in [0, 1), other_rate in (0, 1], top_rate + other_rate <= 1 and other_rate / (1 - top_rate) >= 2^-24 "
                              "(and no NaN), got (" + std::to_string(a) + ", " + std::to_string(b) + ")");
}

void Engine::goss_rows_host(const float *G, int D, int row0, int n, double a, double b, uint64_t seed, int draw, int32_t *rows_out, float *factor_out, float *G_out,
                            int *count) {
    if (factor_out == nullptr) throw InvalidArgument("goss_rows_host: null output");
    check_sample_range("goss_rows_host", row0, n, 1.0, draw, rows_out, count);
    check_goss("goss_rows_host", a, b);
    if (G == nullptr) throw InvalidArgument("goss_rows_host: no gradients");
    if (D < 1 || D > 512) throw InvalidArgument("goss_rows_host: D must be in [1, 512]");
    *count = kern::goss_rows(G, D, row0, n, a, b, seed, draw, rows_out, factor_out, G_out, nullptr, nullptr);
}

void Engine::sample_goss(const PreparedDataset *ds, const float *G, int D, int row0, int n, double a, double b, uint64_t seed, int draw, int32_t *rows_out,
                         float *factor_out, float *G_out, bool io_dev, int *count, int *n_top, uint32_t *tau_bits) {
    if (ds == nullptr) throw InvalidArgument("sample_goss: null data set");
    if (factor_out == nullptr || G_out == nullptr) throw InvalidArgument("sample_goss: null output");
    check_sample_range("sample_goss", row0, n, 1.0, draw, rows_out, count);
    check_goss("sample_goss", a, b);
    if (G == nullptr) throw InvalidArgument("sample_goss: no gradients");
    if (D < 1 || D > 512) throw InvalidArgument("sample_goss: D must be in [1, 512]");
    if (row0 >= ds->n || n > ds->n - row0)
        throw InvalidArgument("sample_goss: rows [" + std::to_string(row0) + ", " + std::to_string(static_cast<long long>(row0) + n) + ") are outside [0, " + std::to_string(ds->n) + ")");
    DeviceScope scope(ds->device);
    hipStream_t s = nullptr;
    const size_t n_el = static_cast<size_t>(n) * D;
    DevBuf scratch, g_in, rows, factor, g_out;
    const kern::GossScratch gs = kern::goss_scratch(static_cast<int32_t *>(scratch.ensure(sizeof(int32_t) * kern::goss_scratch_words(n))), n);
    const float *dG = G;
    int32_t *d_rows = rows_out;
    float *d_factor = factor_out, *d_gout = G_out;
    if (!io_dev) {
        float *up = static_cast<float *>(g_in.ensure(sizeof(float) * n_el));
        hip_check(hipMemcpyAsync(up, G, sizeof(float) * n_el, hipMemcpyHostToDevice, s), "H2D gradients");
        dG = up;
        d_rows = static_cast<int32_t *>(rows.ensure(sizeof(int32_t) * static_cast<size_t>(n)));
        d_factor = static_cast<float *>(factor.ensure(sizeof(float) * static_cast<size_t>(n)));
        d_gout = static_cast<float *>(g_out.ensure(sizeof(float) * n_el));
    }
    const kern::GossPlan plan = kern::goss_plan(n, a, b);
    kern::sample_goss(row0, n, plan.k, plan.thr, plan.amp, seed, draw, dG, D, d_rows, d_factor, d_gout, nullptr, nullptr, gs, s);
    hip_check(hipGetLastError(), "sample_goss launch");
    int32_t h[6] = {0, 0, 0, 0, 0, 0};   // m, all ties, then the selection's state
    hip_check(hipMemcpyAsync(h, gs.m_out, sizeof(h), hipMemcpyDeviceToHost, s), "D2H sample count");
    hip_check(hipStreamSynchronize(s), "sync");
    const size_t m = static_cast<size_t>(h[0]);
    if (!io_dev && m > 0) {
        hip_check(hipMemcpy(rows_out, d_rows, sizeof(int32_t) * m, hipMemcpyDeviceToHost), "D2H sampled rows");
        hip_check(hipMemcpy(factor_out, d_factor, sizeof(float) * m, hipMemcpyDeviceToHost), "D2H factors");
        hip_check(hipMemcpy(G_out, d_gout, sizeof(float) * m * D, hipMemcpyDeviceToHost), "D2H sampled gradients");
    }
    *count = h[0];
    if (n_top) *n_top = plan.k;
    if (tau_bits) *tau_bits = static_cast<uint32_t>(h[2]);
}

void Engine::sample_rows(const PreparedDataset *ds, int row0, int n, double subsample, uint64_t seed, int draw, int32_t *out, bool out_dev, int *count) {
    if (ds == nullptr) throw InvalidArgument("sample_rows: null data set");
    check_sample_range("sample_rows", row0, n, subsample, draw, out, count);
    if (row0 >= ds->n || n > ds->n - row0)
        throw InvalidArgument("sample_rows: rows [" + std::to_string(row0) + ", " + std::to_string(static_cast<long long>(row0) + n) + ") are outside [0, " + std::to_string(ds->n) + ")");
    DeviceScope scope(ds->device);
    DevBuf rows;
    int32_t *d_rows = out_dev ? out : static_cast<int32_t *>(rows.ensure(sizeof(int32_t) * static_cast<size_t>(n)));
    int m = 0;
    sample_gather(row0, n, subsample, seed, draw, nullptr, 0, d_rows, nullptr, &m);
    if (!out_dev && m > 0) hip_check(hipMemcpy(out, d_rows, sizeof(int32_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost), "D2H sampled rows");
    *count = m;
}

}  // namespace gbrl
