// engine_step.hip -- host orchestration of the HIP kernels for GBRL::step and GBRL::fit (see engine.h).
//
// step() restates Fitter::step_cpu (gbrl/src/cpp/fitter.cpp:50-115) as a histogram algorithm:
//   1. gradient statistics + fixed-point quantisation of the build gradients           (A2)
//   2. split candidates: uniform (min/max) or quantile (exact order statistics)          (A3, A4); categorical on the host (A5)
//   3. observations -> per-feature class codes (once per step)
//   4. level-synchronous growth: for every frontier node build (count, sum g[D]) per (feature, class) in LDS, reduce to
//      exact int64 histograms, score every candidate from suffix sums, pick the split, partition the row list   (A6-A10)
//   5. leaf values = exact mean of the raw gradients per leaf                              (A11)
// The reference grows greedy trees depth-first; the split chosen for a node depends only on that node's rows, so growing
// level by level and emitting the leaves in depth-first (left first) order afterwards gives the identical tree.
#include "engine_step_detail.h"

namespace gbrl {

namespace detail {

// ---- A10/A11: the grown tree joins the ensemble (update_ensemble_per_leaf / per_tree, fitter.cpp:493-542) with exact leaf
// means of the raw gradients (acc[node] = int64 fixed-point sums | count; fitter.cpp:545-582).
void append_tree(Model &model, const std::vector<HNode> &nodes, const std::vector<int> &frontier, const std::vector<int64_t> &acc,
                 double leaf_scale, const std::vector<CatCandidate> &cat_cands) {
    gbrl_hip_metadata &md = model.meta;
    const bool oblivious = model.oblivious();
    const int MD = md.max_depth, D = md.output_dim;
// leaf order: oblivious = level order of the last level (child slots 2k, 2k+1, fitter.cpp:469-470); greedy = depth-first,
// left first (fitter.cpp:364-365)
std::vector<int> leaf_order;
if (oblivious) {
    if (nodes.size() == 1) leaf_order.push_back(0);
    else leaf_order = frontier;
} else {
    std::vector<int> stack{0};
    while (!stack.empty()) {
        const int id = stack.back();
        stack.pop_back();
        if (nodes[id].left < 0) { leaf_order.push_back(id); continue; }
        stack.push_back(nodes[id].right);
        stack.push_back(nodes[id].left);
    }
}

// ---- append to the ensemble (update_ensemble_per_leaf / per_tree, fitter.cpp:493-542) -----------------------------
model.begin_tree();
const size_t tree = md.n_trees;
model.tree_indices.push_back(md.n_leaves);
auto write_conditions = [&](const HNode &nd, size_t split_row, size_t leaf_row) {
    for (size_t i = 0; i < nd.path.size(); ++i) {
        const HCond &c = nd.path[i];
        if (c.is_cat && c.cat_cand >= 0)
            std::memcpy(&model.categorical_values[(split_row * MD + i) * kCat], cat_cands[c.cat_cand].name.data(), kCat);
        model.is_numerics[split_row * MD + i] = c.is_cat ? 0 : 1;
        model.feature_indices[split_row * MD + i] = c.feat_idx;
        model.feature_values[split_row * MD + i] = c.value;
        model.inequality_directions[leaf_row * MD + i] = c.dir ? 1 : 0;
        model.edge_weights[leaf_row * MD + i] = c.edge_w;
    }
};
const size_t n_new = leaf_order.size();
const size_t L0 = md.n_leaves;
const size_t S_new = oblivious ? tree + 1 : L0 + n_new;
model.depths.resize(S_new, 0);
model.feature_indices.resize(S_new * MD, 0);
model.feature_values.resize(S_new * MD, 0.0f);
model.is_numerics.resize(S_new * MD, 0);
model.categorical_values.resize(S_new * MD * kCat, 0);
model.values.resize((L0 + n_new) * D, 0.0f);
model.edge_weights.resize((L0 + n_new) * MD, 0.0f);
model.inequality_directions.resize((L0 + n_new) * MD, 0);
for (size_t q = 0; q < n_new; ++q) {
    const HNode &nd = nodes[leaf_order[q]];
    const size_t leaf_row = L0 + q;
    if (oblivious) {
        model.depths[tree] = nd.depth;
        write_conditions(nd, tree, leaf_row);
    } else {
        model.depths[leaf_row] = nd.depth;
        write_conditions(nd, leaf_row, leaf_row);
    }
    const int64_t *a = &acc[static_cast<size_t>(leaf_order[q]) * (D + 1)];
    const int64_t cnt = a[D];
    for (int d = 0; d < D; ++d) {
        float v = 0.0f;
        if (cnt > 0 && nd.depth > 0)  // fitter.cpp:574-578; depth-0 leaf keeps 0 (Q7)
            v = static_cast<float>((static_cast<double>(a[d]) / leaf_scale) / static_cast<double>(cnt));
        model.values[leaf_row * D + d] = v;
    }
}
md.n_leaves += static_cast<int32_t>(n_new);
md.n_trees += 1;
md.iteration += 1;  // fitter.cpp:114
++model.version;
}

}  // namespace detail

// ======================================================================================== the stages step() and step_prepared() share
namespace {
// thresholds and scales reach the host through ONE pinned block: [F * B floats | 64-byte aligned StepScales]
char *pinned_thr_block(PinnedBuf &pin, size_t n_thr, float *&h_thr, kern::StepScales *&h_scales) {
    char *pin_ts = static_cast<char *>(pin.ensure(sizeof(float) * std::max<size_t>(1, n_thr) + sizeof(kern::StepScales) + 64));
    h_thr = reinterpret_cast<float *>(pin_ts);
    h_scales = reinterpret_cast<kern::StepScales *>(pin_ts + ((sizeof(float) * std::max<size_t>(1, n_thr) + 63) & ~static_cast<size_t>(63)));
    return pin_ts;
}
}  // namespace

void Engine::read_step_hooks() {
    if (const char *e = hooks::raw(hooks::FORCE_BISECTION)) force_bisection_ = e[0] == '1';   // test hook
    if (const char *e = hooks::raw(hooks::HOST_CATEGORICAL)) force_host_categorical_ = e[0] == '1';   // test hook: host scan of every cell
    if (const char *e = hooks::raw(hooks::QUANTILE_RADIX)) force_radix_ = e[0] == '1';   // test hook: radix multi-select also for small batches
    if (const char *e = hooks::raw(hooks::QUANTILE_SAMPLE)) force_sample_select_ = e[0] == '1';   // test hook: the sample/splitter selection on one GPU
}

// RL-sized steps on one GPU: statistics, quantisation, split candidates and class codes in ONE launch (kern::small_prep);
// GBRL_HIP_NO_SMALL_PREP=1 (tests / measurement): the separate launches
bool Engine::fused_prep_applies(int N, int F, long long n_global) const {
    const bool no_small_prep = [] { const char *e = hooks::raw(hooks::NO_SMALL_PREP); return e && e[0] == '1'; }();   /* read per call: the tests flip it */
    const bool no_sort_codes = [] { const char *e = hooks::raw(hooks::SORT_NO_CODES); return e && e[0] == '1'; }();   /* read per call: the tests flip it */
    const bool uniform_gen = model.meta.generator_type == GBRL_HIP_GEN_UNIFORM;
    return !has_coll_ && n_global == N && F > 0 && fixed_thr_.empty() && !candidates_only_ && !no_small_prep && !no_sort_codes && !force_bisection_ &&
           !force_sample_select_ && !force_radix_ && N <= (uniform_gen ? 8192 : kern::sort_quantiles_max_rows());
}

// ---- 1. gradient statistics and quantisation (A2) ---------------------------------------------------------------------
// sums -> mean -> centred squares -> std, maxima, scales: all on the device (k_stats_mean / k_stats_finish); the host reads the scales
// together with the thresholds (one synchronisation for both).  Row-sharded runs sum the column sums (fp64) and take the maxima (fp32,
// exact) over ranks between the kernels; the arithmetic stays on the device, so one GPU and N GPUs execute the same instructions on the
// same global sums.  Row-sharded: n_global arrives with the first message, and g.chunk_rows follows it.
void Engine::run_grad_stats(FusedStats &g, int N, long long &n_global) {
    hipStream_t s = stream_;
    const int D = g.D, world = has_coll_ ? coll_.world_size : 1;
    const bool cosine = g.cosine;
    const float *dgrads = g.dgrads;
    double *d_stat = g.d_stat;
    float *d_meanden = g.d_meanden;
    kern::StepScales *d_scales = g.d_scales;
    int32_t *d_qg = g.d_qg;
    const size_t n_el = static_cast<size_t>(N) * D;
    const float *d_mean = nullptr, *d_den = nullptr;
    g.done = true;
    // RL-sized batch on one GPU: statistics and quantisation in ONE launch with the same reduction tree (kern::small_stats)
    if (!has_coll_ && g.fuse && n_global == N && kern::small_stats(dgrads, N, D, !cosine, g.chunk_rows, d_stat, d_meanden, d_scales, d_qg, s)) return;
    const int nblk = kern::column_sums_blocks(N, D);
    double *d_part = static_cast<double *>(d_partials_f64_.ensure(sizeof(double) * nblk * 2 * D));
    double *d_stat2 = d_stat + 2 * D;
    // one message per statistics round: the sums and every rank's maxima (gathered through the sum, kern::stats_pack)
    // (+ one word: this rank's row count in the first round -- integers below 2^53 add exactly in float64)
    const size_t smsg_words = static_cast<size_t>(D) * (world + 1) + 1;
    double *d_smsg = has_coll_ ? static_cast<double *>(d_maxbits_.ensure(sizeof(double) * smsg_words)) : nullptr;
    auto exchange_stats = [&](double *st, bool with_row_count) {
        if (!has_coll_) return;
        kern::stats_pack(st, D, world, coll_.rank, d_smsg, s, with_row_count ? static_cast<double>(N) : 0.0);
        exchange(Red::SumF64, d_smsg, smsg_words);
        kern::stats_unpack(d_smsg, D, world, st, s);
        if (with_row_count) {
            // the host needs the global count from here on (chunk length -> fixed-point scale, target ranks of the selection, leaf scale)
            double hv = 0.0;
            hip_check(hipMemcpyAsync(&hv, d_smsg + smsg_words - 1, sizeof(hv), hipMemcpyDeviceToHost, s), "D2H n");
            hip_check(hipStreamSynchronize(s), "sync");
            n_global = static_cast<long long>(hv);
            g.chunk_rows = chunk_rows_of(n_global);
        }
    };
    kern::column_sums(dgrads, N, D, nullptr, d_part, nblk, d_stat, s);
    exchange_stats(d_stat, true);
    if (!cosine) {
        kern::stats_mean(d_stat, n_global, D, d_meanden, s);
        kern::column_sums(dgrads, N, D, d_meanden, d_part, nblk, d_stat2, s);
        exchange_stats(d_stat2, false);
        kern::stats_finish(d_stat, d_stat2, n_global, D, g.chunk_rows, d_meanden, d_scales, s);
        d_mean = d_meanden;
        d_den = d_meanden + D;
    } else {
        kern::stats_finish(d_stat, nullptr, n_global, D, g.chunk_rows, d_meanden, d_scales, s);
    }
    kern::quantize_grads(dgrads, n_el, D, d_mean, d_den, d_scales, d_qg, s);
}

// ---- 2. split candidates and 3. numeric class codes: the numeric preparation of a batch, written into `pb` -------------------------
// (phases transpose / candidates / binning).  step() calls it with its own workspace and its gradient statistics (`fs`: the fused
// preparation kernel computes them in its launch when the shape qualifies, and they are enqueued behind it when it does not);
// prepare_dataset() with the data set's buffers and fs == nullptr (kern::small_prep with want_stats = false).
NumericPrep Engine::prepare_numeric(PrepBuffers &pb, const float *dobs, int N, int F, int Fc, long long n_global, bool prep_candidate, FusedStats *fs) {
    const gbrl_hip_metadata &md = model.meta;
    hipStream_t s = stream_;
    const int B = md.n_bins;
    const bool uniform_gen = md.generator_type == GBRL_HIP_GEN_UNIFORM;
    phase_begin();
    const size_t n_thr = static_cast<size_t>(F) * B;
    float *d_thr = static_cast<float *>(pb.thr.ensure(sizeof(float) * std::max<size_t>(1, n_thr)));
    uint32_t *d_thrkeys = static_cast<uint32_t *>(pb.thrkeys.ensure(sizeof(uint32_t) * std::max<size_t>(1, n_thr)));
    uint32_t *d_kt = nullptr;
    int pass1_chunks = 0;
    if (F > 0 && !prep_candidate) {
        // order-preserving keys, feature-major: every later pass over the observations (selection, binning) streams columns
        d_kt = static_cast<uint32_t *>(pb.kt.ensure(sizeof(uint32_t) * static_cast<size_t>(N) * F));
        // quantile candidates by radix selection (the branch numeric_thresholds will take): the first digit is counted while the keys
        // pass through LDS (k_transpose_count), which saves one of the selection's passes over the keys
        const bool radix_path = fixed_thr_.empty() && md.generator_type != GBRL_HIP_GEN_UNIFORM && !force_bisection_ && radix_select_applies(B, n_global);
        if (radix_path)
            pass1_chunks = kern::transpose_keys_count(dobs, N, F, d_kt, static_cast<uint32_t *>(d_radix_partial_.ensure(kern::radix_partial_bytes(F))), s);
        if (pass1_chunks == 0) kern::transpose_keys(dobs, N, F, d_kt, s);
    }
    phase_end("transpose");
    phase_begin();
    // class codes (group-major: [slot/16][row][slot%16], u16): allocated here because the RL-sized selection (one sort kernel per
    // step) writes the numeric codes itself
    const int n_slots_codes = F + Fc;
    const int n_code_groups = (n_slots_codes + kern::kCodeGroup - 1) / kern::kCodeGroup;
    const size_t code_elems = static_cast<size_t>(std::max(1, n_code_groups)) * N * kern::kCodeGroup;
    uint16_t *d_codes = static_cast<uint16_t *>(pb.codes.ensure(sizeof(uint16_t) * code_elems));
    // Only the padding slots behind the last categorical column are written by nobody (the numeric writers fill whole groups of 16, padding
    // included, the categorical ones every (row, column)): no clearing when the slots fill their groups exactly (configs[4]: 192 + 64).
    if (Fc > 0 && (F + Fc) % kern::kCodeGroup != 0) hip_check(hipMemsetAsync(d_codes, 0, sizeof(uint16_t) * code_elems, s), "memset codes");
    bool codes_from_sort = false;
    const uint32_t *root_le = nullptr;
    bool prep_done = false;
    const uint16_t *d_codes_fm = nullptr;   // feature-major copy of the numeric codes (kern::small_prep writes it for kern::small_grow)
    int prep_launches = 3;   // (diagnostic, reported as a pseudo-phase at profiling level 2: 1 = the fused preparation kernel ran)
    if (prep_candidate) {
        const int64_t *d_cum = uniform_gen ? nullptr : quantile_cum_device(quantile_target_ranks(n_global, B), n_global, B);
        bool stats_done = false;
        uint16_t *d_fm = static_cast<uint16_t *>(pb.codes_fm.ensure(sizeof(uint16_t) * static_cast<size_t>(N) * F));
        prep_done = kern::small_prep(dobs, N, F, B, uniform_gen, d_cum, d_thr, d_thrkeys, d_codes, d_fm, fs ? fs->dgrads : nullptr, fs ? fs->D : 1, fs ? !fs->cosine : false,
                                     fs ? fs->chunk_rows : 0, fs ? fs->d_stat : nullptr, fs ? fs->d_meanden : nullptr, fs ? fs->d_scales : nullptr, fs ? fs->d_qg : nullptr,
                                     fs != nullptr && fs->fuse, &stats_done, s);
        if (prep_done) { codes_from_sort = true; last_quantile_fallback_ = false; prep_launches = 1; d_codes_fm = d_fm; }
        if (fs) {
            if (stats_done) fs->done = true;
            else run_grad_stats(*fs, N, n_global);
        }
        if (!prep_done) {   // the shape did not qualify after all: the separate launches, keys first
            d_kt = static_cast<uint32_t *>(pb.kt.ensure(sizeof(uint32_t) * static_cast<size_t>(N) * F));
            kern::transpose_keys(dobs, N, F, d_kt, s);
        }
    }
    if (F > 0 && !prep_done) numeric_thresholds(dobs, N, F, B, n_global, d_kt, d_thr, d_thrkeys, pb.root_le, &root_le, pass1_chunks, d_codes, &codes_from_sort);
    phase_end("candidates");
    prof_marks_[1] = std::chrono::steady_clock::now();
    prep_launches_ = F > 0 ? prep_launches : 0;
    // numeric class codes (3. below) before the host waits for the categorical scan
    phase_begin();
    if (F > 0 && !codes_from_sort) kern::bin_cols(d_kt, N, F, d_thrkeys, B, d_codes, s);
    phase_end("binning");
    NumericPrep np;
    np.d_thr = d_thr; np.d_thrkeys = d_thrkeys; np.d_codes = d_codes; np.d_kt = d_kt; np.d_codes_fm = d_codes_fm; np.root_le = root_le;
    return np;
}

// ---- feature slots, candidate order, weights; then 4. growth (level-synchronous; Engine::grow_tree) and 5. leaf sums ------------------
void Engine::grow_step_tree(const StepData &sd, std::vector<HNode> &nodes, std::vector<int> &frontier, std::vector<int64_t> &acc, double &leaf_scale) {
    const gbrl_hip_metadata &md = model.meta;
    const int N = sd.N, F = sd.F, Fc = sd.Fc, D = md.output_dim, B = md.n_bins, MD = md.max_depth;
    const bool cosine = md.split_score_func == GBRL_HIP_SCORE_COSINE;
    const bool oblivious = model.oblivious();
    const std::vector<CatCandidate> &cat_cands = *sd.cat_cands;
    const std::vector<int> &cat_classes = *sd.cat_classes;
    const size_t n_thr = static_cast<size_t>(F) * B;
    float *h_thr = nullptr;
    kern::StepScales *h_scales_pin = nullptr;
    char *pin_ts = pinned_thr_block(pin_thr_, n_thr, h_thr, h_scales_pin);

    // ---- feature slots, candidate order, weights ---------------------------------------------------------------------
    const int n_slots = F + Fc;
    int NB = F > 0 ? B + 1 : 1;
    for (int c = 0; c < Fc; ++c) NB = std::max(NB, cat_classes[c] + 1);
    const int FG = kern::hist_feature_group(NB, D);
    if (kern::hist_lds_bytes(NB, D, FG) > kern::kHistLdsLimit)
        throw Unsupported("(classes per feature) x (output_dim + 1) does not fit the 160 KiB LDS");
    if (static_cast<size_t>(NB + 2) * (D + 1) * 8 > 150 * 1024) throw Unsupported("score kernel LDS limit");
    const int Fp = ((n_slots + FG - 1) / FG) * FG;
    const int n_groups = Fp / FG;
    // internal candidate order = slot-grouped; cand_ref maps to the reference's candidate index (numeric f-major, then the
    // categorical candidates in the hash-map order) which decides ties (lowest reference index wins)
    std::vector<FeatureSlot> slots_local;
    std::vector<int32_t> cand_ref_local, cand_slot_local;
    std::vector<float> cand_w_local;
    std::vector<int> ref_to_internal_local;
    // numeric-only steps: these constants depend on (F, n_bins, policy, feature weights, feature mapping) only -- built once, kept in
    // Engine::step_const_ together with their uploaded copy (grow_tree)
    // A column subset (sd.cols) builds its tables locally, and overwrites the device staging block on its way: the cached upload is dropped,
    // the host tables of the full step stay.
    const bool const_cacheable = Fc == 0 && F > 0 && sd.cols == nullptr;
    // mixed steps: the numeric candidates come first in every table and are the same from step to step -- only the categorical
    // tails (this batch's candidates) are rebuilt and uploaded (51 200 numeric against ~2 000 categorical entries at configs[4])
    const bool prefix_cacheable = Fc > 0 && F > 0;
    if (sd.cols != nullptr) step_const_.dev_base = nullptr;
    bool reuse = false;
    if (const_cacheable || prefix_cacheable) {
        StepConstCache &cc = step_const_;
        reuse = cc.valid && cc.F == F && cc.B == B && cc.oblivious == (oblivious ? 1 : 0) && cc.fw == model.feature_weights && cc.rev == model.reverse_num;
        if (!reuse) {
            cc.valid = false;
            cc.dev_base = nullptr;
            cc.F = F; cc.B = B; cc.oblivious = oblivious ? 1 : 0;
            cc.fw = model.feature_weights;
            cc.rev = model.reverse_num;
        }
    }
    const bool shared_tables = const_cacheable || prefix_cacheable;
    std::vector<FeatureSlot> &slots = shared_tables ? step_const_.slots : slots_local;
    std::vector<int32_t> &cand_ref = shared_tables ? step_const_.cand_ref : cand_ref_local;
    std::vector<int32_t> &cand_slot = shared_tables ? step_const_.cand_slot : cand_slot_local;
    std::vector<float> &cand_w = shared_tables ? step_const_.cand_w : cand_w_local;
    std::vector<int> &ref_to_internal = shared_tables ? step_const_.ref_to_internal : ref_to_internal_local;
    int n_cand = 0;
    const int n_num_cand = F * B;
    if (reuse && const_cacheable) {
        n_cand = static_cast<int>(cand_ref.size());
    } else {
        const bool keep_prefix = reuse && prefix_cacheable;   // the numeric part of every table is in place
        slots.resize(n_slots);
        if (keep_prefix) {
            n_cand = n_num_cand;
        } else {
            for (int f = 0; f < F; ++f) { slots[f] = {0, B, n_cand, 0}; n_cand += B; }
        }
        for (int c = 0; c < Fc; ++c) { slots[F + c] = {1, cat_classes[c], n_cand, 0}; n_cand += cat_classes[c]; }
        if (keep_prefix) {
            cand_ref.resize(n_cand); cand_w.resize(n_cand); ref_to_internal.resize(n_cand); cand_slot.resize(n_cand);
        } else {
            cand_ref.assign(n_cand, 0);
            cand_w.assign(n_cand, 0.0f);
            ref_to_internal.assign(n_cand, 0);
            cand_slot.assign(n_cand, 0);
            for (int f = 0; f < F; ++f)
                for (int k = 0; k < B; ++k) {
                    const int j = slots[f].cand_base + k;
                    cand_ref[j] = f * B + k;
                    // feature weight: greedy indexes by feature_idx, oblivious by the reverse mapping (fitter.cpp:331 vs 432-434, Q6)
                    const int mf = sd.cols ? sd.cols[f] : f;
                    const int wi = oblivious ? model.reverse_num[mf] : mf;
                    cand_w[j] = (wi >= 0 && wi < md.input_dim) ? model.feature_weights[wi] : 0.0f;
                }
            for (int j = 0; j < n_num_cand; ++j) ref_to_internal[cand_ref[j]] = j;
            for (int fs = 0; fs < F; ++fs)
                for (int k = 0; k < slots[fs].n_cand; ++k) cand_slot[slots[fs].cand_base + k] = fs;
        }
        for (size_t q = 0; q < cat_cands.size(); ++q) {
            const CatCandidate &cc = cat_cands[q];
            const int j = slots[F + cc.feat].cand_base + (cc.cls - 1);
            cand_ref[j] = F * B + static_cast<int>(q);
            const int wi = oblivious ? model.reverse_cat[cc.feat] : cc.feat + F;
            cand_w[j] = (wi >= 0 && wi < md.input_dim) ? model.feature_weights[wi] : 0.0f;
        }
        for (int j = n_num_cand; j < n_cand; ++j) ref_to_internal[cand_ref[j]] = j;
        for (int fs = F; fs < n_slots; ++fs)
            for (int k = 0; k < slots[fs].n_cand; ++k) cand_slot[slots[fs].cand_base + k] = fs;
        if (shared_tables) step_const_.valid = true;
    }

    // thresholds and scales reach the pinned block through ONE launch (device-written host memory) instead of two copy-engine transfers:
    // kern::publish_pair at the top of the level loop (grow_tree); the one-launch growth publishes the scales itself and hands the
    // winners' thresholds over with its result blocks
    static_assert(sizeof(kern::StepScales) % 4 == 0, "copied as 32-bit words");
    void *pin_dev = nullptr;
    hip_check(hipHostGetDevicePointer(&pin_dev, pin_ts, 0), "hipHostGetDevicePointer");

    prof_marks_[3] = std::chrono::steady_clock::now();
    // ---- 4. growth (level-synchronous; Engine::grow_tree) and 5. leaf sums --------------------------------------------------
    GrowCtx gc{};
    gc.N = N; gc.F = F; gc.Fc = Fc; gc.D = D; gc.B = B; gc.MD = MD; gc.NB = NB; gc.FG = FG; gc.Fp = Fp; gc.n_groups = n_groups;
    gc.n_slots = n_slots; gc.n_cand = n_cand; gc.chunk_rows = sd.chunk_rows; gc.n_global = sd.n_global; gc.cosine = cosine; gc.oblivious = oblivious;
    gc.slots = &slots; gc.cand_w = &cand_w; gc.cand_ref = &cand_ref; gc.ref_to_internal = &ref_to_internal; gc.cand_slot = &cand_slot;
    gc.const_cacheable = const_cacheable; gc.cat_cands = &cat_cands;
    gc.prefix_cacheable = prefix_cacheable; gc.n_num_cand = n_num_cand; gc.cand_cap = (F + Fc) * B;
    gc.pub_thr_dev = static_cast<char *>(pin_dev); gc.pub_scales_dev = static_cast<char *>(pin_dev) + (reinterpret_cast<char *>(h_scales_pin) - pin_ts); gc.pub_thr_bytes = sizeof(float) * n_thr;
    const NumericPrep &np = sd.prep;
    gc.h_thr = h_thr; gc.h_scales = h_scales_pin; gc.d_thr = np.d_thr; gc.d_thrkeys = np.d_thrkeys; gc.root_le = (Fc == 0 && !has_coll_) ? np.root_le : nullptr; gc.d_kt = np.d_kt; gc.d_codes = np.d_codes; gc.d_codes_fm = np.d_codes_fm;
    gc.d_qg = sd.stats->d_qg; gc.dgrads = sd.stats->dgrads; gc.d_meanden = cosine ? nullptr : sd.stats->d_meanden; gc.d_scales = sd.stats->d_scales;
    grow_tree(gc, nodes, frontier, acc, leaf_scale);
}

// ======================================================================================================== step
void Engine::step(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *grads, bool grads_dev, int n,
                  int n_num, int n_cat) {
    gbrl_hip_metadata &md = model.meta;
    // GBRL::step, gbrl.cpp:946-958
    if (md.iteration == 0) { md.n_num_features = n_num; md.n_cat_features = n_cat; }
    if (n_num != md.n_num_features || n_cat != md.n_cat_features) throw InvalidArgument("Incompatible dataset");
    if (n_num + n_cat != md.input_dim) throw InvalidArgument("Total number of features != correct input dim");
    if (n <= 0 || grads == nullptr) throw InvalidArgument("Cannot call step without grads!");
    if (n_num > 0 && obs == nullptr) throw InvalidArgument("Cannot call step without obs!");
    if (n_cat > 0 && cat == nullptr) throw InvalidArgument("Cannot call step without cat_obs!");
    if (md.max_depth > kern::kMaxPath) throw Unsupported("max_depth > 32 is not supported");
    if (md.n_bins < 1 || md.n_bins > 65534) throw Unsupported("n_bins must be in [1, 65534]");
    ensure_device();
    read_step_hooks();
    detail::StepInputs in{obs, obs_dev, cat, cat_dev, grads, grads_dev, n, n_num, n_cat};
    const bool host_categorical = force_host_categorical_ || cat_clashed_;
    if (step_pass(in, host_categorical)) return;
    // Two different cells of one feature share a 64-bit hash (2^-64 per pair of cells).  The tree just grown used the wrong dictionary id for
    // one of them, but nothing has been booked yet (append_tree is what changes the model): the remembered cells are forgotten, THIS model
    // stays on the host scan of every cell from here on -- it compares bytes, so the pair cannot clash again -- and the tree is grown once
    // more from the same inputs.
    if (host_categorical) throw HipError("two different categories of one feature share a 64-bit hash on the host scan (internal error)");
    if (has_coll_) throw HipError("two different categories of one feature share a 64-bit hash: step refused (row-sharded run: set GBRL_HIP_HOST_CATEGORICAL=1 on every rank)");
    cat_clashed_ = true;
    ++cat_clash_redos_;
    if (!step_pass(in, /*host_categorical=*/true)) throw HipError("two different categories of one feature share a 64-bit hash on the host scan (internal error)");
}

// ---- inputs on the device ---------------------------------------------------------------------------------------------
void Engine::stage_step_inputs(detail::StepInputs &in) {
    hipStream_t s = stream_;
    const int N = in.N, F = in.F, Fc = in.Fc, D = model.meta.output_dim;
    phase_begin();
    in.dobs = in.obs;
    if (F > 0 && !in.obs_dev) {
        in.dobs = static_cast<float *>(d_obs_.ensure(sizeof(float) * N * F));
        hip_check(hipMemcpyAsync(const_cast<float *>(in.dobs), in.obs, sizeof(float) * N * F, hipMemcpyHostToDevice, s), "H2D obs");
    }
    in.dgrads = in.grads;
    if (!in.grads_dev) {
        in.dgrads = static_cast<float *>(d_grads_.ensure(sizeof(float) * N * D));
        hip_check(hipMemcpyAsync(const_cast<float *>(in.dgrads), in.grads, sizeof(float) * N * D, hipMemcpyHostToDevice, s), "H2D grads");
    }
    // categorical cells on the device: the distinct categories of the batch are found there (enqueue_categorical_scan);
    // the host-side scan of every cell is only the fallback
    in.dcells = in.cat;
    if (Fc > 0 && !in.cat_dev) {
        char *t = static_cast<char *>(d_pcells_.ensure(static_cast<size_t>(N) * Fc * kCat));
        hip_check(hipMemcpyAsync(t, in.cat, static_cast<size_t>(N) * Fc * kCat, hipMemcpyHostToDevice, s), "H2D cat cells");
        in.dcells = t;
    }
    phase_end("inputs");
}

// ---- categorical candidates (A5) ----------------------------------------------------------------------------------------
// fit(): the candidates of the whole data set (fitter.cpp:152-164), their dictionary still on the device.  Else the distinct cells found by
// the scan enqueued earlier, replayed on the host; and when that is switched off or declines -- more distinct categories than candidates
// are kept in a row-sharded step, sizes beyond the scan -- the reference's rule on every cell, on the host.
detail::CatStage Engine::categorical_stage(const detail::StepInputs &in, bool host_categorical) {
    const int N = in.N, Fc = in.Fc, D = model.meta.output_dim, B = model.meta.n_bins;
    detail::CatStage cs;
    cs.classes.assign(Fc, 0);
    if (Fc <= 0) return cs;
    if (fixed_cat_valid_) {
        cs.cands = fixed_cat_cands_;
        cs.classes = fixed_cat_classes_;
        cs.codes = detail::CatStage::Dict;
        return cs;
    }
    if ((has_coll_ || !host_categorical) && collect_categorical_candidates(in.dcells, N, Fc, B, in.dgrads, D, cs.cands, cs.classes)) {
        cs.codes = cat_.table.valid ? detail::CatStage::Table : detail::CatStage::Dict;
        return cs;
    }
    std::vector<char> cat_host_buf;
    const char *hcat = in.cat;
    std::vector<float> grads_host_buf;
    const float *hgrads = in.grads;
    if (in.cat_dev) {
        cat_host_buf.resize(static_cast<size_t>(N) * Fc * kCat);
        hip_check(hipMemcpy(cat_host_buf.data(), in.cat, cat_host_buf.size(), hipMemcpyDeviceToHost), "D2H cat");
        hcat = cat_host_buf.data();
    }
    if (in.grads_dev) {
        grads_host_buf.resize(static_cast<size_t>(N) * D);
        hip_check(hipMemcpy(grads_host_buf.data(), in.grads, grads_host_buf.size() * 4, hipMemcpyDeviceToHost), "D2H grads");
        hgrads = grads_host_buf.data();
    }
    cs.cands.clear();
    std::fill(cs.classes.begin(), cs.classes.end(), 0);
    if (has_coll_) sharded_categorical_ranking(hcat, hgrads, N, Fc, D, B, cs.cands, cs.h_codes, cs.classes);
    else detail::categorical_candidates(hcat, hgrads, N, Fc, D, B, cs.cands, cs.h_codes, cs.classes);
    cs.codes = detail::CatStage::Host;
    return cs;
}

// fit(): only the candidates of this (whole) data set are wanted
void Engine::finish_candidates_only(const detail::CatStage &cs, int Fc, const float *d_thr, size_t n_thr) {
    float *h_thr = nullptr;
    kern::StepScales *h_scales_pin = nullptr;
    (void)pinned_thr_block(pin_thr_, n_thr, h_thr, h_scales_pin);
    if (n_thr) hip_check(hipMemcpyAsync(h_thr, d_thr, sizeof(float) * n_thr, hipMemcpyDeviceToHost, stream_), "D2H thr");
    hip_check(hipStreamSynchronize(stream_), "sync");
    fixed_thr_.assign(h_thr, h_thr + n_thr);
    if (Fc > 0) {
        verify_pending_categories();
        if (cat_clash_) { cat_clash_ = false; cat_mem_.forget(); throw HipError("two different categories of one feature share a 64-bit hash: fit() refused"); }
        if (cs.codes == detail::CatStage::Host)   // (the host scan: GBRL_HIP_HOST_CATEGORICAL=1, or the device scan declined -- more than 2^21 distinct cells)
            throw Unsupported("fit(): the categorical candidates of the whole data set need the device scan (GBRL_HIP_HOST_CATEGORICAL=1, or more than 2^21 distinct categories)");
        fixed_cat_cands_ = cs.cands;
        fixed_cat_classes_ = cs.classes;
        fixed_cat_valid_ = true;
    }
    phases_resolve();
}

// ---- 3. categorical class codes (group-major: [slot/16][row][slot%16], u16) --------------------------------------------
void Engine::launch_cat_codes(const detail::StepInputs &in, const detail::CatStage &cs, uint16_t *d_codes) {
    hipStream_t s = stream_;
    const int N = in.N, F = in.F, Fc = in.Fc;
    if (Fc <= 0) return;
    phase_begin();
    switch (cs.codes) {
        case detail::CatStage::Table:
            kern::cat_step_codes_table(in.dcells, N, Fc, F, cat_.table.keys, cat_.table.slot_q, cat_.table.cls_of_q, cat_.table.log2_cap, d_codes, s);
            break;
        case detail::CatStage::Dict:
            kern::cat_step_codes(in.dcells, N, Fc, F, cat_.dict.off, cat_.dict.hash, cat_.dict.cls, cat_.dict.words, d_codes, s);
            break;
        default: {
            uint16_t *d_cc2 = static_cast<uint16_t *>(d_catcodes_.ensure(sizeof(uint16_t) * cs.h_codes.size()));
            hip_check(hipMemcpyAsync(d_cc2, cs.h_codes.data(), sizeof(uint16_t) * cs.h_codes.size(), hipMemcpyHostToDevice, s), "H2D cat codes");
            kern::scatter_cat_codes_grouped(d_cc2, N, Fc, F, d_codes, s);
        }
    }
    phase_end("cat_codes");
}

// One attempt at the step, from the staging of its inputs to the tree joining the ensemble.  false: the categorical replay took one cell
// for another under the same 64-bit hash -- the tree is dropped, nothing has been booked, and step() makes a second pass on the host scan.
bool Engine::step_pass(detail::StepInputs &in, bool host_categorical) {
    const gbrl_hip_metadata &md = model.meta;
    const int N = in.N, F = in.F, Fc = in.Fc, D = md.output_dim, B = md.n_bins;
    const bool cosine = md.split_score_func == GBRL_HIP_SCORE_COSINE;
    prof_step_entry_ = std::chrono::steady_clock::now();   // the per-step diagnostics: a second pass reports itself alone
    ev_used_ = 0;
    ev_names_.clear();
    exch_bytes_ = 0;
    exch_calls_ = 0;
    // global row count (rows are sharded over ranks): it travels with the first gradient-statistics message below (no exchange and no
    // idle device for it); until then n_global holds this rank's count and nothing reads it
    long long n_global = N;
    stage_step_inputs(in);
    prof_marks_[0] = std::chrono::steady_clock::now();
    // the scan for the batch's distinct categorical cells goes first: its result is read by the HOST (collect_categorical_candidates)
    cat_.launched = false;
    if (Fc > 0 && !fixed_cat_valid_ && (has_coll_ || !host_categorical)) (void)enqueue_categorical_scan(in.dcells, N, Fc, B);

    // ---- 1. gradient statistics and quantisation (A2): Engine::run_grad_stats -------------------------------------------------
    phase_begin();
    float *d_meanden = static_cast<float *>(d_meanden_.ensure(sizeof(float) * 2 * D));
    double *d_stat = static_cast<double *>(d_stat_.ensure(sizeof(double) * 4 * D));
    if (D > 512) throw Unsupported("output_dim > 512");
    // LDS accumulators are int32 and one block adds at most `chunk_rows` rows into a cell: the power-of-two scale keeps
    // chunk_rows * max|q| < 2^31 (exactness of the wrapped int32 sums, step_hist_build.hip k_hist_build).  Leaf sums: int64 fixed point with
    // n_global * max|g| * 2^lbits < 2^62.
    kern::StepScales *d_scales = static_cast<kern::StepScales *>(d_scales_.ensure(sizeof(kern::StepScales)));
    int32_t *d_qg = static_cast<int32_t *>(d_qg_.ensure(sizeof(int32_t) * static_cast<size_t>(N) * D));
    const bool no_small_stats = [] { const char *e = hooks::raw(hooks::NO_SMALL_STATS); return e && e[0] == '1'; }();   /* read per call: the tests flip it */
    // (row-sharded: the chunk length is set again once the global count is known)
    FusedStats gs{in.dgrads, D, cosine, d_stat, d_meanden, d_scales, d_qg, chunk_rows_of(n_global), !no_small_stats};
    // RL-sized steps on one GPU: the statistics ride in the fused preparation kernel's launch (prepare_numeric)
    const bool prep_candidate = fused_prep_applies(N, F, n_global);
    if (!prep_candidate) run_grad_stats(gs, N, n_global);
    phase_end("grad_stats");

    // ---- 2. split candidates and 3. numeric class codes: Engine::prepare_numeric, into this engine's workspace ----------------
    // (thresholds and scales reach the host through ONE pinned block, copied behind the binning kernel: nothing waits for them
    // until the first level's result block has arrived)
    const NumericPrep np = prepare_numeric(prep_ws_, in.dobs, N, F, Fc, n_global, prep_candidate, &gs);
    const detail::CatStage cs = categorical_stage(in, host_categorical);
    prof_marks_[2] = std::chrono::steady_clock::now();
    if (candidates_only_) { finish_candidates_only(cs, Fc, np.d_thr, static_cast<size_t>(F) * B); return true; }
    launch_cat_codes(in, cs, np.d_codes);
    // ---- feature slots, candidate order, weights, 4. growth and 5. leaf sums: Engine::grow_step_tree ----------------------------
    StepData sd{};
    sd.N = N; sd.F = F; sd.Fc = Fc; sd.n_global = n_global; sd.chunk_rows = gs.chunk_rows; sd.prep = np; sd.stats = &gs;
    sd.cat_cands = &cs.cands; sd.cat_classes = &cs.classes;
    std::vector<HNode> nodes;
    std::vector<int> frontier;
    std::vector<int64_t> acc;
    double leaf_scale = 1.0;
    grow_step_tree(sd, nodes, frontier, acc, leaf_scale);
    verify_pending_categories();
    if (cat_clash_) {
        cat_clash_ = false;
        cat_mem_.forget();
        return false;
    }
    append_tree(model, nodes, frontier, acc, leaf_scale, cs.cands);
    hip_check(hipGetLastError(), "step kernels");
    phases_resolve();
    return true;
}

// ===================================================================================================== fit
Engine::ColumnStats::ColumnStats(Engine &e) : e_(e), D_(e.model.meta.output_dim), hs_(2 * D_) {
    d_zero_ = static_cast<float *>(e_.d_fit_zero_.ensure(sizeof(float) * D_));
    hip_check(hipMemsetAsync(d_zero_, 0, sizeof(float) * D_, e_.stream_), "memset");
    d_stat_ = static_cast<double *>(e_.d_stat_.ensure(sizeof(double) * 4 * D_));
}

const std::vector<double> &Engine::ColumnStats::sums(const float *g, int rows, const float *center) {
    hipStream_t s = e_.stream_;
    const int nblk = kern::column_sums_blocks(rows, D_);
    double *d_part = static_cast<double *>(e_.d_partials_f64_.ensure(sizeof(double) * nblk * 2 * D_));
    kern::column_sums(g, rows, D_, center, d_part, nblk, d_stat_, s);
    hip_check(hipMemcpyAsync(hs_.data(), d_stat_, sizeof(double) * 2 * D_, hipMemcpyDeviceToHost, s), "D2H stat");
    hip_check(hipStreamSynchronize(s), "sync");
    return hs_;
}

const std::vector<double> &Engine::ColumnStats::weighted_sums(const float *g, const int32_t *labels, const float *factor, int rows) {
    hipStream_t s = e_.stream_;
    const int nblk = kern::column_sums_blocks(rows, D_);
    double *d_part = static_cast<double *>(e_.d_partials_f64_.ensure(sizeof(double) * nblk * 2 * D_));
    kern::column_sums_weighted(g, labels, factor, rows, D_, d_part, nblk, d_stat_, s);
    hip_check(hipMemcpyAsync(hs_.data(), d_stat_, sizeof(double) * 2 * D_, hipMemcpyDeviceToHost, s), "D2H stat");
    hip_check(hipStreamSynchronize(s), "sync");
    return hs_;
}

float Engine::ColumnStats::rmse(const float *grads_dev, int rows) {
    sums(grads_dev, rows, d_zero_);
    double tot = 0.0;
    for (int d = 0; d < D_; ++d) tot += hs_[d];
    return sqrtf(0.5f * static_cast<float>(tot) * (1.0f / static_cast<float>(rows)));
}

float Engine::fit(const float *obs, bool obs_dev, const char *cat, bool cat_dev, const float *targets, bool targets_dev, int n, int n_num,
                  int n_cat, int iterations, bool shuffle) {
    gbrl_hip_metadata &md = model.meta;
    if (md.iteration == 0) { md.n_num_features = n_num; md.n_cat_features = n_cat; }                      // gbrl.cpp:996-999
    if (n_num != md.n_num_features || n_cat != md.n_cat_features) throw InvalidArgument("Incompatible dataset");
    if (n <= 0 || targets == nullptr) throw InvalidArgument("Cannot call fit without targets!");
    if (n_num > 0 && obs == nullptr) throw InvalidArgument("Cannot call fit without obs!");
    if (iterations < 0) throw InvalidArgument("iterations must be >= 0");
    if (n_cat > 0 && cat == nullptr) throw InvalidArgument("Cannot call fit without cat_obs!");
    if (has_coll_) throw Unsupported("fit() is not supported on a row-sharded model");
    if (md.batch_size <= 0) throw InvalidArgument("batch_size must be positive");
    ensure_device();
    hipStream_t s = stream_;
    const int F = n_num, Fc = n_cat, D = md.output_dim;
    struct Guard { Engine *e; ~Guard() { e->fixed_thr_.clear(); e->fixed_cat_valid_ = false; e->fixed_cat_cands_.clear(); e->candidates_only_ = false; } } guard{this};

    // the data set on the device, optionally in shuffled order (gbrl.cpp:1016-1024, 1039-1067; the reference seeds
    // std::mt19937 from std::random_device, i.e. the order differs from run to run there too)
    const float *dobs = obs, *dtar = targets;
    const char *dcat = cat;
    if (Fc > 0 && !cat_dev) {
        char *t = static_cast<char *>(d_fit_cells_.ensure(static_cast<size_t>(n) * Fc * kCat));
        hip_check(hipMemcpyAsync(t, cat, static_cast<size_t>(n) * Fc * kCat, hipMemcpyHostToDevice, s), "H2D cat cells");
        dcat = t;
    }
    if (F > 0 && !obs_dev) {
        float *t = static_cast<float *>(d_fit_obs_.ensure(sizeof(float) * static_cast<size_t>(n) * F));
        hip_check(hipMemcpyAsync(t, obs, sizeof(float) * static_cast<size_t>(n) * F, hipMemcpyHostToDevice, s), "H2D obs");
        dobs = t;
    }
    if (!targets_dev) {
        float *t = static_cast<float *>(d_fit_targets_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
        hip_check(hipMemcpyAsync(t, targets, sizeof(float) * static_cast<size_t>(n) * D, hipMemcpyHostToDevice, s), "H2D targets");
        dtar = t;
    }
    if (shuffle) {
        std::vector<int32_t> perm(n);
        std::iota(perm.begin(), perm.end(), 0);
        std::random_device rd;
        std::mt19937 gen(rd());
        std::shuffle(perm.begin(), perm.end(), gen);
        int32_t *d_perm = static_cast<int32_t *>(d_fit_perm_.ensure(sizeof(int32_t) * n));
        hip_check(hipMemcpyAsync(d_perm, perm.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s), "H2D perm");
        float *o2 = static_cast<float *>(d_fit_obs2_.ensure(sizeof(float) * static_cast<size_t>(n) * F));
        float *t2 = static_cast<float *>(d_fit_targets2_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
        kern::gather_rows(dobs, d_perm, o2, n, F, s);
        kern::gather_rows(dtar, d_perm, t2, n, D, s);
        if (Fc > 0) {   // whole 128-byte cells travel with their row (the reference's shuffled copy keeps only their first byte, Q12)
            char *c2 = static_cast<char *>(d_fit_cells2_.ensure(static_cast<size_t>(n) * Fc * kCat));
            kern::gather_rows(reinterpret_cast<const float *>(dcat), d_perm, reinterpret_cast<float *>(c2), n, Fc * (kCat / 4), s);
            dcat = c2;
        }
        hip_check(hipStreamSynchronize(s), "sync");   // perm goes out of scope
        dobs = o2;
        dtar = t2;
    }
    ColumnStats stats(*this);
    // bias = column means of the targets (gbrl.cpp:1075-1077)
    const std::vector<double> &hs = stats.sums(dtar, n, nullptr);
    for (int d = 0; d < D; ++d) model.bias[d] = static_cast<float>(hs[d] / static_cast<double>(n));
    ++model.version;

    // split candidates from the whole data set, once (fitter.cpp:134-164)
    {
        // Categorical columns: when the data set holds more distinct categories than Fc * n_bins the reference ranks them by the norms of
        // `full_grads` (fitter.cpp:152-160) = predict_cpu(whole data set, trees [0, iterations)) - targets.  predict() restates that call's
        // quirks (predictor.cpp:127-135): a fresh model, or iterations > n_trees, gives the bias alone; iterations == 0 means every tree.
        const float *cand_grads = dtar;   // numeric-only: the gradients feed the (unused) statistics only
        if (Fc > 0) {
            float *fp = static_cast<float *>(d_fit_preds_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
            in_fit_ = true;
            try { predict(dobs, true, dcat, true, n, F, Fc, 0, iterations, fp, true); } catch (...) { in_fit_ = false; throw; }
            in_fit_ = false;
            float *fg = static_cast<float *>(d_fit_grads_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
            kern::sub_arrays(fp, dtar, fg, static_cast<size_t>(n) * D, s);
            cand_grads = fg;
        }
        candidates_only_ = true;
        step(dobs, true, dcat, true, cand_grads, true, n, F, Fc);   // returns right after the candidates
        candidates_only_ = false;
    }
    const int bs = md.batch_size;
    float *d_preds = static_cast<float *>(d_fit_preds_.ensure(sizeof(float) * static_cast<size_t>(std::max(n, 1)) * D));
    float *d_grads = static_cast<float *>(d_fit_grads_.ensure(sizeof(float) * static_cast<size_t>(std::min(n, bs)) * D));
    int start = 0;
    int bn = start + bs < n ? bs : n - start;                                   // fitter.cpp:120
    for (int i = 0; i < iterations; ++i) {
        const float *ob = dobs + static_cast<size_t>(start) * F;
        const float *tb = dtar + static_cast<size_t>(start) * D;
        const char *cb = Fc > 0 ? dcat + static_cast<size_t>(start) * Fc * kCat : nullptr;
        in_fit_ = true;
        try { predict(ob, true, cb, true, bn, F, Fc, 0, i, d_preds, true); } catch (...) { in_fit_ = false; throw; }   // trees [0, i) -- i == 0 means "all" (fitter.cpp:187)
        in_fit_ = false;
        kern::sub_arrays(d_preds, tb, d_grads, static_cast<size_t>(bn) * D, s);
        step(ob, true, cb, true, d_grads, true, bn, F, Fc);
        start += bn;                                                            // fitter.cpp:228-231
        if (start >= n) start = 0;
        bn = start + bs < n ? bs : n - start;
    }
    // loss on the whole data set over trees [0, iterations) (fitter.cpp:246-251)
    in_fit_ = true;   // the chain here too: the returned loss does not depend on how a stand-alone predict() would split the trees
    try { predict(dobs, true, Fc > 0 ? dcat : nullptr, true, n, F, Fc, 0, iterations, d_preds, true); } catch (...) { in_fit_ = false; throw; }
    in_fit_ = false;
    float *d_full_grads = static_cast<float *>(d_fit_grads_.ensure(sizeof(float) * static_cast<size_t>(n) * D));
    kern::sub_arrays(d_preds, dtar, d_full_grads, static_cast<size_t>(n) * D, s);
    return stats.rmse(d_full_grads, n);
}

}  // namespace gbrl
