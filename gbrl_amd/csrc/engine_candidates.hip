// engine_candidates.hip -- the numeric split candidates of a step (A3, A4; see engine_step_detail.h): the choice of the threshold route and one
// function per route (fixed, uniform, bisection, LDS sort, radix multi-select, sample/splitter selection), and the host side of the
// copy-free hand-overs.
#include "engine_step_detail.h"

namespace gbrl {

namespace detail {

// Host side of the copy-free hand-overs: poll a sequence word in coherent pinned memory; every 16384 polls ask the stream for errors
// (a faulted kernel never publishes) and give up after GBRL_HIP_SPIN_SECONDS (default 120) of wall clock -- a hung kernel must not
// spin a core forever, and a slow but healthy run (counter profiling, several ranks sharing one device) must not be declared dead.
// Before giving up the stream is synchronised: kernels still in flight would otherwise keep storing into the pinned result blocks and
// pools that the next call reuses; a stream that does drain turns the timeout into an ordinary completion.
void spin_until_published(volatile uint32_t *flag, uint32_t seq, hipStream_t s, const char *what) {
    const double kSpinSeconds = [] { const char *e = hooks::raw(hooks::SPIN_SECONDS); const double v = e ? std::atof(e) : 0.0; return v > 0.0 ? v : 120.0; }();
    int idle = 0;
    std::chrono::steady_clock::time_point t0;
    bool timed = false;
    for (unsigned spins = 1; *flag != seq; ++spins) {
        if ((spins & 0x3fff) == 0) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) { if (++idle > 64) throw HipError(std::string("internal: ") + what + " were not published"); }
            else if (q != hipErrorNotReady) hip_check(q, what);
            if (!timed) { t0 = std::chrono::steady_clock::now(); timed = true; }
            else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kSpinSeconds) {
                hip_check(hipStreamSynchronize(s), what);   // nothing may still be writing when the caller unwinds
                if (*flag == seq) break;
                throw HipError(std::string("timeout: ") + what + " did not arrive (stream drained, nothing published)");
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
}

// split_candidate_generator.cpp:216-249: n_bins+1 equal-count buckets, threshold i = value at rank cum_i - 1.  With fewer rows than buckets
// the remainder loop still gives the first n_samples buckets one row each, so cum_i = min(i + 1, n_samples) >= 1: the ranks repeat at the
// column maximum (the reference grows valid trees there).
std::vector<int64_t> quantile_target_ranks(long long n_global, int B) {
    std::vector<int64_t> cum(B);
    const long long per = n_global / (B + 1), rem = n_global % (B + 1);
    long long run = 0;
    for (int i = 0; i < B; ++i) { run += per + (i < rem ? 1 : 0); cum[i] = run; }
    return cum;
}

}  // namespace detail


// ---- A3/A4: numeric split candidates ------------------------------------------------------------------------------------
// thresholds [F][B] of the rows in dobs (keys already transposed into d_kt): fixed ones (fit()), uniform (min/max + fma), or
// exact quantiles (radix multi-select; sample-splitter selection and 32-pass bisection kept as cross-checks / fallbacks).
// On return d_thr / d_thrkeys hold them on the device (the caller copies them to the host when it needs them there).
// The quantile target ranks depend on (global row count, n_bins) only: uploaded when they change (an RL loop calls step() with the same
// batch size over and over; the upload from pageable memory costs ~70 us of host time per call), through pinned memory.
int64_t *Engine::quantile_cum_device(const std::vector<int64_t> &cum, long long n_global, int B) {
    hipStream_t s = stream_;
    const bool grown = d_cum_.capacity() < sizeof(int64_t) * static_cast<size_t>(B);
    int64_t *d_cum = static_cast<int64_t *>(d_cum_.ensure(sizeof(int64_t) * B));
    if (grown || cum_cache_n_ != n_global || cum_cache_b_ != B) {
        int64_t *h = static_cast<int64_t *>(pin_cum_.ensure(sizeof(int64_t) * B));
        std::memcpy(h, cum.data(), sizeof(int64_t) * B);
        hip_check(hipMemcpyAsync(d_cum, h, sizeof(int64_t) * B, hipMemcpyHostToDevice, s), "H2D cum");
        hip_check(hipStreamSynchronize(s), "sync cum");   // the pinned block may be rewritten by the next call
        cum_cache_n_ = n_global;
        cum_cache_b_ = B;
    }
    return d_cum;
}

// ---- the routes ------------------------------------------------------------------------------------------------------------------------
// exact MSD radix multi-select applies (prepare_numeric counts its first digit during the transpose when it will run)
bool Engine::radix_select_applies(int B, long long n_global) const {
    return !force_sample_select_ && B <= kern::radix_max_targets() && n_global < (1ll << 32);
}

detail::ThrRoute Engine::threshold_route(int N, int B, long long n_global) const {
    using detail::ThrRoute;
    if (!fixed_thr_.empty()) return ThrRoute::Fixed;
    if (model.meta.generator_type == GBRL_HIP_GEN_UNIFORM) return ThrRoute::Uniform;
    // the sharded sample selection needs a power-of-two world (union sample of world*4096 keys sorted in LDS)
    const bool coll_fast = has_coll_ && (coll_.world_size & (coll_.world_size - 1)) == 0 && coll_.world_size <= 8;
    const bool radix_ok = radix_select_applies(B, n_global);
    if (force_bisection_ || (has_coll_ && !coll_fast && !radix_ok)) return ThrRoute::Bisection;
    if (!has_coll_ && !force_sample_select_ && !force_radix_ && kern::sort_quantiles_fits(N, B)) return ThrRoute::LdsSort;
    return radix_ok ? ThrRoute::Radix : ThrRoute::Sample;
}

void Engine::numeric_thresholds(const float *dobs, int N, int F, int B, long long n_global, const uint32_t *d_kt, float *d_thr,
                                uint32_t *d_thrkeys, DevBuf &root_le_buf, const uint32_t **root_le_out, int pass1_chunks, uint16_t *d_codes_out,
                                bool *codes_written) {
    using detail::ThrRoute;
    if (codes_written) *codes_written = false;
    if (root_le_out) *root_le_out = nullptr;
    if (F <= 0) return;
    const detail::ThrArgs a{dobs, N, F, B, n_global, d_kt, d_thr, d_thrkeys};
    switch (threshold_route(N, B, n_global)) {
        case ThrRoute::Fixed: thresholds_fixed(a); break;
        case ThrRoute::Uniform: thresholds_uniform(a); break;
        case ThrRoute::Bisection: thresholds_bisection(a); break;
        case ThrRoute::LdsSort: { const bool wrote = thresholds_lds_sort(a, d_codes_out); if (codes_written) *codes_written = wrote; break; }
        case ThrRoute::Radix: { const uint32_t *le = thresholds_radix(a, root_le_buf, pass1_chunks); if (root_le_out) *root_le_out = le; break; }
        case ThrRoute::Sample: thresholds_sample(a); break;
    }
}

// fit(): the candidates were generated from the whole data set (fitter.cpp:134-150); this batch only bins against them
void Engine::thresholds_fixed(const detail::ThrArgs &a) {
    if (fixed_thr_.size() != static_cast<size_t>(a.F) * a.B) throw HipError("internal: fixed thresholds do not match this model");
    hip_check(hipMemcpyAsync(a.d_thr, fixed_thr_.data(), sizeof(float) * fixed_thr_.size(), hipMemcpyHostToDevice, stream_), "H2D thresholds");
    kern::floats_to_keys(a.d_thr, a.d_thrkeys, fixed_thr_.size(), stream_);
}

void Engine::thresholds_uniform(const detail::ThrArgs &a) {
    hipStream_t s = stream_;
    const int F = a.F;
    uint32_t *d_mm = static_cast<uint32_t *>(d_minmax_.ensure(sizeof(uint32_t) * 2 * F));
    kern::FillSegments fz{};
    fz.n = 2;
    fz.dst[0] = d_mm; fz.words[0] = static_cast<uint32_t>(F); fz.value[0] = 0xffffffffu;
    fz.dst[1] = d_mm + F; fz.words[1] = static_cast<uint32_t>(F); fz.value[1] = 0u;
    kern::fill_segments(fz, s);
    kern::column_minmax(a.d_kt, a.N, F, d_mm, d_mm + F, s);
    if (has_coll_) {
        // exchange as floats (max / min are exact)
        float *tmp = static_cast<float *>(d_trial_.ensure(sizeof(float) * 2 * F));
        kern::keys_to_floats(d_mm, tmp, 2 * static_cast<size_t>(F), s);
        kern::negate_f32(tmp, F, s);                 // min = -max(-x): minima and maxima in ONE max all-reduce
        exchange(Red::MaxF32, tmp, 2 * static_cast<size_t>(F));
        kern::negate_f32(tmp, F, s);
        kern::floats_to_keys(tmp, d_mm, 2 * static_cast<size_t>(F), s);
    }
    kern::uniform_thresholds(d_mm, d_mm + F, F, a.B, a.d_thr, s, a.d_thrkeys);
}

// exact but slow: 32 counting passes (also the multi-GPU path: only integer counts cross ranks)
void Engine::thresholds_bisection(const detail::ThrArgs &a) {
    hipStream_t s = stream_;
    const int F = a.F, B = a.B;
    int64_t *d_cum = quantile_cum_device(quantile_target_ranks(a.n_global, B), a.n_global, B);
    uint32_t *d_prefix = static_cast<uint32_t *>(d_prefix_.ensure(sizeof(uint32_t) * F * B));
    uint32_t *d_trial = static_cast<uint32_t *>(d_trial_.ensure(sizeof(uint32_t) * F * B));
    int64_t *d_counts = static_cast<int64_t *>(d_counts_.ensure(sizeof(int64_t) * F * (B + 1)));
    kern::qsel_init(d_prefix, d_trial, F, B, s);
    for (int bit = 31; bit >= 0; --bit) {
        hip_check(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * F * (B + 1), s), "memset");
        kern::bin_rows(a.dobs, a.N, F, d_trial, B, /*strict=*/false, d_counts, nullptr, 0, 0, s);
        if (has_coll_) exchange(Red::SumI64, d_counts, static_cast<size_t>(F) * (B + 1));
        kern::qsel_update(d_prefix, d_trial, d_counts, d_cum, F, B, bit, bit - 1, s);
    }
    hip_check(hipMemcpyAsync(a.d_thrkeys, d_trial, sizeof(uint32_t) * F * B, hipMemcpyDeviceToDevice, s), "D2D keys");
    kern::keys_to_floats(a.d_thrkeys, a.d_thr, static_cast<size_t>(F) * B, s);
}

// RL-sized batch: the column fits in LDS -- sort it and read the ranks (one launch; the kernel writes the floats itself, and the class
// codes of its feature: no separate binning launch)
bool Engine::thresholds_lds_sort(const detail::ThrArgs &a, uint16_t *d_codes_out) {
    int64_t *d_cum = quantile_cum_device(quantile_target_ranks(a.n_global, a.B), a.n_global, a.B);
    const bool no_fuse = [] { const char *e = hooks::raw(hooks::SORT_NO_CODES); return e && e[0] == '1'; }();   /* read per call: the tests flip it */   // test / measurement hook
    uint16_t *cdst = no_fuse ? nullptr : d_codes_out;
    kern::sort_quantiles(a.d_kt, a.N, a.F, d_cum, a.B, a.d_thrkeys, a.d_thr, stream_, cdst);
    last_quantile_fallback_ = false;
    return cdst != nullptr;
}

// exact MSD radix multi-select, four counting passes over the transposed keys (radix_select.hip).  Row-sharded runs sum the digit counts of
// every pass over ranks (any world size): 4 all-reduces per step.
const uint32_t *Engine::thresholds_radix(const detail::ThrArgs &a, DevBuf &root_le_buf, int pass1_chunks) {
    hipStream_t s = stream_;
    const int N = a.N, F = a.F, B = a.B;
    int64_t *d_cum = quantile_cum_device(quantile_target_ranks(a.n_global, B), a.n_global, B);
    void *d_rs = d_radix_state_.ensure(kern::radix_state_bytes(F, B));
    uint32_t *d_rp = static_cast<uint32_t *>(d_radix_partial_.ensure(kern::radix_partial_bytes(F)));
    uint32_t *d_rl = static_cast<uint32_t *>(d_qlists_.ensure(kern::radix_list_bytes(N, F)));
    kern::RadixComm comm{};
    if (has_coll_) {
        comm.ctx = this;
        comm.allreduce_sum_i64 = &Engine::radix_exchange_trampoline;
        comm.stream_ordered = rccl_comm_ != nullptr;
        comm.gbuf = static_cast<int64_t *>(d_counts_.ensure(sizeof(int64_t) * kern::radix_exchange_words(F)));
        comm.partial_global = static_cast<uint32_t *>(d_radix_global_.ensure(kern::radix_global_partial_bytes(F)));
    }
    // (one GPU: the selection also reports #{keys <= threshold}, from which the ROOT's class counts follow -- grow_tree, root_le)
    uint32_t *d_le = has_coll_ ? nullptr : static_cast<uint32_t *>(root_le_buf.ensure(sizeof(uint32_t) * (static_cast<size_t>(F) * B + F)));
    const int rc = kern::radix_select(a.d_kt, N, F, d_cum, B, d_rs, d_rp, d_rl, a.d_thrkeys, s, has_coll_ ? &comm : nullptr, pass1_chunks, d_le);
    if (rc != 0) throw HipError(rc == 2 ? "allreduce failed" : "radix select failed");
    last_quantile_fallback_ = false;
    kern::keys_to_floats(a.d_thrkeys, a.d_thr, static_cast<size_t>(F) * B, s);
    return d_le;
}

// Sample/splitter selection: splitters from a sample cut every column into classes, the classes that hold a target rank are extracted and
// the rank is selected inside them.  A class list that outgrows its budget (pathological value distribution) sends the step to the
// bisection instead: exact, slow.
void Engine::thresholds_sample(const detail::ThrArgs &a) {
    hipStream_t s = stream_;
    const int N = a.N, F = a.F, B = a.B;
    const uint32_t *d_kt = a.d_kt;
    uint32_t *d_thrkeys = a.d_thrkeys;
    uint32_t *d_qflags = static_cast<uint32_t *>(d_qflags_.ensure(sizeof(uint32_t) * 4));  // [0,1] allocator, [2] overflow
    kern::QuantilePlan plan = kern::quantile_plan(N);
    if (has_coll_) { plan.sample = 4096; plan.n_split = kern::kQuantileMaxSplit; }   // identical on every rank
    // budget of the extracted class lists: a quarter of the data is ample when the targets are few against the classes
    // (<= 256 targets, 1024 classes); with more targets nearly every class holds one, so the lists can be the whole data
    const size_t all_keys = static_cast<size_t>(N) * F;
    const uint32_t max_elems = static_cast<uint32_t>(B > 256 ? all_keys : std::min<size_t>(all_keys, std::max<size_t>(1u << 20, all_keys / 4)));
    int64_t *d_cum = quantile_cum_device(quantile_target_ranks(a.n_global, B), a.n_global, B);
    uint32_t *d_split = static_cast<uint32_t *>(d_splitters_.ensure(sizeof(uint32_t) * 2 * static_cast<size_t>(F) * kern::kQuantileMaxSplit));
    uint32_t *d_split_bfs = d_split + static_cast<size_t>(F) * kern::kQuantileMaxSplit;
    uint32_t *d_cc = static_cast<uint32_t *>(d_ccounts_.ensure(sizeof(uint32_t) * static_cast<size_t>(plan.n_chunks) * F * kern::kQuantileClasses));
    uint32_t *d_coff = static_cast<uint32_t *>(d_c2l_.ensure(sizeof(uint32_t) * F * kern::kQuantileClasses));
    uint32_t *d_toff = static_cast<uint32_t *>(d_tgt_list_.ensure(sizeof(uint32_t) * 2 * static_cast<size_t>(F) * B));
    uint32_t *d_tlen = d_toff + static_cast<size_t>(F) * B;
    uint32_t *d_tr = static_cast<uint32_t *>(d_tgt_rank_.ensure(sizeof(uint32_t) * F * B));
    uint32_t *d_lists = static_cast<uint32_t *>(d_qlists_.ensure(sizeof(uint32_t) * max_elems));
    hip_check(hipMemsetAsync(d_coff, 0xff, sizeof(uint32_t) * F * kern::kQuantileClasses, s), "memset");
    hip_check(hipMemsetAsync(d_qflags, 0, sizeof(uint32_t) * 4, s), "memset");
    int64_t *d_gcounts = nullptr;
    if (has_coll_) {
        // every rank contributes a 4096-key sample per feature; the union is sorted identically everywhere
        const int S = 4096, SU = S * coll_.world_size;
        uint32_t *d_samp = static_cast<uint32_t *>(d_prefix_.ensure(sizeof(uint32_t) * static_cast<size_t>(F) * S));
        int64_t *d_uni = static_cast<int64_t *>(d_counts_.ensure(sizeof(int64_t) * std::max<size_t>(static_cast<size_t>(F) * SU, static_cast<size_t>(F) * kern::kQuantileClasses)));
        kern::sample_only(d_kt, N, F, S, d_samp, s);
        hip_check(hipMemsetAsync(d_uni, 0, sizeof(int64_t) * static_cast<size_t>(F) * SU, s), "memset");
        kern::place_sample(d_samp, F, S, coll_.rank, SU, d_uni, s);
        exchange(Red::SumI64, d_uni, static_cast<size_t>(F) * SU);
        kern::union_splitters(d_uni, F, SU, plan.n_split, d_split, d_split_bfs, s);
        kern::class_count(d_kt, N, F, plan, d_split_bfs, d_cc, s);
        d_gcounts = d_uni;   // reuse (the union sample is consumed)
        kern::counts_to_i64(d_cc, plan.n_chunks, static_cast<size_t>(F) * kern::kQuantileClasses, d_gcounts, s);
        exchange(Red::SumI64, d_gcounts, static_cast<size_t>(F) * kern::kQuantileClasses);
    } else {
        kern::sample_splitters(d_kt, N, F, plan, d_split, d_split_bfs, s);
        hip_check(hipGetLastError(), "sample_splitters launch");
        kern::class_count(d_kt, N, F, plan, d_split_bfs, d_cc, s);
        hip_check(hipGetLastError(), "class_count launch");
    }
    kern::quantile_targets(d_cc, d_gcounts, d_split, d_cum, F, B, plan, d_coff, d_toff, d_tlen, d_tr, d_thrkeys, d_qflags, max_elems,
                           d_qflags + 2, s);
    kern::quantile_extract(d_kt, N, F, plan, d_split_bfs, d_coff, d_cc, d_lists, s);
    hip_check(hipGetLastError(), "quantile_extract launch");
    if (has_coll_) {
        // the lists stay on their ranks; the order statistic of their union is found by 32 counting rounds
        uint32_t *d_pref = static_cast<uint32_t *>(d_trial_.ensure(sizeof(uint32_t) * static_cast<size_t>(F) * B));
        int64_t *d_scnt = static_cast<int64_t *>(d_selcnt_.ensure(sizeof(int64_t) * (static_cast<size_t>(F) * B + 1)));
        hip_check(hipMemsetAsync(d_pref, 0, sizeof(uint32_t) * static_cast<size_t>(F) * B, s), "memset");
        for (int bit = 31; bit >= 0; --bit) {
            kern::select_count(d_lists, d_toff, d_tlen, d_pref, bit, F * B, d_scnt, s);
            hip_check(hipGetLastError(), "select_count launch");
            exchange(Red::SumI64, d_scnt, static_cast<size_t>(F) * B);
            kern::select_update(d_pref, d_scnt, d_toff, d_tr, bit, F * B, d_thrkeys, s);
            hip_check(hipGetLastError(), "select_update launch");
        }
    } else {
        kern::quantile_select(d_lists, d_toff, d_tlen, d_tr, F * B, d_thrkeys, s);
        hip_check(hipGetLastError(), "quantile_select launch");
    }
    kern::keys_to_floats(d_thrkeys, a.d_thr, static_cast<size_t>(F) * B, s);
    uint32_t qflags[4] = {0, 0, 0, 0};
    hip_check(hipMemcpyAsync(qflags, d_qflags, sizeof(qflags), hipMemcpyDeviceToHost, s), "D2H flags");
    hip_check(hipStreamSynchronize(s), "sync");
    bool fallback = qflags[2] != 0;
    if (has_coll_) fallback = all_ranks_agree(fallback, d_selcnt_);   // the fallback decision must be the same on every rank
    if (fallback) thresholds_bisection(a);
    last_quantile_fallback_ = fallback;
}

}  // namespace gbrl
