// engine_cat_candidates.hip -- a step's categorical split candidates (A5; see engine_step_detail.h): the device scan for the batch's distinct cells in
// stages (tables, insert + verify, publish, collect, the on-device ranking round, the row-sharded gather), the host replay of the reference's
// container (cat_candidates_host.h) and the two forms of its result (the scan's tables, a dictionary); the row-sharded mean-gradient ranking.
#include "engine_step_detail.h"

namespace gbrl {

using detail::CatList;
using detail::CatMemory;
using detail::CatPub;
using detail::CatScan;

namespace {

// Table and list sizes of this step's scan; false: beyond what the scan holds (the host rules decide).
// The per-feature tables are sized for the worst case (every row a new category: 4 N slots); real columns hold a few dozen
// categories, so the step starts with four times the largest distinct count the previous step saw and repeats with the full size
// only if a table overflowed (12 MB of memsets and atomics on a 12 MB table -> 0.2 MB at configs[4]).
bool scan_plan(CatScan &c, int N, int Fc, int B) {
    if (static_cast<long long>(Fc) * B > (1 << 20)) return false;
    c.full_log2 = 8;
    while ((1ll << c.full_log2) < 4ll * N && c.full_log2 < 20) ++c.full_log2;   // (every row of a column may be a category of its own: they are ranked later)
    if ((static_cast<size_t>(Fc) << c.full_log2) >= (1ull << 31)) return false;   // list records are 32-bit table slots
    c.log2_cap = std::min(c.full_log2, std::max(8, c.log2_hint));
    // the list holds EVERY distinct cell (up to 2^21): a batch with more of them than candidates are kept is ranked on the device (kern::cat_rank)
    c.list_cap = static_cast<int>(std::min<long long>(static_cast<long long>(N) * Fc, 1ll << 21));
    c.meta.ensure(sizeof(int32_t) * 4);               // flags[2], counter
    c.lslot.ensure(sizeof(int32_t) * c.list_cap);
    return true;
}

// the per-feature tables at the current size, cleared (with the flags and the counter)
void scan_tables(CatScan &c, int Fc, hipStream_t s) {
    const size_t slots = static_cast<size_t>(Fc) << c.log2_cap;
    uint64_t *d_keys = static_cast<uint64_t *>(c.keys.ensure(sizeof(uint64_t) * slots));
    int32_t *d_first = static_cast<int32_t *>(c.first.ensure(sizeof(int32_t) * slots));
    int32_t *d_meta = c.meta.as<int32_t>();
    if (slots <= (size_t(1) << 22)) {   // the usual few-KiB tables: one launch clears all three
        kern::FillSegments fz{};
        fz.n = 3;
        fz.dst[0] = d_keys; fz.words[0] = static_cast<uint32_t>(2 * slots); fz.value[0] = 0u;
        fz.dst[1] = d_first; fz.words[1] = static_cast<uint32_t>(slots); fz.value[1] = 0x7f7f7f7fu;
        fz.dst[2] = d_meta; fz.words[2] = 4; fz.value[2] = 0u;
        kern::fill_segments(fz, s);
    } else {
        hip_check(hipMemsetAsync(d_keys, 0, sizeof(uint64_t) * slots, s), "memset");
        hip_check(hipMemsetAsync(d_first, 0x7f, sizeof(int32_t) * slots, s), "memset");
        hip_check(hipMemsetAsync(d_meta, 0, sizeof(int32_t) * 4, s), "memset");
    }
}

void scan_insert(CatScan &c, const char *dcells, int N, int Fc, hipStream_t s) {
    int32_t *d_meta = c.meta.as<int32_t>();
    kern::cat_distinct_insert(dcells, N, Fc, c.keys.as<uint64_t>(), c.first.as<int32_t>(), c.log2_cap, d_meta, c.lslot.as<int32_t>(), d_meta + 2, c.list_cap, s);
    kern::cat_distinct_verify(dcells, N, Fc, c.keys.as<uint64_t>(), c.first.as<int32_t>(), c.log2_cap, d_meta, s);
}

// the published block in mapped pinned memory: [64-byte header | hash | feature | first row | the cells | count | total], `cap` records each
struct PubLayout {
    size_t o_hash, o_feat, o_first, o_names, o_cnt, o_tot, bytes;
    explicit PubLayout(int cap) {
        const size_t n = static_cast<size_t>(cap);
        o_hash = 64; o_feat = o_hash + 8 * n; o_first = o_feat + 4 * n;
        o_names = o_first + 4 * n;   // 64 + 16 cap: 16-byte aligned
        o_cnt = o_names + static_cast<size_t>(kCat) * n; o_tot = o_cnt + 4 * n; bytes = 64 + n * (8 + 4 + 4 + kCat + 4 + 4);
    }
};
volatile uint32_t *pub_flag(char *h) { return reinterpret_cast<volatile uint32_t *>(h) + 4; }   // header word 4: written last, by the last block

// ONE launch writes header + records + the distinct cells themselves into mapped pinned memory, ONE synchronisation reads them.  The record
// count is guessed from the last step; a larger batch of distinct cells is published again with the exact count.
void publish_launch(CatScan &c, const char *dcells, int Fc, int cap, CatPub mode, hipStream_t s) {
    const PubLayout o(cap);
    char *h = static_cast<char *>(c.pin.ensure(o.bytes));
    void *dv = nullptr;
    hip_check(hipHostGetDevicePointer(&dv, h, 0), "hipHostGetDevicePointer");
    char *d = static_cast<char *>(dv);
    *pub_flag(h) = 0;
    int32_t *d_slotq = static_cast<int32_t *>(c.slotq.ensure(sizeof(int32_t) * (static_cast<size_t>(Fc) << c.log2_cap)));
    const bool stats = mode != CatPub::Records;
    kern::cat_publish(c.meta.as<int32_t>(), c.lslot.as<int32_t>(), c.keys.as<uint64_t>(), c.first.as<int32_t>(), c.log2_cap, dcells, Fc, cap, reinterpret_cast<int32_t *>(d),
                      reinterpret_cast<int32_t *>(d + o.o_feat), reinterpret_cast<int32_t *>(d + o.o_first), reinterpret_cast<uint64_t *>(d + o.o_hash),
                      mode == CatPub::StatsOnly ? nullptr : d + o.o_names, d_slotq, ++c.pub_seq, s, stats ? c.rank_cnt.as<int32_t>() : nullptr,
                      stats ? c.rank_tot.as<float>() : nullptr, reinterpret_cast<int32_t *>(d + o.o_cnt), reinterpret_cast<float *>(d + o.o_tot));
}

// one round of the scan on the stream: tables, insert + verify, publish
void scan_round(CatScan &c, const char *dcells, int N, int Fc, hipStream_t s) {
    scan_tables(c, Fc, s);
    scan_insert(c, dcells, N, Fc, s);
    c.pub_cap = std::min(c.list_cap, std::max(256, c.publish_guess));
    publish_launch(c, dcells, Fc, c.pub_cap, CatPub::Records, s);
}

// Waits for the publish launched last (the publish only: kernels enqueued behind it keep running) and returns a view of its block.
// The device wrote these lines over PCIe, so every first touch by the host misses its caches: ONE sequential pass (prefetcher friendly) into
// ordinary memory, sized by the published count, instead of the replay's scattered reads (3x slower measured).  The 128-byte cells -- 260 KiB
// of the 290 at configs[4] -- are NOT copied on one GPU: a cell the engine has met before is recognised by its 64-bit hash and feature, and its
// bytes are compared with the remembered ones later, while the device grows the tree (verify_pending_categories); only new cells are read.
CatList publish_collect(CatScan &c, int cap, CatPub mode, bool copy_names, hipStream_t s) {
    const PubLayout o(cap);
    char *h = static_cast<char *>(c.pin.ensure(o.bytes));
    spin_until_published(pub_flag(h), c.pub_seq, s, "the batch's distinct categorical cells");
    const bool stats = mode != CatPub::Records;
    const size_t n_pub = static_cast<size_t>(std::max(0, std::min(reinterpret_cast<const int32_t *>(h)[3], cap)));
    c.host.resize(64 + n_pub * (8 + 4 + 4 + (copy_names ? kCat : 0) + (stats ? 8 : 0)));
    char *m = c.host.data();
    const size_t c_hash = 64, c_feat = c_hash + 8 * n_pub, c_first = c_feat + 4 * n_pub, c_names = c_first + 4 * n_pub,
                 c_cnt = c_names + (copy_names ? static_cast<size_t>(kCat) * n_pub : 0), c_tot = c_cnt + 4 * n_pub;
    std::memcpy(m, h, 64);
    std::memcpy(m + c_hash, h + o.o_hash, 8 * n_pub);
    std::memcpy(m + c_feat, h + o.o_feat, 4 * n_pub);
    std::memcpy(m + c_first, h + o.o_first, 4 * n_pub);
    if (copy_names) std::memcpy(m + c_names, h + o.o_names, static_cast<size_t>(kCat) * n_pub);
    CatList l{};
    if (stats) {
        std::memcpy(m + c_cnt, h + o.o_cnt, 4 * n_pub);
        std::memcpy(m + c_tot, h + o.o_tot, 4 * n_pub);
        l.count = reinterpret_cast<const int32_t *>(m + c_cnt);
        l.total = reinterpret_cast<const float *>(m + c_tot);
    }
    l.hdr = reinterpret_cast<const int32_t *>(m);
    l.hash = reinterpret_cast<const uint64_t *>(m + c_hash);
    l.feat = reinterpret_cast<const int32_t *>(m + c_feat);
    l.first = reinterpret_cast<const int32_t *>(m + c_first);
    l.names = copy_names ? m + c_names : h + o.o_names;
    l.names_in_pinned = !copy_names;
    return l;
}

// one upload that nothing waits for: the next write of the pinned block happens behind the next step's synchronisation
void fetch_pinned(void *dst, void *pinned, size_t words, hipStream_t s) {
    void *dev = nullptr;
    hip_check(hipHostGetDevicePointer(&dev, pinned, 0), "hipHostGetDevicePointer");
    kern::FetchSegments fs{};
    fs.n = 1; fs.dst[0] = dst; fs.src[0] = dev; fs.words[0] = static_cast<uint32_t>(words);
    kern::fetch_segments(fs, s);
}

// Ordinary step on one GPU: the scan's tables ARE the dictionary; the host hands back the class of every list record only.
void result_table(CatScan &c, const CatMemory &mem, const CatList &l, const CatMemory::Replay &rp, int n_distinct, bool overflow,
                  std::vector<CatCandidate> &cat_cands, std::vector<int> &cat_classes, hipStream_t s) {
    const size_t n1 = static_cast<size_t>(std::max(1, n_distinct));
    int32_t *hc = static_cast<int32_t *>(c.pin_cls.ensure(sizeof(int32_t) * n1));
    if (overflow) std::fill(hc, hc + n_distinct, 0);   // a category that is not kept: class 0
    // (the remembered bytes: equal to the published cell's, verified at once or in verify_pending_categories)
    detail::assign_classes(rp.cand_item.size(), [&](size_t k) { const int q = rp.cand_item[k]; return std::make_pair(static_cast<int>(l.feat[q]), static_cast<const char *>(mem.item(rp.item_of_q[q]).name)); },
                           cat_cands, cat_classes, [&](size_t k, int cls) { hc[rp.cand_item[k]] = cls; });
    int32_t *dc = static_cast<int32_t *>(c.clsq.ensure(sizeof(int32_t) * n1));
    fetch_pinned(dc, hc, n1, s);
    c.table.valid = true; c.table.keys = c.keys.as<uint64_t>(); c.table.slot_q = c.slotq.as<int32_t>(); c.table.cls_of_q = dc; c.table.log2_cap = c.log2_cap;
}

// Row-sharded steps and fit(): candidates + the step's dictionary (per feature: entries sorted by raw hash, then class), packed into ONE
// pinned block.
void result_dict(CatScan &c, const CatMemory &mem, const CatList &l, const CatMemory::Replay &rp, int Fc, std::vector<CatCandidate> &cat_cands,
                 std::vector<int> &cat_classes, hipStream_t s) {
    struct DictE { uint64_t h; int cls; int item; };
    const int n_ent = static_cast<int>(rp.cand_item.size());
    std::vector<DictE> ent(n_ent);
    std::vector<int32_t> off(Fc + 1, 0);
    for (int q : rp.cand_item) ++off[l.feat[q] + 1];
    for (int f = 0; f < Fc; ++f) off[f + 1] += off[f];
    std::vector<int32_t> cur(off.begin(), off.end() - 1);
    detail::assign_classes(rp.cand_item.size(), [&](size_t k) { const int q = rp.cand_item[k]; return std::make_pair(static_cast<int>(l.feat[q]), static_cast<const char *>(mem.item(rp.item_of_q[q]).name)); },
                           cat_cands, cat_classes, [&](size_t k, int cls) { const int q = rp.cand_item[k]; ent[cur[l.feat[q]]++] = {l.hash[q], cls, q}; });
    for (int f = 0; f < Fc; ++f)
        std::sort(ent.begin() + off[f], ent.begin() + off[f + 1], [](const DictE &a, const DictE &b2) { return a.h < b2.h || (a.h == b2.h && a.cls < b2.cls); });
    const size_t n1 = static_cast<size_t>(n_ent) + 1;   // one zero entry behind the last: the arrays are never empty
    const size_t o_words = 0, o_hash = o_words + n1 * kCat, o_off = o_hash + n1 * 8, o_cls = o_off + (static_cast<size_t>(Fc) + 1) * 4,
                 dict_bytes = o_cls + n1 * 4;
    char *hd = static_cast<char *>(c.pin_dict.ensure((dict_bytes + 3) & ~static_cast<size_t>(3)));
    for (int e = 0; e < n_ent; ++e) {
        std::memcpy(hd + o_words + static_cast<size_t>(e) * kCat, l.names + static_cast<size_t>(ent[e].item) * kCat, kCat);
        reinterpret_cast<uint64_t *>(hd + o_hash)[e] = ent[e].h;
        reinterpret_cast<int32_t *>(hd + o_cls)[e] = ent[e].cls;
    }
    std::memset(hd + o_words + static_cast<size_t>(n_ent) * kCat, 0, kCat);
    reinterpret_cast<uint64_t *>(hd + o_hash)[n_ent] = 0;
    reinterpret_cast<int32_t *>(hd + o_cls)[n_ent] = 0;
    std::memcpy(hd + o_off, off.data(), (static_cast<size_t>(Fc) + 1) * 4);
    char *dd = static_cast<char *>(c.sdict.ensure((dict_bytes + 3) & ~static_cast<size_t>(3)));
    fetch_pinned(dd, hd, (dict_bytes + 3) / 4, s);
    c.dict.words = reinterpret_cast<const uint64_t *>(dd + o_words);
    c.dict.hash = reinterpret_cast<const uint64_t *>(dd + o_hash);
    c.dict.off = reinterpret_cast<const int32_t *>(dd + o_off);
    c.dict.cls = reinterpret_cast<const int32_t *>(dd + o_cls);
}

}  // namespace

// step() enqueues the scan (tables, insert, verify, publish) BEFORE the gradient statistics, the numeric candidates and the numeric binning,
// none of which depend on it; collect_categorical_candidates polls the publish kernel's own completion word, so the host's replay of the
// reference's container (~0.1 ms at configs[4]) runs while the device works through the numeric preparation instead of in front of an idle
// device (0.17 ms per 4096-row step, profiles/r04_cfg5_timeline_*.txt).
bool Engine::enqueue_categorical_scan(const char *dcells, int N, int Fc, int B) {
    cat_.launched = false;   // (a step that threw between the two stages must not be resumed)
    if (!scan_plan(cat_, N, Fc, B)) return false;
    scan_round(cat_, dcells, N, Fc, stream_);
    cat_.launched = true;
    return true;
}

// More distinct cells than candidates are kept, one GPU: count and total of every distinct cell are computed on the device (kern::cat_rank)
// and published beside the list.  false: a cell was not found in its table (cannot happen) -- the host scan decides.
bool Engine::cat_rank_round(const char *dcells, int N, int Fc, const float *dgrads, int D, int n_distinct, CatList &list) {
    hipStream_t s = stream_;
    phase_begin(/*key=*/true);
    void *d_scr = cat_.rank.ensure(kern::cat_rank_scratch_bytes(N, Fc, n_distinct));
    int32_t *d_rcnt = static_cast<int32_t *>(cat_.rank_cnt.ensure(sizeof(int32_t) * static_cast<size_t>(n_distinct)));
    float *d_rtot = static_cast<float *>(cat_.rank_tot.ensure(sizeof(float) * static_cast<size_t>(n_distinct)));
    int32_t *d_slotq = static_cast<int32_t *>(cat_.slotq.ensure(sizeof(int32_t) * (static_cast<size_t>(Fc) << cat_.log2_cap)));
    kern::cat_rank(dcells, N, Fc, dgrads, D, cat_.keys.as<uint64_t>(), cat_.log2_cap, cat_.meta.as<int32_t>(), cat_.lslot.as<int32_t>(), n_distinct, d_slotq, d_scr, d_rcnt, d_rtot, s);
    const bool all_here = n_distinct <= list.hdr[3];   // every record has arrived already: only 8 bytes per distinct cell travel now
    const int cap = all_here ? cat_.pub_cap : n_distinct;
    const CatPub mode = all_here ? CatPub::StatsOnly : CatPub::RecordsAndStats;
    publish_launch(cat_, dcells, Fc, cap, mode, s);
    phase_end("cat_rank", /*key=*/true);
    list = publish_collect(cat_, cap, mode, has_coll_, s);
    return list.hdr[0] == 0 && list.hdr[2] == n_distinct;
}

// Row-sharded: every rank needs the distinct cells of ALL ranks, in the order a single process would meet them (rank after rank = global
// row order): 18-word records (feature, first row, the 128 bytes), this rank's in its insertion order.  The global lists (kept in `store`)
// replace the local views.
void Engine::cat_gather_sharded(CatList &list, std::vector<int> &order, int &n_distinct, std::vector<char> &store) {
    std::vector<int64_t> mine(static_cast<size_t>(n_distinct) * 18, 0);
    for (int q = 0; q < n_distinct; ++q) {
        int64_t *r18 = &mine[static_cast<size_t>(q) * 18];
        r18[0] = list.feat[order[q]];
        r18[1] = list.first[order[q]];
        std::memcpy(r18 + 2, list.names + static_cast<size_t>(order[q]) * kCat, kCat);
    }
    const std::vector<int64_t> rec = all_gather_records(mine, 18, size_t(1) << 20);
    // global list, already rank-major and (feature, first row)-sorted inside a rank: stable sort by feature keeps that order
    n_distinct = static_cast<int>(rec.size() / 18);
    store.resize(static_cast<size_t>(n_distinct) * (8 + 4 + kCat));   // [hash | feature | the cells]
    uint64_t *g_hash = reinterpret_cast<uint64_t *>(store.data());
    int32_t *g_feat = reinterpret_cast<int32_t *>(store.data() + 8 * static_cast<size_t>(n_distinct));
    char *g_names = store.data() + 12 * static_cast<size_t>(n_distinct);
    for (int q = 0; q < n_distinct; ++q) {
        const int64_t *r18 = &rec[static_cast<size_t>(q) * 18];
        g_feat[q] = static_cast<int32_t>(r18[0]);
        std::memcpy(g_names + static_cast<size_t>(q) * kCat, r18 + 2, kCat);
        uint64_t w[16];
        std::memcpy(w, r18 + 2, kCat);
        g_hash[q] = cat_cell_hash_raw(w);
    }
    list.feat = g_feat; list.hash = g_hash; list.names = g_names; list.first = nullptr; list.names_in_pinned = false;
    order.resize(n_distinct);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return list.feat[a] < list.feat[b2]; });
}

// Collects the scan and builds the step's candidates: the distinct cells are inserted into the reference's container in the reference's
// insertion order on the host => same candidate order (Q8).  false: declined -- the host rules on every cell decide.
bool Engine::collect_categorical_candidates(const char *dcells, int N, int Fc, int B, const float *dgrads, int D, std::vector<CatCandidate> &cat_cands,
                                            std::vector<int> &cat_classes) {
    hipStream_t s = stream_;
    if (!cat_.launched) return false;   // declined at its sizes
    cat_.launched = false;
    const long long keep = static_cast<long long>(Fc) * B;
    CatList list = publish_collect(cat_, cat_.pub_cap, CatPub::Records, has_coll_, s);
    if (list.hdr[0] != 0 && cat_.log2_cap < cat_.full_log2) {   // a table (or the list) overflowed: once more at full size
        cat_.log2_cap = cat_.full_log2;
        scan_round(cat_, dcells, N, Fc, s);
        list = publish_collect(cat_, cat_.pub_cap, CatPub::Records, has_coll_, s);
    }
    const bool cat_prof = [] { const char *e = hooks::raw(hooks::CAT_PROF); return e && e[0] == '1'; }();   // measurement hook
    std::chrono::steady_clock::time_point cp[5];
    if (cat_prof) cp[0] = std::chrono::steady_clock::now();
    int n_distinct = list.hdr[2];
    // More distinct cells than candidates are kept: the reference ranks them by mean gradient norm (split_candidate_generator.cpp:131-150).
    // One GPU: cat_rank_round.  Row-sharded: declined (sharded_categorical_ranking).
    const bool overflow = n_distinct > keep;
    const bool can_rank = !has_coll_ && dgrads != nullptr && D > 0 && n_distinct <= cat_.list_cap && kern::cat_rank_fits(N, Fc);
    bool declined = list.hdr[0] != 0 || list.hdr[1] != 0 || (overflow && !can_rank);
    if (has_coll_) declined = all_ranks_agree(declined, cat_.xchg);
    if (declined) return false;
    if (overflow) {
        if (!cat_rank_round(dcells, N, Fc, dgrads, D, n_distinct, list)) return false;
    } else if (n_distinct > list.hdr[3]) {
        publish_launch(cat_, dcells, Fc, n_distinct, CatPub::Records, s);
        list = publish_collect(cat_, n_distinct, CatPub::Records, has_coll_, s);
    }
    cat_.publish_guess = n_distinct + n_distinct / 4 + 64;
    detail::FirstOccurrence fo = detail::first_occurrence_order(list.feat, list.first, n_distinct, N, Fc);
    cat_.log2_hint = 8;                       // table size the next step starts with
    while ((1 << cat_.log2_hint) < 4 * fo.max_per_feature && cat_.log2_hint < 20) ++cat_.log2_hint;
    std::vector<char> gathered;
    if (has_coll_) cat_gather_sharded(list, fo.order, n_distinct, gathered);
    if (cat_prof) cp[1] = std::chrono::steady_clock::now();
    CatMemory::Replay rp = cat_mem_.replay(fo.order, list.feat, list.hash, list.names, n_distinct, list.names_in_pinned, cat_prof ? &cp[2] : nullptr);
    if (cat_prof) cp[3] = std::chrono::steady_clock::now();
    // The replay leans on libstdc++ internals.  Production processes check it against the real container on their FIRST categorical
    // steps (eight of them: the early ones have the fewest rehashes) and then trust it; GBRL_HIP_CAT_CHECK=1 (the test suite) checks
    // every step, =0 never.  A disagreement is an error, not a silent reordering of the candidates.
    const int check_mode = [] { const char *e = hooks::raw(hooks::CAT_CHECK); return e ? (e[0] == '1' ? 1 : (e[0] == '0' ? 0 : 2)) : 2; }();
    static std::atomic<int> checks_left{8};
    const bool check_replay = check_mode == 1 || (check_mode == 2 && !fo.order.empty() && checks_left.load(std::memory_order_relaxed) > 0 &&
                                                   checks_left.fetch_sub(1, std::memory_order_relaxed) > 0);
    if (check_replay && !detail::replay_matches_container(fo.order, list.feat, list.names, rp.cand_item))
        throw HipError("categorical candidates: the hash-replay order differs from the string-keyed container's");
    if (overflow && !has_coll_ && static_cast<long long>(rp.cand_item.size()) > keep) {
        // (key, mean) in the container's iteration order; mean = float32 total / float(count), total bit-identical to the reference's
        // row-order sum (kern::cat_rank)
        std::vector<std::pair<int, float>> vec;
        vec.reserve(rp.cand_item.size());
        for (int q : rp.cand_item) vec.emplace_back(q, list.total[q] / static_cast<float>(list.count[q]));
        detail::keep_top_by_mean(vec, static_cast<size_t>(keep));
        rp.cand_item.resize(static_cast<size_t>(keep));
        for (size_t k = 0; k < rp.cand_item.size(); ++k) rp.cand_item[k] = vec[k].first;
    }
    if (static_cast<long long>(rp.cand_item.size()) > keep)
        throw Unsupported("more distinct categories than Fc * n_bins in a row-sharded step (the reference's mean-gradient ranking is not available sharded)");
    cat_.table.valid = false;
    if (has_coll_ || candidates_only_) {
        result_dict(cat_, cat_mem_, list, rp, Fc, cat_cands, cat_classes, s);
        return true;
    }
    result_table(cat_, cat_mem_, list, rp, n_distinct, overflow, cat_cands, cat_classes, s);
    if (cat_prof) {
        cp[4] = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[cat host, us] %d distinct: insertion order %.1f  items %.1f  container order %.1f  candidates + classes %.1f\n", n_distinct, us(cp[0], cp[1]), us(cp[1], cp[2]), us(cp[2], cp[3]), us(cp[3], cp[4]));
    }
    return true;
}

// A categorical cell that the replay recognised by (feature, 64-bit hash) alone: its 128 bytes, still in the pinned block the device published
// them to, are compared with the remembered ones HERE -- called while the device grows the tree, so the 260 KiB of PCIe-written lines are read
// off the critical path.  A difference means two categories share a 64-bit hash: step() grows the tree again on the host scan.
void Engine::verify_pending_categories() {
    if (cat_mem_.verify_pending(hooks::on(hooks::TEST_CAT_CLASH))) cat_clash_ = true;   // (test hook: pretend a remembered cell's bytes differ)
}

// More distinct cells than candidates are kept in a row-sharded step: the reference's rule on every cell (detail::categorical_candidates)
// with the distinct cells, their counts and their row-order float32 totals gathered over ranks.
void Engine::sharded_categorical_ranking(const char *hcat, const float *hgrads, int N, int Fc, int D, int B,
                                         std::vector<detail::CatCandidate> &cat_cands, std::vector<uint16_t> &h_catcodes, std::vector<int> &cat_classes) {
    const int world = coll_.world_size, rank = coll_.rank;
    const std::vector<float> norms = detail::squared_norms(hgrads, N, D);
    // (1) local scan: local id of every cell, distinct pairs in local first-occurrence order (feature-major)
    std::unordered_map<std::string, int> local_id;
    std::vector<int> l_feat;
    std::vector<std::string> l_name;
    std::vector<int32_t> cell_lid(static_cast<size_t>(N) * Fc);
    for (int f = 0; f < Fc; ++f)
        for (int i = 0; i < N; ++i) {
            std::string name(hcat + (static_cast<size_t>(i) * Fc + f) * kCat, kCat);
            auto it = local_id.emplace(name + "_" + std::to_string(f), static_cast<int>(l_feat.size()));
            if (it.second) { l_feat.push_back(f); l_name.push_back(std::move(name)); }
            cell_lid[static_cast<size_t>(i) * Fc + f] = it.first->second;
        }
    // (2) global list of distinct pairs: 17-word records (feature, the 128 bytes) in rank order
    std::vector<int64_t> mine(l_feat.size() * 17, 0);
    for (size_t q = 0; q < l_feat.size(); ++q) {
        mine[q * 17] = l_feat[q];
        std::memcpy(&mine[q * 17 + 1], l_name[q].data(), kCat);
    }
    const std::vector<int64_t> all = all_gather_records(mine, 17, (size_t(1) << 24) / 17);   // (2^24 words)
    const size_t n_rec = all.size() / 17;
    // the reference inserts feature-major, then in row order: stable sort of the rank-major list by feature
    std::vector<int> order(n_rec);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return all[static_cast<size_t>(a) * 17] < all[static_cast<size_t>(b) * 17]; });
    struct Info { float total = 0.f; long long count = 0; int feat = 0; std::string name; int gid = -1; };
    std::unordered_map<std::string, Info> uniq;   // same container, same insertion sequence as the reference => same iteration order (Q8)
    std::vector<std::string> gkey;                // global id -> key
    for (int q : order) {
        const int f = static_cast<int>(all[static_cast<size_t>(q) * 17]);
        std::string name(reinterpret_cast<const char *>(&all[static_cast<size_t>(q) * 17 + 1]), kCat);
        std::string key = name + "_" + std::to_string(f);
        auto it = uniq.find(key);
        if (it == uniq.end()) {
            Info ci;
            ci.feat = f; ci.name = std::move(name); ci.gid = static_cast<int>(gkey.size());
            gkey.push_back(key);
            uniq.emplace(std::move(key), std::move(ci));
        }
    }
    const size_t G = gkey.size();
    std::vector<int> lid_to_gid(l_feat.size());
    for (size_t q = 0; q < l_feat.size(); ++q) lid_to_gid[q] = uniq[l_name[q] + "_" + std::to_string(l_feat[q])].gid;
    // counts: exact integer all-reduce
    std::vector<int64_t> cnts(std::max<size_t>(G, 1), 0);
    for (size_t c = 0; c < cell_lid.size(); ++c) ++cnts[lid_to_gid[cell_lid[c]]];
    allreduce_host(Red::SumI64, cnts.data(), cnts.size(), cat_.xchg);
    // (3) totals: float32 sums in GLOBAL row order, one rank at a time.  The reference's loop is feature-major over ALL rows, but a key
    // belongs to one feature, so per key the order of its additions is simply the global row order.
    std::vector<double> tot(std::max<size_t>(G, 1), 0.0);   // transported as doubles (exact for float32 values), summed with zeros
    for (int r = 0; r < world; ++r) {
        std::vector<double> send(tot.size(), 0.0);
        if (r == rank) {
            std::vector<float> t32(tot.size());
            for (size_t k = 0; k < tot.size(); ++k) t32[k] = static_cast<float>(tot[k]);
            for (int f = 0; f < Fc; ++f)
                for (int i = 0; i < N; ++i) {
                    float &t = t32[lid_to_gid[cell_lid[static_cast<size_t>(i) * Fc + f]]];
                    t += norms[i];
                }
            for (size_t k = 0; k < tot.size(); ++k) send[k] = static_cast<double>(t32[k]);
        }
        allreduce_host(Red::SumF64, send.data(), send.size(), cat_.xchg);
        tot.swap(send);
    }
    for (auto &kv : uniq) { kv.second.total = static_cast<float>(tot[kv.second.gid]); kv.second.count = cnts[kv.second.gid]; }
    // (4) the reference's ranking (split_candidate_generator.cpp:131-161)
    std::vector<std::pair<std::string, float>> vec;
    for (const auto &kv : uniq) vec.emplace_back(kv.first, kv.second.total / static_cast<float>(static_cast<int>(kv.second.count)));
    detail::keep_top_by_mean(vec, static_cast<size_t>(Fc) * B);
    std::vector<int> cls_of_gid(std::max<size_t>(G, 1), 0);
    detail::assign_classes(vec.size(), [&](size_t k) { const Info &ci = uniq[vec[k].first]; return std::make_pair(ci.feat, ci.name.data()); },
                           cat_cands, cat_classes, [&](size_t k, int cls) { cls_of_gid[uniq[vec[k].first].gid] = cls; });
    h_catcodes.assign(static_cast<size_t>(N) * Fc, 0);
    for (size_t c = 0; c < cell_lid.size(); ++c) h_catcodes[c] = static_cast<uint16_t>(cls_of_gid[lid_to_gid[cell_lid[c]]]);
}

}  // namespace gbrl
