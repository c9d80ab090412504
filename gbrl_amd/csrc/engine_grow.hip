// engine_grow.hip -- Engine::grow_tree (see engine_grow_detail.h): one tree from the prepared candidates, class codes and quantised gradients.
// grow_tree uploads the step's constant tables and chooses the growth path: RL-sized steps in one launch (grow_small, k_small_grow), everything
// else level by level (grow_levels, engine_grow_levels.hip: A6-A10).  The host bookkeeping all paths share (TreeBuilder, chunk tables) is here too.
#include "engine_grow_detail.h"

namespace gbrl {
namespace detail {

GrowDims::GrowDims(const GrowCtx &c, bool has_coll, int world_size, int rank, Engine::Parity parity) {
    const int N = c.N, D = c.D, MD = c.MD, NB = c.NB, Fp = c.Fp;
    max_front = 1 << std::max(0, MD - 1);
    max_nodes = 2 * (1 << MD);
    max_chunks = std::max((N + 1023) / 1024, (N + kern::kPartitionRows - 1) / kern::kPartitionRows) + 2 * (1 << MD) + 2;
    l2_degenerate = !c.cosine && c.n_global < 2;
    table_cap = c.prefix_cacheable ? static_cast<size_t>(std::max(c.cand_cap, c.n_cand)) : static_cast<size_t>(c.n_cand);
    stage_bytes = 4096 + sizeof(FeatureSlot) * c.n_slots + table_cap * 16 + 5 * 256 +
                  sizeof(Chunk) * (static_cast<size_t>(max_chunks) + N / 4096 + 2 * max_nodes + 64) +
                  static_cast<size_t>(max_front) * (kern::kMaxPath * 12 + 256);
    hist_chunk_budget = std::max(32, 256 / std::max(1, c.n_groups));
    hist_max_chunks = std::max(hist_chunk_budget, (N + c.chunk_rows - 1) / c.chunk_rows) + 2 * (1 << MD) + 2;
    n_acc = static_cast<size_t>(NB) * (D + 1) * c.FG;
    hist_node_elems = static_cast<size_t>(Fp) * NB * (D + 1);
    feat_elems = static_cast<size_t>(NB) * (D + 1);
    coll_P = has_coll ? std::max(1, world_size) : 1;
    coll_Fs = (Fp + coll_P - 1) / coll_P;
    coll_lo = has_coll ? rank * coll_Fs : 0;
    own_slots = has_coll ? std::max(0, std::min(c.n_slots, coll_lo + coll_Fs) - coll_lo) : c.n_slots;
    const char *ar_env = hooks::raw(hooks::HIST_ALLREDUCE_MAX_KB);
    ar_max_bytes = static_cast<size_t>(ar_env ? std::max(0L, std::atol(ar_env)) : 10240L) * 1024;
    am_parts = kern::argmax_parts(std::max(1, c.n_cand));
    am_cap = static_cast<size_t>(max_front) * std::max(am_parts, std::max(1, c.n_slots));
    res_bytes = ResultBlock::bytes(max_front);
    const char *rel_env = hooks::raw(hooks::NEARTIE_REL), *max_env = hooks::raw(hooks::NEARTIE_MAX_ROWS);
    near_rel = rel_env ? static_cast<float>(std::atof(rel_env)) : 9.5367431640625e-07f;
    // The model's parity setting, then the two hooks over it: each hook that is set does exactly what it did before the setting existed.
    Engine::ParityMode mode = parity.mode;
    int limit = parity.max_node_rows;
    if (max_env && N > kern::kNearMaxRows) { mode = Engine::ParityMode::Reference; limit = std::max(0, std::atoi(max_env)); }
    if (hooks::on(hooks::NO_NEARTIE_REPLAY)) mode = Engine::ParityMode::ExactArgmax;
    near_max_rows = N <= kern::kNearMaxRows ? 0 : (mode == Engine::ParityMode::Reference ? limit : -1);
    near_on = mode != Engine::ParityMode::ExactArgmax && !has_coll && c.n_global == N && c.n_cand > 0 && kern::near_tie_supported(N, D) && near_max_rows >= 0;
    reference_asked = parity.mode == Engine::ParityMode::Reference && mode == Engine::ParityMode::Reference;
    event_results = hooks::on(hooks::EVENT_RESULTS);
}

ChunkTable make_chunks(const std::vector<HNode> &nodes, const std::vector<int> &ids, int rows_per_chunk, bool slot_is_node_id) {
    ChunkTable t;
    t.begin.assign(1, 0);
    for (size_t k = 0; k < ids.size(); ++k) {
        const HNode &nd = nodes[ids[k]];
        if (slot_is_node_id && nd.depth == 0) { t.begin.push_back(static_cast<int32_t>(t.chunks.size())); continue; }  // Q7
        // equal parts (no short remainder chunk): parts = ceil(n / rows_per_chunk), each ceil(n / parts) rows
        const int parts = (nd.n_local + rows_per_chunk - 1) / rows_per_chunk;
        const int each = parts ? (nd.n_local + parts - 1) / parts : 0;
        for (int off = 0; off < nd.n_local; off += each)
            t.chunks.push_back({static_cast<int32_t>(slot_is_node_id ? ids[k] : static_cast<int>(k)), nd.seg_start + off,
                                std::min(each, nd.n_local - off), 0});
        t.begin.push_back(static_cast<int32_t>(t.chunks.size()));
    }
    return t;
}

int balanced_chunk_rows(const std::vector<HNode> &nodes, const std::vector<int> &ids, int chunk_rows, int budget) {
    int lo = 1024, hi = chunk_rows;
    auto parts_at = [&](int t) { long long p = 0; for (int id : ids) p += (nodes[id].n_local + t - 1) / t; return p; };
    if (parts_at(hi) > budget) return hi;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (parts_at(mid) <= budget) hi = mid; else lo = mid + 1;
    }
    return hi;
}

int CatIndex::find(const std::vector<CatCandidate> &cat_cands, int Fc, int feat, int cls) {
    if (off.empty()) {
        off.assign(static_cast<size_t>(Fc) + 1, 0);
        for (const CatCandidate &cc : cat_cands) off[cc.feat + 1] = std::max(off[cc.feat + 1], cc.cls);
        for (int f = 0; f < Fc; ++f) off[f + 1] += off[f];
        index.assign(static_cast<size_t>(off[Fc]), -1);
        for (size_t z = 0; z < cat_cands.size(); ++z)
            if (cat_cands[z].cls >= 1) index[off[cat_cands[z].feat] + cat_cands[z].cls - 1] = static_cast<int>(z);
    }
    if (feat < 0 || feat >= Fc || cls < 1 || cls > off[feat + 1] - off[feat]) return -1;
    return index[off[feat] + cls - 1];
}

void TreeBuilder::reset(int max_nodes) {
    nodes.clear();
    nodes.reserve(max_nodes);
    nodes.push_back(HNode{});
    nodes[0].n_local = c_.N;
    nodes[0].n_global = c_.n_global;
    frontier.assign(1, 0);
    in_cond_.clear();
}

std::vector<int> TreeBuilder::active_nodes() const {
    std::vector<int> active;
    for (int id : frontier)
        if (c_.oblivious || nodes[id].n_global > 0) active.push_back(id);
    return active;
}

// Host bookkeeping of one level from its result block: decisions, children, paths.
LevelOutcome TreeBuilder::digest_level(const std::vector<int> &active, const ResultBlock &res, const DigestMode &mode) {
    LevelOutcome out;
    const bool oblivious = c_.oblivious;
    const std::vector<FeatureSlot> &slots = *c_.slots;
    const int n_act = static_cast<int>(active.size());
    const int32_t *best_idx_h = res.best_idx();
    const float *best_score_h = res.best_score();
    const int64_t *tot_g = res.total(), *right_g = res.right();
    const int64_t *right_l = row_sharded_ ? res.right_local() : right_g;
    if (oblivious && best_score_h[0] == -INFINITY) { out.stop = true; return out; }  // fitter.cpp:458
    // -- decisions (best_idx are REFERENCE candidate indices)
    std::vector<NodeSplit> sp(n_act);
    std::vector<int> &splitting = out.splitting, &new_leaves = out.new_leaves;
    for (int k = 0; k < n_act; ++k) {
        HNode &nd = nodes[active[k]];
        const int bk = oblivious ? 0 : k;
        const bool do_split = oblivious || best_score_h[bk] >= 0.0f;  // fitter.cpp:357
        NodeSplit q{};
        q.seg_start = nd.seg_start;
        if (do_split) {
            const int j = (*c_.ref_to_internal)[best_idx_h[bk]];
            const int fs = (*c_.cand_slot)[j];
            q.do_split = 1;
            q.fslot = fs;
            q.is_cat = slots[fs].is_cat;
            q.bin = slots[fs].is_cat ? (j - slots[fs].cand_base + 1) : (j - slots[fs].cand_base);
            splitting.push_back(k);
        } else {
            nd.leaf = true;
            new_leaves.push_back(active[k]);
        }
        sp[k] = q;
    }
    if (!oblivious)
        for (int id : frontier)
            if (nodes[id].n_global == 0 && !nodes[id].leaf) { nodes[id].leaf = true; new_leaves.push_back(id); }
    std::vector<int> &next = out.next;
    for (int k : splitting) {
        const int id = active[k];
        if (!mode.counts_later && tot_g[k] != nodes[id].n_global) throw HipError("internal: histogram row count mismatch");
        const NodeSplit &q = sp[k];
        HCond c{};
        c.fslot = q.fslot;
        c.is_cat = q.is_cat != 0;
        c.bin = q.bin;
        if (c.is_cat) {
            c.feat_idx = q.fslot - c_.F;
            c.value = INFINITY;
            c.cat_cand = cat_index_.find(*c_.cat_cands, c_.Fc, c.feat_idx, q.bin);
        } else {
            c.feat_idx = q.fslot;
            c.value = mode.win_thr ? mode.win_thr[k] : c_.h_thr[static_cast<size_t>(q.fslot) * c_.B + q.bin];
            c.cat_cand = -1;
        }
        const long long npar = nodes[id].n_global, nr = right_g[k], nl = npar - nr;
        HNode l, r;
        l.depth = r.depth = nodes[id].depth + 1;
        l.parent = r.parent = id;
        HCond cl = c, cr = c;
        cl.dir = false;
        cl.edge_w = npar > 0 ? static_cast<float>(nl) / static_cast<float>(npar) : 0.0f;  // node.cpp:131
        cr.dir = true;
        cr.edge_w = npar > 0 ? static_cast<float>(nr) / static_cast<float>(npar) : 0.0f;
        if (mode.lazy_paths) {   // (one-launch growth: only the leaves' paths are ever read -- built once, at the end, from the conditions that lead INTO the nodes)
            if (in_cond_.empty()) in_cond_.reserve(nodes.capacity());
            in_cond_.resize(nodes.size() + 2);
            in_cond_[nodes.size()] = cl;
            in_cond_[nodes.size() + 1] = cr;
        } else {
            l.path = nodes[id].path;
            r.path = nodes[id].path;
            l.path.push_back(cl);
            r.path.push_back(cr);
        }
        const int nl_local = static_cast<int>(nodes[id].n_local - right_l[k]);
        l.seg_start = nodes[id].seg_start;
        l.n_local = nl_local;
        l.n_global = nl;
        r.seg_start = nodes[id].seg_start + nl_local;
        r.n_local = static_cast<int>(right_l[k]);
        r.n_global = nr;
        sp[k].n_left = nl_local;
        nodes[id].left = static_cast<int>(nodes.size());
        nodes.push_back(l);
        nodes[id].right = static_cast<int>(nodes.size());
        nodes.push_back(r);
        next.push_back(nodes[id].left);
        next.push_back(nodes[id].right);
    }
    return out;
}

void TreeBuilder::finish_small(const int64_t *h_acc, uint32_t kernel_nodes, std::vector<int64_t> &acc) {
    const int N = c_.N, D = c_.D;
    in_cond_.resize(nodes.size());
    for (int id : frontier)
        if (!nodes[id].leaf) nodes[id].leaf = true;
    if (nodes.size() == 1) nodes[0].leaf = true;
    if (nodes.size() != static_cast<size_t>(kernel_nodes)) throw HipError("internal: the growth kernel numbered " + std::to_string(kernel_nodes) + " nodes, the replay " + std::to_string(nodes.size()));
    acc.assign(nodes.size() * (D + 1), 0);
    for (size_t id = 0; id < nodes.size(); ++id)
        if (nodes[id].left < 0) std::memcpy(&acc[id * (D + 1)], h_acc + id * (D + 1), sizeof(int64_t) * (D + 1));
    if (c_.oblivious && nodes.size() > 1) {
        // An oblivious level keeps both children of every node, so the kernel never counts them: a node's size is the sum of its leaves'
        // row counts (bottom-up: children have higher ids than their parent), and the edge weights follow (node.cpp:131).
        std::vector<long long> cnt(nodes.size(), 0);
        for (size_t id = nodes.size(); id-- > 0;)
            cnt[id] = nodes[id].left < 0 ? acc[id * (D + 1) + D] : cnt[nodes[id].left] + cnt[nodes[id].right];
        if (cnt[0] != N) throw HipError("internal: the leaves of the grown tree hold " + std::to_string(cnt[0]) + " of " + std::to_string(N) + " rows");
        for (size_t id = 0; id < nodes.size(); ++id) {
            HNode &nd = nodes[id];
            nd.n_global = cnt[id];
            nd.n_local = static_cast<int>(cnt[id]);
            if (id > 0) in_cond_[id].edge_w = cnt[nd.parent] > 0 ? static_cast<float>(cnt[id]) / static_cast<float>(cnt[nd.parent]) : 0.0f;
        }
    }
    for (size_t id = 0; id < nodes.size(); ++id) {   // the leaves' paths (what append_tree writes into the model), root first
        HNode &nd = nodes[id];
        if (nd.left >= 0 || nd.depth == 0) continue;
        nd.path.resize(nd.depth);
        int at = static_cast<int>(id);
        for (int d = nd.depth - 1; d >= 0; --d) { nd.path[d] = in_cond_[at]; at = nodes[at].parent; }
    }
}

}  // namespace detail

using namespace detail;

// ---- the tree of one step: on return `nodes` is the tree, `frontier` the unsplit nodes of the last level, acc the per-node int64
// fixed-point sums of the raw gradients (| count) and leaf_scale their scale.
void Engine::grow_tree(const GrowCtx &c, std::vector<HNode> &nodes, std::vector<int> &frontier, std::vector<int64_t> &acc, double &leaf_scale) {
    const GrowDims dims(c, has_coll_, coll_.world_size, coll_.rank, parity_);
    if (dims.reference_asked && c.n_cand > 0) {
        // "reference" is a promise about the result, so a step that cannot replay says so instead of growing the exact arg-max's tree quietly.
        // Nothing has been booked yet: the model is as it was before the call.
        if (!dims.near_on) throw Unsupported("parity mode \"reference\": the near-tie replay does not support this shape (at most 2^30 rows, output_dim <= 1024)");
        if (dims.event_results) throw Unsupported("parity mode \"reference\": GBRL_HIP_EVENT_RESULTS=1 reads the level results without the near-tie replay; unset it or use another parity mode");
        if (c.oblivious && device_levels_requested()) throw Unsupported("parity mode \"reference\": GBRL_HIP_DEVICE_LEVELS=1 grows oblivious trees without the near-tie replay; unset it or use another parity mode");
    }
    const StepTables tables = upload_step_tables(c, dims);
    TreeBuilder tb(c, has_coll_, nodes, frontier);
    // RL-sized steps on one GPU grow the whole tree in ONE launch (kern::small_grow, small_grow.hip): no level buffers, no partials,
    // no row lists.  GBRL_HIP_NO_SMALL_GROW=1 (tests / measurement): the level loop for every shape.
    const bool small_applies = !has_coll_ && !hooks::on(hooks::NO_SMALL_GROW) && c.n_global == c.N && c.n_cand > 0 && !dims.l2_degenerate && c.MD >= 1 &&
                               !(c.oblivious && device_levels_requested()) && kern::small_grow_supported(c.N, c.D, c.NB, c.MD, c.n_slots, c.n_cand);
    const int small_blocks = small_applies ? kern::small_grow_blocks(c.n_slots) : 0;
    if (small_blocks > 0 && !small_grow_off_) {
        const char *why = nullptr;
        switch (grow_small(c, dims, tables, small_blocks, tb, acc, leaf_scale, why)) {
        case SmallGrowth::Grown:
            return;
        case SmallGrowth::Unavailable:
            // The one-launch kernel is an optimisation, never a requirement: when it cannot be launched (LDS budget, device attributes) or its
            // blocks abandon a grid barrier (they were not co-resident: another process, stream or model held CUs / LDS), nothing has been
            // booked yet, so the level loop grows this tree, and this engine keeps to it from now on.
            sg_sync_ptr_ = nullptr;           // (the barrier words are in an unknown state)
            small_grow_off_ = true;
            ++small_grow_fallbacks_;
            if (model.meta.verbose > 0) fprintf(stderr, "gbrl_hip: %s; this model grows its trees level by level from now on\n", why);
            break;
        case SmallGrowth::NearTie:
            // a level of this tree has a near-tie: the level loop grows it, with the candidates in the window re-scored in the reference's order
            ++near_bailouts_;
            break;
        }
    }
    grow_levels(c, dims, tables, tb, acc, leaf_scale);
}

// ---- per-step constants on the device: slots, candidate weights / reference order / slot lookup (once per tree; a tree that falls back
// from the one-launch growth to the level loop reuses the addresses) ---------------------------------------------------------------
StepTables Engine::upload_step_tables(const GrowCtx &c, const GrowDims &dims) {
    hipStream_t s = stream_;
    const std::vector<FeatureSlot> &slots = *c.slots;
    const std::vector<float> &cand_w = *c.cand_w;
    const std::vector<int32_t> &cand_ref = *c.cand_ref, &cand_slot = *c.cand_slot;
    const std::vector<int> &ref_to_internal = *c.ref_to_internal;
    const size_t table_cap = dims.table_cap, stage_bytes = dims.stage_bytes;
    Stager stc(pin_const_, d_stage_const_, stage_bytes, s);
    StepTables t{};
    static_assert(sizeof(int) == sizeof(int32_t), "ref_to_internal is uploaded as int32");
    if (c.prefix_cacheable) {
        // fixed layout (capacity (F + Fc) * n_bins entries per table): the numeric prefixes are uploaded once per layout, every step
        // uploads the slot table and the four categorical tails
        const size_t np = static_cast<size_t>(c.n_num_cand), nt = static_cast<size_t>(c.n_cand) - np;
        const bool have_prefix = step_const_.dev_base == stc.device_base() && step_const_.stage_bytes == stage_bytes;
        t.slots = stc.reserve<FeatureSlot>(slots.size());
        t.cand_w = stc.reserve<float>(table_cap);
        t.cand_ref = stc.reserve<int32_t>(table_cap);
        t.ref_to_internal = stc.reserve<int32_t>(table_cap);
        t.cand_slot = stc.reserve<int32_t>(table_cap);
        char *hb = stc.host_base();
        const char *db = static_cast<const char *>(stc.device_base());
        auto mirror = [&](const void *dptr) -> char * { return hb + (static_cast<const char *>(dptr) - db); };
        void *hb_dev = nullptr;
        hip_check(hipHostGetDevicePointer(&hb_dev, hb, 0), "hipHostGetDevicePointer");
        kern::FetchSegments fs{};
        static_assert(sizeof(FeatureSlot) % 4 == 0, "fetched as 32-bit words");
        auto up = [&](void *dptr, const void *src, size_t first, size_t count, size_t elem) {   // one kernel fetches all five from the pinned mirror
            if (!count) return;
            char *hm = mirror(dptr) + first * elem;
            std::memcpy(hm, static_cast<const char *>(src) + first * elem, count * elem);
            fs.dst[fs.n] = static_cast<char *>(dptr) + first * elem;
            fs.src[fs.n] = static_cast<const char *>(hb_dev) + (hm - hb);
            fs.words[fs.n] = static_cast<uint32_t>(count * elem / 4);
            ++fs.n;
        };
        const size_t lo = have_prefix ? np : 0, cnt = have_prefix ? nt : static_cast<size_t>(c.n_cand);
        up(t.slots, slots.data(), 0, slots.size(), sizeof(FeatureSlot));
        up(t.cand_w, cand_w.data(), lo, cnt, 4);
        up(t.cand_ref, cand_ref.data(), lo, cnt, 4);
        up(t.ref_to_internal, ref_to_internal.data(), lo, cnt, 4);
        up(t.cand_slot, cand_slot.data(), lo, cnt, 4);
        kern::fetch_segments(fs, s);
        step_const_.dev_base = stc.device_base();
        step_const_.stage_bytes = stage_bytes;
    } else if (c.const_cacheable && step_const_.dev_base == stc.device_base() && step_const_.stage_bytes == stage_bytes) {
        t.slots = stc.reserve<FeatureSlot>(slots.size());          // uploaded by an earlier step, same layout
        t.cand_w = stc.reserve<float>(cand_w.size());
        t.cand_ref = stc.reserve<int32_t>(cand_ref.size());
        t.ref_to_internal = reinterpret_cast<int32_t *>(stc.reserve<int>(ref_to_internal.size()));
        t.cand_slot = stc.reserve<int32_t>(cand_slot.size());
    } else {
        t.slots = stc.put(slots.data(), slots.size());
        t.cand_w = stc.put(cand_w.data(), cand_w.size());
        t.cand_ref = stc.put(cand_ref.data(), cand_ref.size());
        t.ref_to_internal = reinterpret_cast<int32_t *>(stc.put(ref_to_internal.data(), ref_to_internal.size()));
        t.cand_slot = stc.put(cand_slot.data(), cand_slot.size());
        stc.flush();
        if (c.const_cacheable) { step_const_.dev_base = stc.device_base(); step_const_.stage_bytes = stage_bytes; }
    }
    return t;
}

// ---- RL-sized steps: ONE launch grows the tree, ONE wait, then the bookkeeping is replayed from the per-level result blocks -------
// Grown: the tree is in `tb`, `acc`, `leaf_scale`.  NearTie / Unavailable (`why` says what failed): nothing has been booked.
Engine::SmallGrowth Engine::grow_small(const GrowCtx &c, const GrowDims &dims, const StepTables &t, int blocks, TreeBuilder &tb, std::vector<int64_t> &acc,
                                       double &leaf_scale, const char *&why) {
    hipStream_t s = stream_;
    const int N = c.N, F = c.F, D = c.D, MD = c.MD;
    const bool oblivious = c.oblivious;
    const size_t res_stride = kern::small_grow_res_stride(MD);
    const size_t res_all = res_stride * MD;
    const size_t acc_words = static_cast<size_t>(2u << MD) * (D + 1);
    const size_t o_acc = (res_all + 255) & ~static_cast<size_t>(255), o_status = o_acc + sizeof(int64_t) * acc_words;
    char *h_blk = static_cast<char *>(pin_res_all_.ensure(o_status + 64 + 64));
    void *h_blk_dev = nullptr;
    hip_check(hipHostGetDevicePointer(&h_blk_dev, h_blk, 0), "hipHostGetDevicePointer");
    char *d_blk = static_cast<char *>(h_blk_dev);
    volatile uint32_t *h_status = reinterpret_cast<volatile uint32_t *>(h_blk + o_status);
    unsigned *d_sync = static_cast<unsigned *>(d_sg_sync_.ensure(4096));
    if (d_sync != sg_sync_ptr_) {
        hip_check(hipMemsetAsync(d_sync, 0, 4096, s), "memset barrier words");
        sg_sync_ptr_ = d_sync;
    }
    kern::SmallGrowIO io{};
    io.codes = c.d_codes; io.codes_fm = c.d_codes_fm; io.n_fm = c.d_codes_fm ? F : 0; io.n_thr_slots = F; io.qg = c.d_qg; io.grads = c.dgrads; io.scales = c.d_scales; io.slots = t.slots; io.thr = c.d_thr; io.cand_w = t.cand_w; io.cand_ref = t.cand_ref;
    io.N = N; io.D = D; io.B = c.B; io.n_slots = c.n_slots; io.NB = c.NB; io.MD = MD; io.min_data = model.meta.min_data_in_leaf; io.cosine = c.cosine; io.oblivious = oblivious;
    io.G = blocks;
    io.bests = d_sg_bests_.ensure(kern::small_grow_bests_bytes(MD, blocks, oblivious));
    io.sync = d_sync;
    io.res = d_blk; io.res_dev = static_cast<char *>(d_res_all_.ensure(res_all)); io.acc = reinterpret_cast<int64_t *>(d_blk + o_acc); io.status = reinterpret_cast<uint32_t *>(d_blk + o_status);
    uint32_t seq = next_seq();
    io.seq = seq;
    io.scales_out = reinterpret_cast<kern::StepScales *>(c.pub_scales_dev);
    io.near_rel = dims.near_on ? dims.near_rel : 0.0f;
    if (dims.near_on) { io.near_scratch = d_sg_near_.ensure(kern::small_grow_near_bytes(blocks, N, MD)); io.meanden = c.d_meanden; }
    const bool sg_prof = hooks::on(hooks::SMALL_GROW_PROF);   // measurement hook
    if (sg_prof) io.prof = reinterpret_cast<uint32_t *>(d_blk + o_status + 64);
    h_status[0] = 0;
    const int sg_fail = hooks::num(hooks::TEST_SMALL_GROW_FAIL, 0);   // test hook (1: launch failure, 2: abandoned barrier)
    phase_begin();
    if (sg_fail == 1 || !kern::small_grow(io, s)) {
        (void)hipGetLastError();
        why = "the one-launch growth kernel could not be launched";
        return SmallGrowth::Unavailable;
    }
    phase_end("small_grow");
    const auto t_launched = std::chrono::steady_clock::now();
    verify_pending_categories();   // (host work hidden behind the kernel)
    spin_until_published(h_status, seq, s, "small-step tree");
    const auto t_seen = std::chrono::steady_clock::now();
    hip_check(hipGetLastError(), "growth kernel");
    if (h_status[3] == 2 && !io.replay) {
        // a level of this tree has a near-tie: the kernel variant that replays a flagged node itself grows the tree once more (the
        // default variant only detects: the replay code inside it slows every step, small_grow.hip)
        io.replay = true;
        io.resume = h_status[5] == 1;     // (the default variant left its state: only the flagged level's second pass and what follows run again)
        seq = next_seq();
        io.seq = seq;
        h_status[0] = 0;
        phase_begin();
        if (!kern::small_grow(io, s)) {
            (void)hipGetLastError();
            why = "the one-launch growth kernel (near-tie replay variant) could not be launched";
            return SmallGrowth::Unavailable;
        }
        phase_end("small_grow");
        spin_until_published(h_status, seq, s, "small-step tree (near-tie replay)");
        hip_check(hipGetLastError(), "growth kernel");
    }
    near_in_kernel_ += h_status[4];
    if (h_status[3] == 2) return SmallGrowth::NearTie;
    if (h_status[3] != 0 || sg_fail == 2) {
        why = "the one-launch growth kernel gave up at a grid barrier (its blocks were not co-resident)";
        return SmallGrowth::Unavailable;
    }
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    if (sg_prof) {
        static const char *names[14] = {"codes", "zero", "accumulate", "scan", "carries", "score", "select", "slot_best", "barrier", "winners", "tables", "route", "level_end", "leaves"};
        const volatile uint32_t *pw = reinterpret_cast<const volatile uint32_t *>(h_blk + o_status + 64);
        std::string line = "[small_grow block 0, us]";
        for (int i = 0; i < 14; ++i) line += std::string(" ") + names[i] + " " + std::to_string(pw[i] / 100.0).substr(0, 5);
        fprintf(stderr, "%s\n", line.c_str());
        fprintf(stderr, "[small step host, us] inputs+cat launch %.1f  preparation enqueued %.1f  categorical candidates (host) %.1f  tables + cat codes %.1f  grow_tree to launch %.1f\n",
                us(prof_step_entry_, prof_marks_[0]), us(prof_marks_[0], prof_marks_[1]), us(prof_marks_[1], prof_marks_[2]), us(prof_marks_[2], prof_marks_[3]), us(prof_marks_[3], t_launched));
    }
    // the bookkeeping, replayed from the per-level result blocks
    tb.reset(dims.max_nodes);
    const int levels_written = static_cast<int>(h_status[1]);
    for (int depth = 0; depth < MD; ++depth) {
        const std::vector<int> active = tb.active_nodes();
        if (active.empty()) break;
        if (depth >= levels_written) throw HipError("internal: the growth kernel wrote fewer levels than the replay needs");
        const ResultBlock res{h_blk + static_cast<size_t>(depth) * res_stride, static_cast<size_t>(dims.max_front)};
        LevelOutcome lvl = tb.digest_level(active, res, DigestMode{res.win_thr(), /*lazy_paths=*/true, /*counts_later=*/oblivious});
        if (lvl.stop) break;
        if (lvl.splitting.empty()) { tb.frontier.clear(); break; }
        tb.frontier = lvl.next;
    }
    tb.finish_small(reinterpret_cast<const int64_t *>(h_blk + o_acc), h_status[2], acc);
    if (!std::isfinite(c.h_scales->hmax_build) || !std::isfinite(c.h_scales->hmax_raw)) throw InvalidArgument("non-finite gradients");
    leaf_scale = c.h_scales->leaf_scale;
    if (sg_prof) fprintf(stderr, "[small step host, us] entry->growth launched %.1f  wait %.1f  replay %.1f\n", us(prof_step_entry_, t_launched), us(t_launched, t_seen), us(t_seen, std::chrono::steady_clock::now()));
    return SmallGrowth::Grown;
}

}  // namespace gbrl
