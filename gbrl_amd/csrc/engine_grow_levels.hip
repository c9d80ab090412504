// engine_grow_levels.hip -- Engine::grow_levels (see engine_grow_detail.h): level-by-level growth of one tree (A6-A10), for every step the
// one-launch growth does not take.  Two loops over one workspace -- the level-synchronous host loop (grow_levels_host: stage_level,
// level_histograms, score_select_level, replay_near_ties) and the opt-in device-planned oblivious loop (grow_levels_planned) -- then the
// leaf sums of the last level and their publication (finish_leaves).
#include "engine_grow_detail.h"

namespace gbrl {

using namespace detail;

void Engine::grow_levels(const GrowCtx &c, const GrowDims &dims, const StepTables &t, TreeBuilder &tb, std::vector<int64_t> &acc, double &leaf_scale) {
    hipStream_t s = stream_;
    // Oblivious trees on one GPU, opt-in (GBRL_HIP_DEVICE_LEVELS=1): the whole tree is enqueued without a host round trip per level.
    // Measured (round 2, profiles/r02_device_levels.txt): the planner launch (~10 us) and the empty blocks of the worst-case grids cost
    // what the host round trip (~30 us, partly hidden behind the partition) costs -- 2.301 vs 2.307 ms per step at 2^20 x 128, and
    // 0.64 vs 0.59 ms at 4096 x 128 -- so the level-synchronous host loop stays the default; the test suite checks that both grow the same bytes.
    const bool device_plan = c.oblivious && !has_coll_ && device_levels_requested() && c.MD > 0 && c.MD <= 11 /* k_plan_oblivious: <= 1024 nodes per level */ &&
                             c.n_cand > 0 && !dims.l2_degenerate;
    Stager sta(pin_a_, d_stage_a_, dims.stage_bytes, s), stb(pin_b_, d_stage_b_, dims.stage_bytes, s);
    LevelWork w = level_workspace(c, dims);
    // No synchronisation here: thresholds and scales are on their way to pinned memory; the first level's wait (or the final
    // synchronisation) covers them.  Non-finite gradients are rejected after the loop, before anything joins the model.
    tb.reset(dims.max_nodes);
    kern::publish_pair(c.d_thr, c.pub_thr_dev, c.pub_thr_bytes, c.d_scales, c.pub_scales_dev, sizeof(kern::StepScales), s);
    if (device_plan) grow_levels_planned(c, dims, t, w, tb);
    else if (c.n_cand > 0 && !dims.l2_degenerate) grow_levels_host(c, dims, t, w, tb, sta, stb);
    finish_leaves(c, dims, w, tb, sta, acc, leaf_scale);
}

// The level loops' buffers at their real sizes, and what has to be on the stream before the first level: clean leaf accumulators, a
// zero publication counter, the root's row list.
LevelWork Engine::level_workspace(const GrowCtx &c, const GrowDims &dims) {
    hipStream_t s = stream_;
    const int N = c.N, D = c.D, max_front = dims.max_front;
    LevelWork w{};
    w.rows[0] = static_cast<int32_t *>(d_rows_[0].ensure(sizeof(int32_t) * N));
    w.rows[1] = static_cast<int32_t *>(d_rows_[1].ensure(sizeof(int32_t) * N));
    w.partials = static_cast<int32_t *>(d_hist_partials_.ensure(sizeof(int32_t) * static_cast<size_t>(dims.hist_max_chunks) * c.n_groups * dims.n_acc));
    w.hist_lvl[0] = static_cast<int64_t *>(d_hist_.ensure(sizeof(int64_t) * max_front * dims.hist_node_elems));
    w.hist_lvl[1] = static_cast<int64_t *>(d_hist_prev_.ensure(sizeof(int64_t) * max_front * dims.hist_node_elems));
    if (has_coll_) {
        w.hist_coll = static_cast<int64_t *>(d_hist_local_.ensure(sizeof(int64_t) * max_front * static_cast<size_t>(dims.coll_P) * dims.coll_Fs * dims.feat_elems));
        w.hist_recv = static_cast<int64_t *>(d_hist_recv_.ensure(sizeof(int64_t) * max_front * static_cast<size_t>(dims.coll_Fs) * dims.feat_elems));
        w.gather = static_cast<int64_t *>(d_gather_.ensure(sizeof(int64_t) * static_cast<size_t>(dims.coll_P) * 3 * max_front));
    }
    w.ar_prefix = has_coll_;
    w.scores = static_cast<float *>(d_scores_.ensure(sizeof(float) * static_cast<size_t>(max_front) * std::max(1, c.n_cand)));
    w.parent = static_cast<float *>(d_parent_.ensure(sizeof(float) * max_front));
    w.am_v = static_cast<float *>(d_am_v_.ensure(sizeof(float) * dims.am_cap));
    w.am_i = static_cast<int32_t *>(d_am_i_.ensure(sizeof(int32_t) * dims.am_cap));
    w.am_s = dims.near_on ? static_cast<float *>(d_am_s_.ensure(sizeof(float) * dims.am_cap * 2)) : nullptr;
    w.am_n = (w.am_s && N > 8192) ? reinterpret_cast<int32_t *>(w.am_s + dims.am_cap) : nullptr;
    w.cursors = static_cast<int32_t *>(d_cursors_.ensure(sizeof(int32_t) * max_front * 2));
    {   // leaf accumulators: zero unless the last tree's publication handed these words back clean
        const size_t need = sizeof(int64_t) * dims.max_nodes * (D + 1);
        w.leafacc = static_cast<int64_t *>(d_leafacc_.ensure(need));
        if (!(leafacc_clean_ptr_ == w.leafacc && need <= leafacc_clean_bytes_))
            hip_check(hipMemsetAsync(w.leafacc, 0, need, s), "memset leaf acc");
        leafacc_clean_ptr_ = nullptr;     // dirty until the end of this tree
        leafacc_clean_bytes_ = need;
    }
    w.d_res = ResultBlock{static_cast<char *>(d_results_.ensure(dims.res_bytes)), static_cast<size_t>(max_front)};
    w.h_res = ResultBlock{static_cast<char *>(pin_res_.ensure(dims.res_bytes + 64)), static_cast<size_t>(max_front)};
    w.h_flag = reinterpret_cast<volatile uint32_t *>(w.h_res.base + dims.res_bytes);
    hip_check(hipHostGetDevicePointer(&w.h_res_dev, w.h_res.base, 0), "hipHostGetDevicePointer");
    w.d_flag = reinterpret_cast<uint32_t *>(static_cast<char *>(w.h_res_dev) + dims.res_bytes);
    *w.h_flag = 0;   // nothing is in flight here; a freshly allocated block must not hold a stale sequence number
    w.d_pub_done = static_cast<unsigned *>(d_pub_done_.ensure(256));
    if (w.d_pub_done != pub_done_ptr_) {
        hip_check(hipMemsetAsync(w.d_pub_done, 0, 256, s), "memset publication counter");
        pub_done_ptr_ = w.d_pub_done;
    }
    w.resolved = static_cast<NodeSplit *>(d_splits_.ensure(sizeof(NodeSplit) * max_front));
    // The root's row list 0 .. N-1 is kept between steps (generated again only when N outgrows it): level 0 reads it in place of
    // rows[0] and, after the first partition, rows[0] becomes the second scratch list again.  The device-planned loop partitions INTO
    // rows[depth parity] and keeps generating its own: it must never be handed the cached list.
    w.rows_scratch = w.rows[0];
    if (!(c.oblivious && device_levels_requested()) && !hooks::on(hooks::NO_IOTA_CACHE) /* measurement hook */) {
        int32_t *d_iota = static_cast<int32_t *>(d_rows_iota_.ensure(sizeof(int32_t) * N));
        if (d_iota != iota_ptr_ || iota_n_ < N) {
            kern::iota_rows(d_iota, N, s);
            iota_ptr_ = d_iota;
            iota_n_ = N;
        }
        w.rows[0] = d_iota;
        w.iota_root = true;
    } else {
        kern::iota_rows(w.rows[0], N, s);
    }
    return w;
}

// ---- the device-planned oblivious loop: k_plan_oblivious builds every level's descriptors on the device from the previous level's resolved
// splits; the consumers run on worst-case grids (unused chunk entries have len 0).  The host synchronises ONCE, reads all levels' result
// blocks and replays the bookkeeping (digest_level).
void Engine::grow_levels_planned(const GrowCtx &c, const GrowDims &dims, const StepTables &t, LevelWork &w, TreeBuilder &tb) {
    hipStream_t s = stream_;
    const int N = c.N, D = c.D, B = c.B, MD = c.MD, NB = c.NB, FG = c.FG, Fp = c.Fp, n_groups = c.n_groups, n_cand = c.n_cand;
    const int mf = dims.max_front;
    const size_t res_bytes = dims.res_bytes;
    const int cap_h = dims.hist_chunk_budget + mf + 2;
    const int cap_p = (N + kern::kPartitionRows - 1) / kern::kPartitionRows + mf + 2;
    if (cap_h > dims.hist_max_chunks) throw HipError("internal: chunk table overflow");
    // carve the plan out of one device block
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~static_cast<size_t>(255); return o; };
    const size_t o_seg = take(sizeof(int32_t) * (MD + 1) * mf), o_n = take(sizeof(int32_t) * (MD + 1) * mf);
    const size_t o_chunks = take(sizeof(Chunk) * cap_h), o_cb = take(sizeof(int32_t) * (mf + 2));
    const size_t o_sm = take(sizeof(int32_t) * mf), o_sp = take(sizeof(int32_t) * mf), o_ss = take(sizeof(int32_t) * mf);
    const size_t o_pl = take(sizeof(int32_t) * mf), o_ps = take(sizeof(int32_t) * mf * kern::kMaxPath), o_pb = take(sizeof(int32_t) * mf * kern::kMaxPath);
    const size_t o_ir = take(sizeof(int32_t) * mf), o_pv = take(sizeof(float) * mf * kern::kMaxPath);
    const size_t o_pc = take(sizeof(Chunk) * cap_p), o_st = take(sizeof(int32_t) * mf), o_state = take(sizeof(int32_t) * 4);
    const size_t o_cs = take(sizeof(int32_t) * kern::kMaxPath), o_cbin = take(sizeof(int32_t) * kern::kMaxPath), o_cv = take(sizeof(float) * kern::kMaxPath);
    char *pb_ = static_cast<char *>(d_plan_.ensure(off));
    kern::ObliviousPlan pl{};
    pl.node_seg = reinterpret_cast<int32_t *>(pb_ + o_seg); pl.node_n = reinterpret_cast<int32_t *>(pb_ + o_n); pl.mf = mf;
    pl.chunks = reinterpret_cast<Chunk *>(pb_ + o_chunks); pl.cap_h = cap_h; pl.chunk_begin = reinterpret_cast<int32_t *>(pb_ + o_cb);
    pl.slot_map = reinterpret_cast<int32_t *>(pb_ + o_sm); pl.sub_par = reinterpret_cast<int32_t *>(pb_ + o_sp); pl.sub_sib = reinterpret_cast<int32_t *>(pb_ + o_ss);
    pl.path_len = reinterpret_cast<int32_t *>(pb_ + o_pl); pl.path_slot = reinterpret_cast<int32_t *>(pb_ + o_ps); pl.path_bin = reinterpret_cast<int32_t *>(pb_ + o_pb);
    pl.is_root = reinterpret_cast<int32_t *>(pb_ + o_ir); pl.path_val = reinterpret_cast<float *>(pb_ + o_pv);
    pl.part_chunks = reinterpret_cast<Chunk *>(pb_ + o_pc); pl.cap_p = cap_p; pl.seg_starts = reinterpret_cast<int32_t *>(pb_ + o_st);
    pl.state = reinterpret_cast<int32_t *>(pb_ + o_state);
    pl.cond_slot = reinterpret_cast<int32_t *>(pb_ + o_cs); pl.cond_bin = reinterpret_cast<int32_t *>(pb_ + o_cbin); pl.cond_val = reinterpret_cast<float *>(pb_ + o_cv);
    // one result block per level
    char *d_res_all = static_cast<char *>(d_res_all_.ensure(res_bytes * MD));
    char *h_res_all = static_cast<char *>(pin_res_all_.ensure(res_bytes * MD));
    auto level_block = [&](char *all, int depth) { return ResultBlock{all + static_cast<size_t>(depth) * res_bytes, static_cast<size_t>(mf)}; };
    for (int depth = 0; depth < MD; ++depth) {
        const int n_act = 1 << depth, n_comp = depth == 0 ? 1 : n_act / 2;
        const ResultBlock res = level_block(d_res_all, depth);
        const float *best_prev = depth ? level_block(d_res_all, depth - 1).best_score() : nullptr;
        int64_t *d_hist = w.hist_lvl[depth & 1];
        const int64_t *d_hist_prev = w.hist_lvl[(depth & 1) ^ 1];
        phase_begin();
        kern::plan_oblivious_level(depth, N, c.chunk_rows, dims.hist_chunk_budget, depth ? w.resolved : nullptr, best_prev, c.d_thr, B, pl, s);
        phase_end("plan");
        {
            const auto ev = kernel_events("hist_build", /*key=*/true);
            kern::hist_build(c.d_codes, N, c.d_qg, D, w.rows[depth & 1], pl.chunks, cap_h, n_groups, FG, NB, w.partials, s, ev.first, ev.second);
        }
        phase_begin();
        kern::hist_reduce(w.partials, pl.chunk_begin, pl.slot_map, n_comp, n_groups, FG, NB, D, Fp, d_hist, s, std::max(1, dims.hist_chunk_budget / n_comp));
        phase_end("hist_reduce");
        phase_begin();
        kern::score_candidates(d_hist, d_hist_prev, depth > 0 ? pl.sub_par : nullptr, pl.sub_sib, n_act, Fp, NB, D, t.slots, c.n_slots, c.d_thr, B, n_cand, model.meta.min_data_in_leaf,
                               c.cosine ? 1 : 0, c.d_scales, pl.path_len, pl.path_slot, pl.path_val, pl.path_bin, w.scores, w.parent, t.cand_w, t.cand_ref, pl.is_root,
                               nullptr, w.am_i, s);
        kern::argmax(w.scores, n_act, n_cand, t.cand_w, t.cand_ref, w.parent, pl.is_root, true, w.am_v, w.am_i, res.best_idx(), res.best_score(), s);
        kern::resolve_splits(w.am_v, w.am_i, dims.am_parts, res.best_idx(), res.best_score(), true, n_act, t.ref_to_internal, t.cand_slot, t.slots, d_hist, nullptr, Fp, NB, D, w.resolved,
                             res.counts(), mf, pl.seg_starts, w.cursors, c.d_thrkeys, B, s);
        phase_end("score_select");
        phase_begin();
        kern::partition_rows(w.rows[depth & 1], w.rows[(depth & 1) ^ 1], c.d_codes, c.d_kt, N, pl.part_chunks, cap_p, w.resolved, w.cursors, s);
        phase_end("partition");
    }
    hip_check(hipMemcpyAsync(h_res_all, d_res_all, res_bytes * MD, hipMemcpyDeviceToHost, s), "D2H tree results");
    hip_check(hipStreamSynchronize(s), "sync tree");
    hip_check(hipGetLastError(), "growth kernels");
    // replay the bookkeeping level by level
    for (int depth = 0; depth < MD; ++depth) {
        const std::vector<int> active = tb.frontier;   // oblivious: the whole level
        if (static_cast<int>(active.size()) != (1 << depth)) throw HipError("internal: level size mismatch");
        LevelOutcome lvl = tb.digest_level(active, level_block(h_res_all, depth), DigestMode{});
        if (lvl.stop || lvl.splitting.empty()) { if (!lvl.stop) tb.frontier.clear(); break; }
        w.cur ^= 1;
        tb.frontier = lvl.next;
    }
}

// ---- the level-synchronous host loop.  Per level the host (1) uploads ONE packed descriptor block (chunk tables, slot maps, paths,
// partition chunks) from pinned memory, (2) enqueues histogram / reduce / subtract / score / argmax / resolve kernels, the publication
// of ONE small result block (best candidate, child sizes) and -- from descriptors the device completes itself -- the partition,
// (3) waits for the result block only (a sequence word, not the stream) and books the children while the partition runs.  Leaf
// sums are enqueued when a node becomes a leaf.
void Engine::grow_levels_host(const GrowCtx &c, const GrowDims &dims, const StepTables &t, LevelWork &w, TreeBuilder &tb, Stager &sta, Stager &stb) {
    hipStream_t s = stream_;
    const int N = c.N;
    for (int depth = 0; depth < c.MD; ++depth) {
        std::vector<int> active = tb.active_nodes();
        if (active.empty()) break;
        const Level L = stage_level(c, dims, w, tb, sta, depth, std::move(active));
        level_histograms(c, dims, w, L);
        // -- scores, selection, and the child sizes of the selected split(s): all on the device, ONE read-back
        const uint32_t seq = score_select_level(c, dims, t, w, L);
        // One GPU: the partition of this level is enqueued right behind the selection kernels, from descriptors the device
        // completes itself (k_resolve_splits), so that it runs while the host is still waiting for / digesting the read-back.
        if (dims.event_results) hip_check(hipEventRecord(ev_level_, s), "hipEventRecord");
        phase_begin();
        if (!L.part_chunks.empty())
            kern::partition_rows(w.rows[w.cur], w.rows[w.cur ^ 1], c.d_codes, c.d_kt, N, L.d_part_chunks, static_cast<int>(L.part_chunks.size()), w.resolved, w.cursors, s);
        phase_end("partition");
        // spin on the event (a blocking wait costs a thread wake-up of ~10-20 us per level; the wait itself is a few tens of us)
        if (dims.event_results) {
            for (;;) {
                const hipError_t q = hipEventQuery(ev_level_);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) hip_check(q, "hipEventQuery(level results)");
            }
        } else {
            // poll the sequence word; now and then ask the stream for errors (a faulted kernel would never publish)
            verify_pending_categories();   // (first level only does work: hidden behind the level's kernels)
            spin_until_published(w.h_flag, seq, s, "level results");
        }
        hip_check(hipGetLastError(), "growth kernels");
        if (w.am_s != nullptr && !has_coll_ && !dims.event_results) replay_near_ties(c, dims, t, w, tb.nodes, L);
        LevelOutcome lvl = tb.digest_level(L.active, w.h_res, DigestMode{});
        if (lvl.stop) break;
        // -- leaves finalised at this level (their segment is intact in the current list) and the partition: enqueued, not awaited
        stb.reset();
        if (!lvl.new_leaves.empty()) {
            const ChunkTable leaves = make_chunks(tb.nodes, lvl.new_leaves, 1024, true);
            if (!leaves.chunks.empty()) {
                Chunk *d_lc = stb.put(leaves.chunks.data(), leaves.chunks.size());
                stb.flush();
                phase_begin();
                kern::leaf_sums(c.dgrads, c.D, w.rows[w.cur], d_lc, static_cast<int>(leaves.chunks.size()), c.d_scales, w.leafacc, s);
                phase_end("leaves");
            }
        }
        if (lvl.splitting.empty()) { tb.frontier.clear(); break; }
        w.cur ^= 1;   // the partition was enqueued from the device-side descriptors (same decisions: best_score rule, n_left)
        if (w.iota_root) { w.rows[0] = w.rows_scratch; w.iota_root = false; }   // the root list is read-only: the next partition writes the scratch list
        tb.frontier = lvl.next;
    }
}

// Which nodes of the level are accumulated and which derived, the level's descriptor tables, and their upload through stage A.
// Level 0: the root.  Deeper levels: of every sibling pair only the child with fewer rows is accumulated from the data; the other one
// is parent - sibling (exact integers), which halves the LDS-atomic work.  The level buffers hold GLOBAL histograms.  Row-sharded runs
// pick the "smaller" child by its global row count (the same on every rank), exchange only those children and subtract globally.
Level Engine::stage_level(const GrowCtx &c, const GrowDims &dims, LevelWork &w, TreeBuilder &tb, Stager &sta, int depth, std::vector<int> active) {
    std::vector<HNode> &nodes = tb.nodes;
    Level L;
    L.depth = depth;
    L.active = std::move(active);
    const std::vector<int> &act = L.active;
    const int n_act = L.n_act = static_cast<int>(act.size());
    L.d_hist = w.hist_lvl[depth & 1];
    L.d_hist_prev = w.hist_lvl[(depth & 1) ^ 1];
    std::vector<int> &compute_ids = L.compute_ids;
    std::vector<int32_t> &slot_map = L.slot_map, sub_par(n_act, -1), sub_sib(n_act, -1);
    if (depth == 0) {
        compute_ids = act;
        for (int k = 0; k < n_act; ++k) slot_map.push_back(k);
    } else {
        std::vector<int> slot_of(nodes.size(), -1);
        for (int k = 0; k < n_act; ++k) slot_of[act[k]] = k;
        for (int k = 0; k < n_act; ++k) {
            const int id = act[k], par = nodes[id].parent;
            const int sib = nodes[par].left == id ? nodes[par].right : nodes[par].left;
            const bool sib_active = slot_of[sib] >= 0;
            // the child that is accumulated: fewer local rows; ties -> the left child
            const long long mine = has_coll_ ? nodes[id].n_global : nodes[id].n_local;
            const long long theirs = has_coll_ ? nodes[sib].n_global : nodes[sib].n_local;
            const bool i_am_small = sib_active && (mine < theirs || (mine == theirs && nodes[par].left == id));
            if (i_am_small) {
                compute_ids.push_back(id);
                slot_map.push_back(k);
            } else {
                sub_par[k] = nodes[par].hist_slot;
                sub_sib[k] = sib_active ? slot_of[sib] : -1;
            }
        }
    }
    for (int k = 0; k < n_act; ++k) nodes[act[k]].hist_slot = k;
    // chunk table of ALL active nodes: the partition's and (row-sharded runs count the local child sizes from the rows themselves) the counting's
    L.part_chunks = make_chunks(nodes, act, kern::kPartitionRows, false).chunks;
    if (has_coll_) L.count_chunks = L.part_chunks;
    // RL-sized levels on one GPU: every accumulated node is ONE chunk (empty nodes included) and k_hist_build stores the node's
    // int64 histogram itself -- no partials, no hist_reduce launch (kern::HistDirect).  A block then walks up to `direct_cap` rows
    // alone: the cap keeps that below ~10 us of LDS atomics ((D + 1) per row and feature).
    const int direct_cap = std::min(8192, std::max(1024, 9216 / (c.D + 1)));
    L.hist_direct = !has_coll_ && !hooks::on(hooks::NO_DIRECT_HIST) /* test / measurement hook */ && kern::hist_direct_supported(c.FG) && !compute_ids.empty() &&
                    compute_ids.size() <= static_cast<size_t>(dims.hist_max_chunks);
    for (int id : compute_ids) L.hist_direct = L.hist_direct && nodes[id].n_local <= direct_cap;
    if (L.hist_direct) {
        L.hist.begin.assign(1, 0);
        for (size_t k = 0; k < compute_ids.size(); ++k) {
            const HNode &nd = nodes[compute_ids[k]];
            L.hist.chunks.push_back({static_cast<int32_t>(k), nd.seg_start, nd.n_local, 0});
            L.hist.begin.push_back(static_cast<int32_t>(L.hist.chunks.size()));
        }
    } else {
        L.hist = make_chunks(nodes, compute_ids, balanced_chunk_rows(nodes, compute_ids, c.chunk_rows, dims.hist_chunk_budget), false);
    }
    if (L.hist.chunks.size() > static_cast<size_t>(dims.hist_max_chunks)) throw HipError("internal: chunk table overflow");
    // paths (duplicate-on-path rejection, node.cpp:154-166)
    std::vector<int32_t> pl(n_act), ps(static_cast<size_t>(n_act) * kern::kMaxPath, -1), pb(static_cast<size_t>(n_act) * kern::kMaxPath, 0), root(n_act);
    std::vector<float> pv(static_cast<size_t>(n_act) * kern::kMaxPath, 0.f);
    std::vector<int32_t> seg_starts(n_act), n_locals(n_act);
    for (int k = 0; k < n_act; ++k) {
        const HNode &nd = nodes[act[k]];
        pl[k] = static_cast<int32_t>(nd.path.size());
        root[k] = nd.depth == 0;
        for (size_t q = 0; q < nd.path.size(); ++q) {
            ps[k * kern::kMaxPath + q] = nd.path[q].fslot;
            pv[k * kern::kMaxPath + q] = nd.path[q].value;
            pb[k * kern::kMaxPath + q] = nd.path[q].bin;
        }
        seg_starts[k] = nd.seg_start;
        n_locals[k] = nd.n_local;
    }
    sta.reset();
    L.d_chunks = sta.put(L.hist.chunks.data(), L.hist.chunks.size());
    L.d_chunk_begin = sta.put(L.hist.begin.data(), L.hist.begin.size());
    L.d_slotmap = sta.put(slot_map.data(), slot_map.size());
    L.d_sub_par = sta.put(sub_par.data(), sub_par.size());
    L.d_sub_sib = sta.put(sub_sib.data(), sub_sib.size());
    L.d_path_len = sta.put(pl.data(), pl.size());
    L.d_path_slot = sta.put(ps.data(), ps.size());
    L.d_path_val = sta.put(pv.data(), pv.size());
    L.d_path_bin = sta.put(pb.data(), pb.size());
    L.d_isroot = sta.put(root.data(), root.size());
    L.d_count_chunks = sta.put(L.count_chunks.data(), L.count_chunks.size());
    L.d_part_chunks = sta.put(L.part_chunks.data(), L.part_chunks.size());
    L.d_seg_starts = sta.put(seg_starts.data(), seg_starts.size());
    L.d_n_locals = sta.put(n_locals.data(), n_locals.size());
    sta.flush();
    // root of a numeric-only tree on one GPU whose candidates came from the radix selection: the class counts are known from the
    // selection's ranks, so the histogram build skips the count atomic (8 instead of 9 per (row, feature) at D = 8) and hist_reduce
    // writes the counts (GBRL_HIP_ROOT_COUNTS=0: accumulate them like every other level; =2: do both and compare, the tests)
    L.root_mode = hooks::num(hooks::ROOT_COUNTS, 1);
    L.root_countless = depth == 0 && c.root_le != nullptr && L.root_mode != 0 && !L.hist_direct && !has_coll_ && c.n_global == c.N && c.NB == c.B + 1 &&
                       kern::hist_countless_supported(c.D, c.FG, c.N);
    L.ar_level = w.ar_prefix && sizeof(int64_t) * compute_ids.size() * dims.hist_node_elems <= dims.ar_max_bytes;
    w.ar_prefix = L.ar_level;
    L.lvl_slots = L.ar_level ? c.n_slots : dims.own_slots;
    L.lvl_lo = (has_coll_ && !L.ar_level) ? dims.coll_lo : 0;
    // last level on one GPU: the derived siblings are scored but not written back (nothing subtracts from them any more)
    L.drop_derived = !has_coll_ && !hooks::on(hooks::KEEP_LAST_DERIVED) /* measurement hook */ && depth > 0 && depth == c.MD - 1;
    return L;
}

// The level's histograms into L.d_hist, by one of three transports: one GPU (k_hist_reduce, or k_hist_build directly), row-sharded with a
// whole-level all-reduce, row-sharded with a reduce-scatter by feature.
void Engine::level_histograms(const GrowCtx &c, const GrowDims &dims, const LevelWork &w, const Level &L) {
    hipStream_t s = stream_;
    const int N = c.N, F = c.F, D = c.D, B = c.B, NB = c.NB, FG = c.FG, Fp = c.Fp, n_groups = c.n_groups;
    const int n_chunks = static_cast<int>(L.hist.chunks.size()), nc = static_cast<int>(L.compute_ids.size());
    const int32_t *d_rows = w.rows[w.cur];
    int64_t *d_hist = L.d_hist;
    bool hist_written = false;
    if (n_chunks) {
        const auto ev = kernel_events("hist_build", /*key=*/true);   // the dispatch's own timestamps: no bubble in the stream
        kern::HistDirect hd;
        if (L.hist_direct) { hd.hist = d_hist; hd.slot_map = L.d_slotmap; hd.Fp = Fp; }
        hist_written = kern::hist_build(c.d_codes, N, c.d_qg, D, d_rows, L.d_chunks, n_chunks, n_groups, FG, NB, w.partials, s, ev.first, ev.second,
                                        L.hist_direct ? &hd : nullptr, !L.root_countless);
    }
    if (!hist_written) phase_begin();   // (no phase record for a level whose histograms k_hist_build stored itself)
    if (!has_coll_) {
        if (nc && !hist_written)
            kern::hist_reduce(w.partials, L.d_chunk_begin, L.d_slotmap, nc, n_groups, FG, NB, D, Fp, d_hist, s, n_chunks / nc, 0, L.root_countless ? c.root_le : nullptr, F, B, N);
    } else if (nc && L.ar_level) {
        // whole-level all-reduce: plain [node][feature][class][D+1] layout (scatter with ONE owner), global sums to the level slots
        bool in_place = true;      // the computed nodes fill the first level slots in order (the root; a level whose first nc nodes are the smaller children)
        for (int k = 0; k < nc; ++k) in_place = in_place && L.slot_map[k] == k;
        int64_t *buf = in_place ? d_hist : w.hist_coll;
        kern::hist_reduce(w.partials, L.d_chunk_begin, nullptr, nc, n_groups, FG, NB, D, Fp, buf, s, n_chunks / nc, Fp);
        exchange(Red::SumI64, buf, static_cast<size_t>(nc) * dims.hist_node_elems);
        if (!in_place) kern::hist_place(buf, d_hist, L.d_slotmap, nc, dims.hist_node_elems, s);
    } else if (nc) {
        // local sums of the computed nodes in the feature-scattered send layout -> ONE reduce-scatter -> this rank's feature
        // slice of the global sums goes to the nodes' level slots (the other features of d_hist are never read on this rank)
        const int coll_P = dims.coll_P, coll_Fs = dims.coll_Fs;
        if (coll_P * coll_Fs != Fp) hip_check(hipMemsetAsync(w.hist_coll, 0, sizeof(int64_t) * static_cast<size_t>(coll_P) * nc * coll_Fs * dims.feat_elems, s), "memset");
        kern::hist_reduce(w.partials, L.d_chunk_begin, nullptr, nc, n_groups, FG, NB, D, Fp, w.hist_coll, s, n_chunks / nc, coll_Fs);
        reduce_scatter_i64(w.hist_coll, w.hist_recv, static_cast<size_t>(nc) * coll_Fs * dims.feat_elems);
        kern::hist_place_slice(w.hist_recv, d_hist, L.d_slotmap, nc, coll_Fs, dims.coll_lo, Fp, dims.feat_elems, s);
    }
    if (L.root_countless && L.root_mode == 2) {
        // GBRL_HIP_ROOT_COUNTS=2 (tests): the root's count fields once more by accumulation, compared entry by entry
        int64_t *d_alt = w.hist_lvl[(L.depth & 1) ^ 1];
        kern::hist_build(c.d_codes, N, c.d_qg, D, d_rows, L.d_chunks, n_chunks, n_groups, FG, NB, w.partials, s, nullptr, nullptr, nullptr, true);
        kern::hist_reduce(w.partials, L.d_chunk_begin, L.d_slotmap, nc, n_groups, FG, NB, D, Fp, d_alt, s, n_chunks / nc);
        const size_t ne = dims.hist_node_elems;
        std::vector<int64_t> ha(ne), hb(ne);
        hip_check(hipMemcpyAsync(ha.data(), d_hist, ne * 8, hipMemcpyDeviceToHost, s), "D2H root histogram");
        hip_check(hipMemcpyAsync(hb.data(), d_alt, ne * 8, hipMemcpyDeviceToHost, s), "D2H root histogram");
        hip_check(hipStreamSynchronize(s), "sync");
        for (int f = 0; f < F; ++f)
            for (int cl = 0; cl < NB; ++cl)
                for (int d = 0; d <= D; ++d) {
                    const size_t i = (static_cast<size_t>(f) * NB + cl) * (D + 1) + d;
                    if (ha[i] != hb[i])
                        throw HipError("root histogram check: feature " + std::to_string(f) + " class " + std::to_string(cl) + " field " + std::to_string(d) + ": " +
                                       std::to_string(ha[i]) + " from the selection's ranks, " + std::to_string(hb[i]) + " accumulated");
                }
    }
    if (!hist_written) phase_end("hist_reduce");
}

// Scores, selection and the child sizes of the selected split(s), the row-sharded winner exchange, and the publication of the level's
// result block.  Returns the sequence number the host waits for (0: GBRL_HIP_EVENT_RESULTS, a copy and an event instead).
uint32_t Engine::score_select_level(const GrowCtx &c, const GrowDims &dims, const StepTables &t, const LevelWork &w, const Level &L) {
    hipStream_t s = stream_;
    const int N = c.N, D = c.D, B = c.B, NB = c.NB, Fp = c.Fp, n_cand = c.n_cand, n_act = L.n_act, max_front = dims.max_front, depth = L.depth;
    const bool oblivious = c.oblivious, event_results = dims.event_results;
    const ResultBlock &res = w.d_res;
    phase_begin();
    // (row-sharded: this rank scores its own feature slots only; candidates of the other ranks stay at -inf)
    if (has_coll_ && !L.ar_level && oblivious) kern::fill_f32(w.scores, static_cast<size_t>(n_act) * n_cand, -INFINITY, s);
    if (L.lvl_slots > 0)
        kern::score_candidates(L.d_hist, L.d_hist_prev, depth > 0 ? L.d_sub_par : nullptr, L.d_sub_sib, n_act, Fp, NB, D, t.slots, L.lvl_slots, c.d_thr, B, n_cand, model.meta.min_data_in_leaf, c.cosine ? 1 : 0,
                               c.d_scales, L.d_path_len, L.d_path_slot, L.d_path_val, L.d_path_bin, w.scores, w.parent, t.cand_w, t.cand_ref, L.d_isroot,
                               oblivious ? nullptr : w.am_v, w.am_i, s, L.lvl_lo, !L.drop_derived, oblivious ? nullptr : w.am_s, oblivious ? nullptr : w.am_n);
    // oblivious: the scores are summed over the level's nodes first (stage 1 below); greedy: k_score has already reduced every
    // feature of every node to its best gain, so only the final reduction inside k_resolve_splits is left
    if (oblivious)
        kern::argmax(w.scores, n_act, n_cand, t.cand_w, t.cand_ref, w.parent, L.d_isroot, oblivious, w.am_v, w.am_i, res.best_idx(), res.best_score(), s, w.am_s);
    // counts = [total | right] from the (global) histogram; sharded runs add [right_local] counted from the local rows
    // (one GPU: the kernel itself mirrors the result block into the pinned host copy and its last block publishes the sequence word)
    const bool publish_in_resolve = !has_coll_ && !event_results;
    const uint32_t seq = event_results ? 0 : next_seq();
    const bool near_level = w.am_s != nullptr && publish_in_resolve;
    const kern::NearDetect near_detect{w.am_s, oblivious ? nullptr : w.am_n, dims.near_rel, w.parent, L.d_isroot, c.cosine ? 1 : 0, N};
    kern::resolve_splits(w.am_v, w.am_i, oblivious ? dims.am_parts : L.lvl_slots, res.best_idx(), res.best_score(), oblivious, n_act, t.ref_to_internal, t.cand_slot, t.slots, L.d_hist, nullptr, Fp, NB, D, w.resolved,
                         res.counts(), max_front, L.d_seg_starts, w.cursors, c.d_thrkeys, B, s, publish_in_resolve ? w.h_res_dev : nullptr, w.d_flag, seq, w.d_pub_done,
                         L.drop_derived ? L.d_hist_prev : nullptr, L.drop_derived ? L.d_sub_par : nullptr, L.drop_derived ? L.d_sub_sib : nullptr, near_level ? &near_detect : nullptr);
    if (has_coll_) {
        if (!L.ar_level) {
            // the level's winner over all ranks: every rank holds the best of ITS features and the child sizes it induces
            const int n_win = oblivious ? 1 : n_act;
            const size_t gwords = static_cast<size_t>(dims.coll_P) * (n_win + 2 * n_act);
            kern::winner_pack(res.best_idx(), res.best_score(), res.counts(), max_front, n_win, n_act, coll_.rank, w.gather, s, dims.coll_P);
            exchange(Red::SumI64, w.gather, gwords);
            kern::winner_adopt(w.gather, dims.coll_P, n_win, n_act, oblivious, t.ref_to_internal, t.cand_slot, t.slots, L.d_seg_starts, c.d_thrkeys, B, res.best_idx(), res.best_score(),
                               res.counts(), max_front, w.resolved, w.cursors, s);
        }
        // (whole-level all-reduce: k_resolve_splits has resolved the global winner on every rank and cleared the third counts array)
        int64_t *d_right_local = res.right_local();   // (cleared by winner_adopt)
        if (!L.count_chunks.empty())
            kern::count_right(w.rows[w.cur], c.d_codes, c.d_kt, N, L.d_count_chunks, static_cast<int>(L.count_chunks.size()), w.resolved, d_right_local, s);
        // global left sizes -> this rank's, and the completed result block to the host: one launch.  (Round 6: the counting kernel's last
        // block doing this instead cost 8 us per level MORE -- its 256 blocks queue on one completion counter, ~30 ns per returning atomic.)
        if (event_results) kern::localize_splits(w.resolved, L.d_n_locals, d_right_local, n_act, s);
        else kern::localize_publish(w.resolved, L.d_n_locals, d_right_local, n_act, res.base, w.h_res_dev, dims.res_bytes, w.d_flag, seq, s);
    }
    if (event_results) hip_check(hipMemcpyAsync(w.h_res.base, res.base, dims.res_bytes, hipMemcpyDeviceToHost, s), "D2H level results");
    phase_end("score_select");
    return seq;
}

// Near-tie replay of one level (one GPU), after its result block has arrived.  Flags of the level (k_resolve_splits): any -> the candidates
// in the window are scored once more, the reference's way, the final arg-max stage runs on their outcome and the partition -- already
// enqueued from the exact decision, its input list is intact -- runs again; returns once the replayed result block has arrived.
void Engine::replay_near_ties(const GrowCtx &c, const GrowDims &dims, const StepTables &t, const LevelWork &w, const std::vector<HNode> &nodes, const Level &L) {
    hipStream_t s = stream_;
    const int N = c.N, D = c.D, B = c.B, NB = c.NB, Fp = c.Fp, n_cand = c.n_cand, n_act = L.n_act, max_front = dims.max_front, depth = L.depth;
    const int near_max_rows = dims.near_max_rows, own_slots = dims.own_slots;
    const bool oblivious = c.oblivious, cosine = c.cosine;
    const std::vector<int> &active = L.active;
    const int64_t *near_h = w.h_res.near_flags();
    // nodes above the requested size limit keep the exact arg-max (GBRL_HIP_NEARTIE_MAX_ROWS, batches above 65 536 rows only; 0 = no limit;
    // an oblivious level is replayed only when every one of its nodes is within the limit)
    bool any = false;
    if (oblivious) {
        any = near_h[0] != 0;
        if (any && near_max_rows > 0) for (int k = 0; k < n_act; ++k) any = any && nodes[active[k]].n_local <= near_max_rows;
    } else {
        for (int k = 0; k < n_act; ++k) any = any || (near_h[k] != 0 && (near_max_rows == 0 || nodes[active[k]].n_local <= near_max_rows));
    }
    if (!any) return;
    if (hooks::on(hooks::NEARTIE_DEBUG)) {   // measurement hook
        const float *bs = w.h_res.best_score();
        for (int k = 0; k < (oblivious ? 1 : n_act); ++k)
            if (near_h[k]) {
                const int32_t sb = static_cast<int32_t>(w.h_res.near_second()[k]);
                float sec; std::memcpy(&sec, &sb, 4);
                fprintf(stderr, "[near-tie] depth %d node %d of %d (%d rows): best gain %.9g (candidate %d), runner-up %.9g, difference %.3g\n", depth, k, n_act, nodes[active[k]].n_local,
                        bs[k], w.h_res.best_idx()[k], sec, bs[k] - sec);
            }
    }
    ++near_replays_;
    phase_begin();
    int32_t *d_cand_nr = (oblivious || N <= 8192) ? nullptr : static_cast<int32_t *>(d_near_nr_.ensure(sizeof(int32_t) * static_cast<size_t>(max_front) * std::max(1, n_cand)));
    if (!oblivious)   // every candidate's exact score and child sizes (the greedy selection kept the per-slot bests only)
        kern::score_candidates(L.d_hist, L.d_hist_prev, depth > 0 ? L.d_sub_par : nullptr, L.d_sub_sib, n_act, Fp, NB, D, t.slots, own_slots, c.d_thr, B, n_cand, model.meta.min_data_in_leaf, cosine ? 1 : 0,
                               c.d_scales, L.d_path_len, L.d_path_slot, L.d_path_val, L.d_path_bin, w.scores, w.parent, t.cand_w, t.cand_ref, L.d_isroot, nullptr, w.am_i, s, 0, !L.drop_derived, nullptr, nullptr, d_cand_nr);
    kern::NearTieIO io{};
    io.rows = w.rows[w.cur]; io.seg_start = L.d_seg_starts; io.n_rows = L.d_n_locals; io.codes = c.d_codes; io.N = N; io.D = D; io.grads = c.dgrads; io.meanden = c.d_meanden;
    io.cosine = cosine ? 1 : 0; io.oblivious = oblivious ? 1 : 0; io.min_data = model.meta.min_data_in_leaf; io.slots = t.slots; io.cand_slot = t.cand_slot; io.cand_w = t.cand_w; io.cand_ref = t.cand_ref;
    io.n_cand = n_cand; io.scores = w.scores; io.cand_nr = d_cand_nr; io.parent = w.parent; io.is_root = L.d_isroot; io.best_score = w.d_res.best_score(); io.near = w.d_res.near_flags();
    io.rel = dims.near_rel; io.n_act = n_act;
    int32_t *lists = static_cast<int32_t *>(d_near_list_.ensure(sizeof(int32_t) * static_cast<size_t>(max_front) * (kern::kNearCands + 1)));
    io.list = lists; io.list_n = lists + static_cast<size_t>(max_front) * kern::kNearCands;
    io.ent = static_cast<int32_t *>(d_near_ent_.ensure(sizeof(int32_t) * std::max(static_cast<size_t>(kern::kNearCands + 1) * N, static_cast<size_t>(n_cand))));
    io.rep = static_cast<float *>(d_near_rep_.ensure(sizeof(float) * static_cast<size_t>(max_front) * (kern::kNearCands + 1)));
    io.part_v = w.am_v; io.part_i = w.am_i; io.n_parts = oblivious ? dims.am_parts : own_slots;
    io.max_node_rows = near_max_rows;
    if (const size_t mw = kern::near_tie_map_words(N, n_act)) io.maps = static_cast<uint32_t *>(d_near_maps_.ensure(sizeof(uint32_t) * mw));
    int near_largest = 0;      // the largest node this replay will walk
    for (int k = 0; k < n_act; ++k)
        if ((oblivious || near_h[k] != 0) && (near_max_rows == 0 || nodes[active[k]].n_local <= near_max_rows)) near_largest = std::max(near_largest, nodes[active[k]].n_local);
    // (below ~10^5 rows per node the one-lane-per-chain core is the faster one: the parallel evaluation summarises 17 N D elements
    // per pass whatever the nodes' sizes -- profiles/r06_neartie_fullsize_cost.txt)
    if (kern::near_tie_fast_supported(N, D) && (reinterpret_cast<uintptr_t>(c.dgrads) & 15) == 0 /* float4 pieces of the gradient rows */ && !hooks::on(hooks::NEARTIE_SERIAL) && near_largest > (cosine ? 32768 : 98304)) {   // (the dot chains of Cosine are D times longer: the parallel evaluation pays off earlier)
        // big batch, D a multiple of 4: the float32 chains are evaluated by seqsum.hip on the whole GPU (GBRL_HIP_NEARTIE_SERIAL=1: the
        // one-lane-per-chain core of neartie_core.h, same bits -- the tests compare the two)
        const size_t rows17 = static_cast<size_t>(kern::kNearCands + 1) * N, blocks17 = static_cast<size_t>(n_act) * (kern::kNearCands + 1);
        io.fast = 1;
        io.pos = static_cast<int32_t *>(d_near_pos_.ensure(sizeof(int32_t) * rows17));
        io.nr = static_cast<int32_t *>(d_near_nrb_.ensure(sizeof(int32_t) * blocks17));
        io.vals = static_cast<float *>(d_near_vals_.ensure(sizeof(float) * rows17 * D));
        io.means = static_cast<float *>(d_near_means_.ensure(sizeof(float) * blocks17 * 2 * D));
        io.sums = static_cast<float *>(d_near_sums_.ensure(sizeof(float) * blocks17 * 2 * D));
        io.rowsort = static_cast<int32_t *>(d_near_rowsort_.ensure(sizeof(int32_t) * static_cast<size_t>(N)));
        io.tiles = static_cast<int32_t *>(d_near_tiles_.ensure(sizeof(int32_t) * kern::near_tie_fast_tiles(N, n_act)));
        io.seq_blocks = kern::near_tie_fast_blocks(N, D, n_act);
        io.chains_bytes = kern::near_tie_fast_chain_bytes(N, D, n_act);
        io.chains = d_near_chains_.ensure(io.chains_bytes);
    }
    kern::near_tie_replay(io, s);
    const uint32_t seq = next_seq();
    kern::resolve_splits(w.am_v, w.am_i, oblivious ? dims.am_parts : own_slots, w.d_res.best_idx(), w.d_res.best_score(), oblivious, n_act, t.ref_to_internal, t.cand_slot, t.slots, L.d_hist, nullptr, Fp, NB, D, w.resolved,
                         w.d_res.counts(), max_front, L.d_seg_starts, w.cursors, c.d_thrkeys, B, s, w.h_res_dev, w.d_flag, seq, w.d_pub_done,
                         L.drop_derived ? L.d_hist_prev : nullptr, L.drop_derived ? L.d_sub_par : nullptr, L.drop_derived ? L.d_sub_sib : nullptr, nullptr);
    if (!L.part_chunks.empty())
        kern::partition_rows(w.rows[w.cur], w.rows[w.cur ^ 1], c.d_codes, c.d_kt, N, L.d_part_chunks, static_cast<int>(L.part_chunks.size()), w.resolved, w.cursors, s);
    phase_end("near_tie_replay");
    spin_until_published(w.h_flag, seq, s, "level results after the near-tie replay");
    hip_check(hipGetLastError(), "near-tie replay kernels");
}

// ---- the leaves of the last level, the row-sharded sum of the leaf accumulators and their way to the host (both level loops end here)
void Engine::finish_leaves(const GrowCtx &c, const GrowDims &dims, const LevelWork &w, TreeBuilder &tb, Stager &sta, std::vector<int64_t> &acc, double &leaf_scale) {
    hipStream_t s = stream_;
    const int D = c.D;
    std::vector<HNode> &nodes = tb.nodes;
    std::vector<int> last;
    for (int id : tb.frontier)
        if (!nodes[id].leaf) { nodes[id].leaf = true; last.push_back(id); }
    if (nodes.size() == 1) nodes[0].leaf = true;
    const ChunkTable leaves = make_chunks(nodes, last, 1024, true);
    if (!leaves.chunks.empty()) {
        // stage B may still be in flight for the partition of the last level: stage A is free (its level is complete)
        sta.reset();
        Chunk *d_lc = sta.put(leaves.chunks.data(), leaves.chunks.size());
        sta.flush();
        phase_begin();
        kern::leaf_sums(c.dgrads, D, w.rows[w.cur], d_lc, static_cast<int>(leaves.chunks.size()), c.d_scales, w.leafacc, s);
        phase_end("leaves");
    }
    const size_t n_acc_words = nodes.size() * (D + 1);
    if (has_coll_) exchange(Red::SumI64, w.leafacc, n_acc_words);
    // The leaf sums reach the host the way the level results do: a one-block kernel stores them into pinned, device-mapped memory and
    // then a sequence word; the host polls it instead of a copy-engine transfer + hipStreamSynchronize (a blocking wait costs a thread
    // wake-up).  Seeing the word means every earlier operation of the stream -- all kernels that read the caller's inputs, the
    // copies of thresholds and scales -- has completed.
    const size_t acc_bytes = sizeof(int64_t) * std::max<size_t>(1, n_acc_words);
    char *h_acc_raw = static_cast<char *>(pin_acc_.ensure(acc_bytes + 64));
    int64_t *h_acc = reinterpret_cast<int64_t *>(h_acc_raw);
    if (dims.event_results) {
        hip_check(hipMemcpyAsync(h_acc, w.leafacc, sizeof(int64_t) * n_acc_words, hipMemcpyDeviceToHost, s), "D2H leaf acc");
        hip_check(hipStreamSynchronize(s), "sync");
    } else {
        void *h_acc_dev = nullptr;
        hip_check(hipHostGetDevicePointer(&h_acc_dev, h_acc_raw, 0), "hipHostGetDevicePointer");
        volatile uint32_t *h_aflag = reinterpret_cast<volatile uint32_t *>(h_acc_raw + acc_bytes);
        const uint32_t seq = next_seq();
        *h_aflag = 0;
        kern::publish_block(w.leafacc, h_acc_dev, sizeof(int64_t) * n_acc_words, reinterpret_cast<uint32_t *>(static_cast<char *>(h_acc_dev) + acc_bytes), seq, s,
                            /*zero_src=*/true);
        spin_until_published(h_aflag, seq, s, "leaf sums");
        leafacc_clean_ptr_ = w.leafacc;   // only the copied words were ever written, and the kernel cleared them
    }
    acc.assign(h_acc, h_acc + n_acc_words);
    // everything enqueued for this tree has completed: scales are in pinned memory
    if (!std::isfinite(c.h_scales->hmax_build) || !std::isfinite(c.h_scales->hmax_raw)) throw InvalidArgument("non-finite gradients");
    leaf_scale = c.h_scales->leaf_scale;
}

}  // namespace gbrl
