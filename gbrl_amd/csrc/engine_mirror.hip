// engine_mirror.hip -- the device mirror of the ensemble: the append-only structure-of-arrays and the packed records the fast predict kernels
// read (sync_model_to_device), the code book of the packed-code path (ensure_pc_book), the view of both that a kernel gets (mirror_view), and
// the category dictionary on the host and on the device.  Every record that is derived from the model is built by mirror_records.h (host
// only, tested without a device); this file keeps the upload marks (engine.h states their invariant) and moves the bytes.
#include "engine.h"
#include "hooks.h"

#include "cat_hash.h"

#include <algorithm>
#include <cstring>

namespace gbrl {

namespace {

// The slices one sync_model_to_device() appends (one new tree after a step: a dozen pieces of a few hundred bytes) are collected and leave
// together in flush(): staged in ONE pinned block and copied by one kernel launch, instead of a hipMemcpyAsync from pageable memory per piece
// plus a stream synchronisation -- 0.1 ms per predict-after-step in an RL loop.
struct MirrorUpload {
    hipStream_t s;
    PinnedBuf &stage;
    hipEvent_t stage_read;   // behind the last launch that read the staging block
    struct Seg { char *dst; const char *src; size_t bytes; };
    std::vector<Seg> segs;

    // the elements [old_n, new_n) of a host array whose first old_n elements the buffer holds
    void append(DevBuf &buf, const void *host, size_t elem, size_t old_n, size_t new_n) {
        char *p = static_cast<char *>(buf.ensure_keep(std::max<size_t>(new_n, 1) * elem, old_n * elem, s));
        if (new_n > old_n) segs.push_back({p + old_n * elem, static_cast<const char *>(host) + old_n * elem, (new_n - old_n) * elem});
    }
    // records followed by `pad` zero elements that the kernels read past the last tree: when the buffer did not move, the old padding is still
    // in place and only the new records and the padding's extension travel (the padding is 128 KiB for the value records)
    void append_padded(DevBuf &buf, const float *host, size_t old_recs, size_t new_recs, size_t rec, size_t pad) {
        const void *before = buf.raw();
        char *p = static_cast<char *>(buf.ensure_keep((new_recs * rec + pad) * 4, old_recs * rec * 4, s));
        if (p != before || old_recs == 0 || old_recs > new_recs) {
            segs.push_back({p + old_recs * rec * 4, reinterpret_cast<const char *>(host + old_recs * rec), ((new_recs - old_recs) * rec + pad) * 4});
        } else if (new_recs > old_recs) {
            segs.push_back({p + old_recs * rec * 4, reinterpret_cast<const char *>(host + old_recs * rec), (new_recs - old_recs) * rec * 4});
            segs.push_back({p + (old_recs * rec + pad) * 4, reinterpret_cast<const char *>(host + old_recs * rec + pad), (new_recs - old_recs) * rec * 4});
        }
    }
    void flush() {
        size_t total = 0;
        for (const Seg &g : segs) total += (g.bytes + 15) & ~static_cast<size_t>(15);
        if (segs.empty()) return;
        if (segs.size() <= 32 && total <= (size_t(1) << 20)) {
            hip_check(hipEventSynchronize(stage_read), "sync");   // the previous use of the staging block has been read (normally long ago)
            char *st = static_cast<char *>(stage.ensure(total));
            void *st_dev = nullptr;
            hip_check(hipHostGetDevicePointer(&st_dev, st, 0), "hipHostGetDevicePointer");
            size_t off = 0;
            for (size_t i = 0; i < segs.size(); i += kern::kStageSegments) {
                kern::StageSegments ss{};
                for (size_t k = i; k < segs.size() && k < i + kern::kStageSegments; ++k) {
                    std::memcpy(st + off, segs[k].src, segs[k].bytes);
                    ss.dst[ss.n] = segs[k].dst; ss.src_off[ss.n] = static_cast<uint32_t>(off); ss.bytes[ss.n] = static_cast<uint32_t>(segs[k].bytes);
                    ++ss.n;
                    off += (segs[k].bytes + 15) & ~static_cast<size_t>(15);
                }
                kern::stage_copy(ss, st_dev, s);
            }
            hip_check(hipEventRecord(stage_read, s), "hipEventRecord");
        } else {   // a whole loaded ensemble: ordinary copies, and the host arrays must outlive them
            for (const Seg &g : segs) hip_check(hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyHostToDevice, s), "H2D model");
            hip_check(hipStreamSynchronize(s), "sync model upload");
        }
        segs.clear();
    }
};

detail::RecordShape record_shape(const gbrl_hip_metadata &md, bool greedy) {
    return {static_cast<size_t>(kern::obl2_levels(md.max_depth)), static_cast<size_t>(kern::obl2_padded_outputs(md.output_dim)), greedy};
}

}  // namespace

// The category dictionary of the model's conditions: host work only, so that a call can check a dictionary token before it needs a device
// (predict_leaves_encoded).  sync_model_to_device() starts with it; a second call for the same model version does nothing.
void Engine::sync_cat_dict() {
    const gbrl_hip_metadata &md = model.meta;
    const size_t T = md.n_trees, L = md.n_leaves, S = model.split_rows();
    if (dict_model_version_ == model.version) return;
    if (up_splits_ > S || up_trees_ > T || up_leaves_ > L || dict_splits_ > S) {   // the ensemble has shrunk: nothing is kept
        up_splits_ = up_trees_ = up_leaves_ = 0; dict_splits_ = 0; grd_up_nodes_ = 0;
        cat_dict_.clear(); cat_ids_host_.clear(); cond_pack_host_.clear();
        dict_version_ = static_cast<size_t>(-1);
    }
    detail::extend_cat_ids(model, dict_splits_, cat_dict_, cat_ids_host_);
    dict_splits_ = S;
    dict_model_version_ = model.version;
}

// Values of EXISTING trees have changed (refit_leaves): every upload mark goes back to the start, and the next sync_model_to_device() builds
// and uploads every derived array again (the code book of the packed-code path and the SHAP program follow model.version by themselves).
// The category dictionary is NOT reset -- unlike the shrunken ensemble of sync_cat_dict(): the conditions have not changed, so ids encoded
// before the refit and the dictionary token stay valid.
void Engine::invalidate_mirror() {
    up_trees_ = up_leaves_ = up_splits_ = 0;
    values_redo_tree_ = kNoRedo;
    grd_up_nodes_ = 0;
    rate_trees_ = 0;
    mirror_version_ = ~0ull;
}

// The values of tree t alone have changed (newton_leaves_prepared; inside fit_prepared t is the tree the step has just appended): the upload mark of
// the values goes back to the tree's first leaf and the next sync_model_to_device() appends them again from there -- m_values_ from that leaf
// on, the pre-swizzled value records from that tree on.  Conditions, node records, code tables and the dictionary hold no value and stay.
void Engine::rewind_values(int t) {
    up_leaves_ = std::min(up_leaves_, static_cast<size_t>(model.tree_indices[t]));
    values_redo_tree_ = std::min(values_redo_tree_, static_cast<size_t>(t));
}

void Engine::sync_model_to_device() {
    const gbrl_hip_metadata &md = model.meta;
    const size_t T = md.n_trees, L = md.n_leaves, S = model.split_rows(), MD = md.max_depth, D = md.output_dim;
    if (mirror_version_ == model.version) return;
    // 1. the dictionary, and the packed conditions that carry its ids
    sync_cat_dict();
    detail::extend_cond_pack(model, cat_ids_host_, up_splits_, cond_pack_host_);
    MirrorUpload up{stream_, pin_model_stage_, ev_model_stage_, {}};
    // 2. the model's arrays as they are
    up.append(m_tree_indices_, model.tree_indices.data(), 4, up_trees_, T);
    up.append(m_depths_, model.depths.data(), 4, up_splits_, S);
    up.append(m_feature_indices_, model.feature_indices.data(), 4, up_splits_ * MD, S * MD);
    up.append(m_feature_values_, model.feature_values.data(), 4, up_splits_ * MD, S * MD);
    up.append(m_is_numerics_, model.is_numerics.data(), 1, up_splits_ * MD, S * MD);
    up.append(m_cat_ids_, cat_ids_host_.data(), 4, up_splits_ * MD, S * MD);
    up.append(m_cond_pack_, cond_pack_host_.data(), 4, up_splits_ * MD * 2, S * MD * 2);
    up.append(m_values_, model.values.data(), 4, up_leaves_ * D, L * D);
    up.append(m_ineq_, model.inequality_directions.data(), 1, up_leaves_ * MD, L * MD);
    // 3. the derived records (mirror_records.h); the value records are rebuilt from vt0 (rewind_values; else only the new trees)
    const size_t vt0 = std::min(up_trees_, values_redo_tree_);
    if (model.oblivious() && kern::obl2_feasible(md.max_depth, md.output_dim, false)) {
        const detail::RecordShape sh = record_shape(md, false);
        detail::extend_oblivious_records(model, cond_pack_host_, sh, up_trees_, vt0, cond_ra_host_, values_sw_host_);
        up.append(m_cond_ra_, cond_ra_host_.data(), 4, up_trees_ * 2 * sh.MX, (T + detail::kPadTrees) * 2 * sh.MX);
        up.append_padded(m_values_sw_, values_sw_host_.data(), vt0, T, sh.rec(), sh.pad());
    }
    if (!model.oblivious()) {
        if (up_trees_ == 0) grd_.reset();
        for (size_t t = up_trees_; t < T; ++t) grd_.append_tree(model, cat_ids_host_, t);
        up.append(m_grd_nodes_, grd_.nodes.data(), 4, grd_up_nodes_ * 4, grd_.nodes.size());
        up.append(m_grd_off_, grd_.off.data(), 4, 0, grd_.off.size());
        if (grd_.ok && kern::obl2_feasible(md.max_depth, md.output_dim, true)) {
            const detail::RecordShape sh = record_shape(md, true);
            detail::extend_greedy_records(model, grd_, sh, up_trees_, vt0, values_sw_host_);
            up.append_padded(m_values_sw_, values_sw_host_.data(), vt0, T, sh.rec(), sh.pad());
        }
    }
    // 4. small, mutable state: always refreshed
    up.append(m_bias_, model.bias.data(), 4, 0, D);
    std::vector<int32_t> os, oe;
    std::vector<float> olr;
    for (const auto &o : model.opts) { os.push_back(o.start_idx); oe.push_back(o.stop_idx); olr.push_back(o.init_lr); }  // ConstScheduler::get_lr
    up.append(m_opt_start_, os.data(), 4, 0, os.size());
    up.append(m_opt_stop_, oe.data(), 4, 0, oe.size());
    up.append(m_opt_lr_, olr.data(), 4, 0, olr.size());
    if (model.scheduled()) {
        const size_t rate_from = rate_.extend(model, rate_trees_);
        up.append(m_rate_, rate_.rate.data(), 4, rate_from * model.opts.size(), T * model.opts.size());
    } else {
        rate_.opts.clear();
    }
    // 5. one copy for all of it
    up.flush();
    // 6. the marks
    up_trees_ = T; up_leaves_ = L; up_splits_ = S;
    values_redo_tree_ = kNoRedo;
    grd_up_nodes_ = grd_.nodes.size() / 4;
    rate_trees_ = model.scheduled() ? T : 0;
    mirror_version_ = model.version;
}

// The code book of the packed-code predict path (detail::build_pc_book has the encoding).  Rebuilt from the host model whenever it has
// changed (a new threshold shifts the ranks of its feature).
bool Engine::ensure_pc_book(int n_num, int n_cat) {
    if (pc_version_ == model.version && pc_f_ == n_num && pc_fc_ == n_cat) return pc_ok_;
    pc_version_ = model.version; pc_f_ = n_num; pc_fc_ = n_cat; pc_ok_ = false;
    const detail::PcBook b = detail::build_pc_book(model, cat_ids_host_, cat_dict_.size(), n_num, n_cat, static_cast<size_t>(kern::obl2_levels(model.meta.max_depth)),
                                                   kern::predict_pc_bank_words());
    if (!b.ok) return false;
    upload(m_pc_cond_, b.cond.data(), b.cond.size(), "H2D code book");
    upload(m_pc_thr_, b.thr.data(), b.thr.size(), "H2D code book");
    upload(m_pc_thr_off_, b.thr_off.data(), b.thr_off.size(), "H2D code book");
    upload(m_pc_cat_slot_, b.cat_slot.data(), b.cat_slot.size(), "H2D code book");
    upload(m_pc_word_cols_, b.word_cols.data(), b.word_cols.size(), "H2D code book");
    hip_check(hipStreamSynchronize(stream_), "sync code book");   // the host vectors go out of scope
    pc_wn_ = b.wn; pc_nw_ = b.nw; pc_row_words_ = b.row_words; pc_iters_ = b.iters;
    pc_ok_ = true;
    return true;
}

// Dictionary ids of a batch of categorical cells (0 = a category no condition of the model mentions).  Needs sync_model_to_device().
int32_t *Engine::encode_categorical_batch(const char *cat, bool cat_dev, int n, int n_cat) {
    hipStream_t s = stream_;
    int32_t *dcat = nullptr;
    // dictionary encoding on the device: the cells are hashed (strcmp semantics: bytes before the first NUL), looked up in
    // the per-feature, hash-sorted dictionary of the categories the model's conditions mention, and confirmed word by word
    const char *dcells = cat;
    if (!cat_dev) {
        char *tmp = static_cast<char *>(d_pcells_.ensure(static_cast<size_t>(n) * n_cat * kCat));
        hip_check(hipMemcpyAsync(tmp, cat, static_cast<size_t>(n) * n_cat * kCat, hipMemcpyHostToDevice, s), "H2D cat cells");
        dcells = tmp;
    }
    if (dict_version_ != cat_dict_.size() || dict_fc_ != n_cat) {
        struct E { uint64_t h; int id; uint64_t w[16]; };
        std::vector<std::vector<E>> per(n_cat);
        for (size_t z = 0; z < cat_dict_.size(); ++z) {
            const int f = cat_dict_[z].first;
            if (f < 0 || f >= n_cat) continue;
            E e{};
            uint64_t raw[16];
            std::memcpy(raw, cat_dict_[z].second.data(), kCat);
            e.h = cat_cell_hash(raw, e.w);
            e.id = static_cast<int>(z) + 1;
            per[f].push_back(e);
        }
        std::vector<int32_t> off(n_cat + 1, 0), ids;
        std::vector<uint64_t> hs, ws;
        for (int f = 0; f < n_cat; ++f) {
            std::sort(per[f].begin(), per[f].end(), [](const E &a, const E &b) { return a.h < b.h || (a.h == b.h && a.id < b.id); });
            for (const E &e : per[f]) { hs.push_back(e.h); ids.push_back(e.id); ws.insert(ws.end(), e.w, e.w + 16); }
            off[f + 1] = static_cast<int32_t>(hs.size());
        }
        hs.push_back(0); ids.push_back(0); ws.resize(ws.size() + 16, 0);   // never empty
        hip_check(hipMemcpyAsync(d_dict_off_.ensure(off.size() * 4), off.data(), off.size() * 4, hipMemcpyHostToDevice, s), "H2D dict");
        hip_check(hipMemcpyAsync(d_dict_hash_.ensure(hs.size() * 8), hs.data(), hs.size() * 8, hipMemcpyHostToDevice, s), "H2D dict");
        hip_check(hipMemcpyAsync(d_dict_id_.ensure(ids.size() * 4), ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s), "H2D dict");
        hip_check(hipMemcpyAsync(d_dict_words_.ensure(ws.size() * 8), ws.data(), ws.size() * 8, hipMemcpyHostToDevice, s), "H2D dict");
        hip_check(hipStreamSynchronize(s), "sync");   // the host vectors go out of scope
        dict_version_ = cat_dict_.size();
        dict_fc_ = n_cat;
    }
    dcat = static_cast<int32_t *>(d_pcat_.ensure(sizeof(int32_t) * static_cast<size_t>(n) * n_cat));
    kern::encode_categories(dcells, n, n_cat, d_dict_off_.as<int32_t>(), d_dict_hash_.as<uint64_t>(), d_dict_id_.as<int32_t>(),
                            d_dict_words_.as<uint64_t>(), dcat, s);
    return dcat;
}

uint64_t Engine::cat_dict_token() {
    if (dict_token_size_ != cat_dict_.size()) {
        uint64_t h = 0xcbf29ce484222325ull;      // FNV-1a over (feature, 128-byte category) in dictionary order
        auto mix = [&](const void *p, size_t nbytes) { const unsigned char *b = static_cast<const unsigned char *>(p); for (size_t i = 0; i < nbytes; ++i) { h ^= b[i]; h *= 0x100000001b3ull; } };
        for (const auto &e : cat_dict_) {
            const int32_t f = e.first;
            char cell[kCat] = {0};
            std::memcpy(cell, e.second.data(), std::min<size_t>(kCat, e.second.size()));
            mix(&f, sizeof(f));
            mix(cell, kCat);
        }
        const uint64_t n_entries = cat_dict_.size();
        mix(&n_entries, sizeof(n_entries));
        dict_token_ = h;
        dict_token_size_ = cat_dict_.size();
    }
    return dict_token_;
}

void Engine::encode_categorical(const char *cat, bool cat_dev, int n, int n_cat, int32_t *ids_out, bool out_dev, uint64_t *token) {
    gbrl_hip_metadata &md = model.meta;
    if (n <= 0 || n_cat <= 0 || cat == nullptr || ids_out == nullptr) throw InvalidArgument("encode_categorical: no cells");
    if (md.iteration != 0 && n_cat != md.n_cat_features) throw InvalidArgument("Incompatible dataset");
    ensure_device();
    sync_model_to_device();
    hipStream_t s = stream_;
    const int32_t *dcat = encode_categorical_batch(cat, cat_dev, n, n_cat);
    hip_check(hipMemcpyAsync(ids_out, dcat, sizeof(int32_t) * static_cast<size_t>(n) * n_cat, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s), "ids out");
    hip_check(hipStreamSynchronize(s), "sync");
    if (token) *token = cat_dict_token();
}

kern::PredictModel Engine::mirror_view() {
    const gbrl_hip_metadata &md = model.meta;
    const int D = md.output_dim;
    kern::PredictModel pm{};   // (no packed codes, no partial sums, no chain slots: predict() offers those itself)
    pm.tree_indices = m_tree_indices_.as<int32_t>();
    pm.depths = m_depths_.as<int32_t>();
    pm.feature_indices = m_feature_indices_.as<int32_t>();
    pm.cat_ids = m_cat_ids_.as<int32_t>();
    pm.feature_values = m_feature_values_.as<float>();
    pm.values = m_values_.as<float>();
    pm.bias = m_bias_.as<float>();
    pm.is_numerics = m_is_numerics_.as<uint8_t>();
    pm.inequality_directions = m_ineq_.as<uint8_t>();
    pm.n_trees = md.n_trees; pm.n_leaves = md.n_leaves; pm.max_depth = md.max_depth; pm.D = D;
    pm.oblivious = model.oblivious() ? 1 : 0;
    pm.n_opts = static_cast<int>(model.opts.size());
    pm.opt_start = m_opt_start_.as<int32_t>();
    pm.opt_stop = m_opt_stop_.as<int32_t>();
    pm.opt_lr = m_opt_lr_.as<float>();
    pm.cond_pack = m_cond_pack_.as<int32_t>();
    pm.grd_nodes = m_grd_nodes_.as<int32_t>();
    pm.grd_node_off = m_grd_off_.as<int32_t>();
    pm.grd_ok = (!model.oblivious() && grd_.ok) ? 1 : 0;
    pm.grd_max_nodes = grd_.max_nodes;
    pm.grd_max_leaves = grd_.max_leaves;
    pm.obl_ok = model.oblivious() ? 1 : 0;
    pm.cat_dict_size = static_cast<int>(cat_dict_.size());
    if (model.oblivious() && kern::obl2_feasible(md.max_depth, D, false) && md.n_trees > 0) {
        pm.obl2_maxd = kern::obl2_levels(md.max_depth);
        pm.values_sw = m_values_sw_.as<float>();
        pm.cond_ra = m_cond_ra_.as<int32_t>();
    } else if (!model.oblivious() && grd_.ok && kern::obl2_feasible(md.max_depth, D, true) && md.n_trees > 0) {
        pm.obl2_maxd = kern::obl2_levels(md.max_depth);   // greedy mode of the same kernel: records = values + nodes
        pm.values_sw = m_values_sw_.as<float>();
    }
    if (const char *e = hooks::raw(hooks::PREDICT_OBL1)) {      // test / measurement hook: the first-generation oblivious kernel
        if (e[0] == '1') pm.obl2_maxd = 0;
    }
    if (const char *e = hooks::raw(hooks::PREDICT_GENERIC)) {   // test hook: the general kernels only
        if (e[0] == '1') { pm.grd_ok = 0; pm.obl_ok = 0; }
    }
    pm.coef_ok = D <= 64 ? 1 : 0;
    for (size_t oi = 0; oi < model.opts.size(); ++oi) {   // one learning rate per output unless two optimisers share an output
        const auto &o = model.opts[oi];
        for (int j = o.start_idx; j < o.stop_idx && pm.coef_ok; ++j) {
            if (j < 0 || j >= D || ((pm.coef_cover >> j) & 1ull)) { pm.coef_ok = 0; break; }
            pm.coef_cover |= 1ull << j;
            pm.coef[j] = o.init_lr;
            pm.owner[j] = static_cast<uint8_t>(oi);
        }
    }
    if (model.opts.size() > 255) pm.coef_ok = pm.coef_ok && !model.scheduled();   // (owner is a byte; D <= 64 bounds the optimizers of a covered model anyway)
    // Linear schedules: the kernels of predict_sched.hip read the rate of (tree, optimizer) from the mirror's table
    pm.rate = (model.scheduled() && md.n_trees > 0) ? m_rate_.as<float>() : nullptr;
    return pm;
}

}  // namespace gbrl
