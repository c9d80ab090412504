// mirror_records.h -- the host half of the device mirror of the ensemble: every record the predict kernels read that is DERIVED from the host
// Model, each rule written once.  No device, no HIP header, plain C++17 over model.h:
//   - dictionary ids of the categorical conditions (extend_cat_ids) and the packed condition pair (packed_condition, extend_cond_pack);
//   - the second-generation records (predict_obl2.hip): their shape and swizzle (RecordShape), the oblivious record of a tree and the padding
//     trees (extend_oblivious_records), the greedy node records (GreedyNodes) and the greedy record of a tree (extend_greedy_records);
//   - the learning-rate table of Linear schedules (RateTable);
//   - the code book of the packed-code path (build_pc_book).
// The engine (engine_mirror.hip) keeps the upload marks and appends what these build; tests/cxx/mirror_records_check.cpp checks them against
// the model's own per-leaf rule on random ensembles (compiled and run by tests/test_host.py).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "model.h"

namespace gbrl {
namespace detail {

constexpr size_t kPadTrees = 32;   // the kernels fetch whole groups of records (<= 32 trees) past the last tree

inline int32_t float_bits(float v) {
    int32_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

// ---------------------------------------------------------------------------------------------------------- conditions
// (categorical feature, 128-byte category) -> id >= 1, in order of first appearance: strings are compared on the host once, the device compares ids
using CatDict = std::vector<std::pair<int, std::string>>;

// The ids of the categorical conditions of the split rows [from_split, S); a category the dictionary does not hold yet joins it.
inline void extend_cat_ids(const Model &model, size_t from_split, CatDict &dict, std::vector<int32_t> &cat_ids) {
    const size_t S = model.split_rows(), MD = model.meta.max_depth;
    cat_ids.resize(S * MD, 0);
    for (size_t c = from_split * MD; c < S * MD; ++c) {
        if (model.is_numerics[c]) continue;
        const int f = model.feature_indices[c];
        std::string name(&model.categorical_values[c * kCat], kCat);
        int id = 0;
        for (size_t z = 0; z < dict.size(); ++z)
            if (dict[z].first == f && dict[z].second == name) { id = static_cast<int>(z) + 1; break; }
        if (id == 0) { dict.emplace_back(f, name); id = static_cast<int>(dict.size()); }
        cat_ids[c] = id;
    }
}

// Condition c as the kernels read it through the scalar cache: (feature, threshold bits) when numeric, (~feature, category id) when categorical.
struct PackedCondition { int32_t key, arg; };
inline PackedCondition packed_condition(const Model &model, const std::vector<int32_t> &cat_ids, size_t c) {
    if (model.is_numerics[c]) return {model.feature_indices[c], float_bits(model.feature_values[c])};
    return {~model.feature_indices[c], cat_ids[c]};
}

inline void extend_cond_pack(const Model &model, const std::vector<int32_t> &cat_ids, size_t from_split, std::vector<int32_t> &cond_pack) {
    const size_t S = model.split_rows(), MD = model.meta.max_depth;
    cond_pack.resize(S * MD * 2, 0);
    for (size_t c = from_split * MD; c < S * MD; ++c) {
        const PackedCondition p = packed_condition(model, cat_ids, c);
        cond_pack[2 * c] = p.key;
        cond_pack[2 * c + 1] = p.arg;
    }
}

// --------------------------------------------------------------------------------------- second-generation records
// One record per tree, in dwords: the leaf values of 2^levels leaves (the kernel's tree stride is a compile-time constant) pre-swizzled as
// [worker][leaf][DMAX/4], and in greedy mode the tree's node records [2^levels] x int4 behind them.  The kernels load whole groups of records
// and up to 4 x 1024 x 16 bytes per block unconditionally: zero padding of pad() dwords follows the last tree.
struct RecordShape {
    size_t MX, DMAX;   // levels (kern::obl2_levels) and padded outputs (kern::obl2_padded_outputs)
    bool greedy;
    size_t DW() const { return DMAX / 4; }
    size_t LS() const { return size_t(1) << MX; }
    size_t VT() const { return LS() * DMAX; }
    size_t rec() const { return VT() + (greedy ? LS() * 4 : 0); }
    size_t pad() const { return kPadTrees * rec() + (size_t(64) << 10) / sizeof(float); }
    size_t swizzle(size_t leaf, size_t j) const { return ((j / DW()) * LS() + leaf) * DW() + (j % DW()); }
    void put_values(const Model &model, size_t t, size_t n_leaves, float *rec_out) const {
        const size_t l0 = model.first_leaf(static_cast<int>(t)), D = model.meta.output_dim;
        for (size_t leaf = 0; leaf < n_leaves && leaf < LS(); ++leaf)
            for (size_t j = 0; j < D; ++j) rec_out[swizzle(leaf, j)] = model.values[(l0 + leaf) * D + j];
    }
};

// the condition pair no row passes: in front of a shallow tree, and for every level of the padding trees
inline void put_never(int32_t *pair) { pair[0] = 0; pair[1] = float_bits(std::numeric_limits<float>::infinity()); }

// Oblivious ensembles: per tree MX condition pairs RIGHT-aligned (cond_ra, kPadTrees padding trees behind the last) and a value record
// (values_sw).  `up_trees` trees are on the device already (0: start over); the records of [from_tree, T) are (re)built, from_tree <= up_trees.
inline void extend_oblivious_records(const Model &model, const std::vector<int32_t> &cond_pack, const RecordShape &sh, size_t up_trees, size_t from_tree,
                                     std::vector<int32_t> &cond_ra, std::vector<float> &values_sw) {
    const size_t T = model.meta.n_trees, MD = model.meta.max_depth, MX = sh.MX, VT = sh.VT();
    if (up_trees == 0) { cond_ra.clear(); values_sw.clear(); }
    cond_ra.resize((T + kPadTrees) * 2 * MX);
    values_sw.resize(T * VT + sh.pad());
    std::fill(values_sw.begin() + static_cast<long>(from_tree * VT), values_sw.end(), 0.0f);
    for (size_t t = from_tree; t < T; ++t) {
        const size_t depth = static_cast<size_t>(model.depths[t]);
        int32_t *cr = &cond_ra[t * 2 * MX];
        for (size_t d = 0; d < MX - depth; ++d) put_never(cr + 2 * d);
        std::copy_n(&cond_pack[2 * t * MD], 2 * depth, cr + 2 * (MX - depth));
        sh.put_values(model, t, size_t(1) << depth, &values_sw[t * VT]);
    }
    for (size_t p = T * MX; p < (T + kPadTrees) * MX; ++p) put_never(&cond_ra[2 * p]);
}

// Greedy ensembles: every tree rebuilt as a binary tree from its leaves' paths (leaves are stored depth-first, left first; fitter.cpp:364-365),
// for the descent of k_predict_grd.  A node is (packed condition, left, right); a child code >= 0 is a node of the tree, ~leaf a leaf of it.
// A tree whose leaves do not form a proper binary tree (a hand-edited model file), or a one-leaf tree (Q7), adds no node and switches the
// fast path off for the whole ensemble.
struct GreedyNodes {
    std::vector<int32_t> nodes;   // [n][4]
    std::vector<int32_t> off;     // [T + 1] first node of a tree
    bool ok = true;
    int max_nodes = 0, max_leaves = 1;

    void reset() { nodes.clear(); off.assign(1, 0); ok = true; max_nodes = 0; max_leaves = 1; }

    void append_tree(const Model &model, const std::vector<int32_t> &cat_ids, size_t t) {
        const int l0 = static_cast<int>(model.first_leaf(static_cast<int>(t))), l1 = l0 + static_cast<int>(model.leaf_count(static_cast<int>(t)));
        Build b{model, cat_ids, l0, nodes.size() / 4, l1 - l0 > 1};   // (one leaf: it never passes in the reference, Q7)
        if (b.ok && build(b, l0, l1, 0) != 0) b.ok = false;           // the root must be node 0
        if (!b.ok) { ok = false; nodes.resize(b.base * 4); }
        off.push_back(static_cast<int32_t>(nodes.size() / 4));
        max_nodes = std::max<int>(max_nodes, static_cast<int>(nodes.size() / 4 - b.base));
        max_leaves = std::max(max_leaves, l1 - l0);
    }

   private:
    struct Build { const Model &model; const std::vector<int32_t> &cat_ids; int l0; size_t base; bool ok; };

    // same condition at depth d for the leaves a and b?
    static bool same_cond(const Build &b, int la, int lb, int d) {
        const Model &m = b.model;
        const size_t MD = m.meta.max_depth, ca = static_cast<size_t>(la) * MD + d, cb = static_cast<size_t>(lb) * MD + d;
        if (m.is_numerics[ca] != m.is_numerics[cb] || m.feature_indices[ca] != m.feature_indices[cb]) return false;
        if (m.is_numerics[ca]) return std::memcmp(&m.feature_values[ca], &m.feature_values[cb], 4) == 0;
        return b.cat_ids[ca] == b.cat_ids[cb];
    }

    // the leaves [lo, hi) share their first d conditions; returns the child code
    int build(Build &b, int lo, int hi, int d) {
        const Model &m = b.model;
        const size_t MD = m.meta.max_depth;
        if (!b.ok) return -1;
        if (hi - lo == 1) {
            if (m.depths[lo] != d) b.ok = false;
            return ~(lo - b.l0);
        }
        if (d >= static_cast<int>(MD)) { b.ok = false; return -1; }
        int mid = lo;
        for (int q = lo; q < hi; ++q) {
            if (m.depths[q] <= d || !same_cond(b, lo, q, d)) { b.ok = false; return -1; }
            const bool right = m.inequality_directions[static_cast<size_t>(q) * MD + d] != 0;
            if (!right) { if (q != mid) { b.ok = false; return -1; } ++mid; }   // left leaves first, contiguous
        }
        if (mid == lo || mid == hi) { b.ok = false; return -1; }
        const size_t me = nodes.size() / 4 - b.base;
        nodes.insert(nodes.end(), {0, 0, 0, 0});
        const int left = build(b, lo, mid, d + 1), right = build(b, mid, hi, d + 1);
        const PackedCondition p = packed_condition(m, b.cat_ids, static_cast<size_t>(lo) * MD + d);
        int32_t *nd = &nodes[(b.base + me) * 4];   // (the children have grown the array)
        nd[0] = p.key; nd[1] = p.arg; nd[2] = left; nd[3] = right;
        return static_cast<int>(me);
    }
};

// Greedy mode of the second-generation kernel: the record of a tree is its swizzled values followed by its nodes, copied only when they fit
// the 2^levels slots (a larger tree never takes this kernel).  Marks as in extend_oblivious_records.
inline void extend_greedy_records(const Model &model, const GreedyNodes &grd, const RecordShape &sh, size_t up_trees, size_t from_tree,
                                  std::vector<float> &values_sw) {
    const size_t T = model.meta.n_trees, REC = sh.rec();
    if (up_trees == 0) values_sw.clear();
    values_sw.resize(T * REC + sh.pad());
    std::fill(values_sw.begin() + static_cast<long>(from_tree * REC), values_sw.end(), 0.0f);
    for (size_t t = from_tree; t < T; ++t) {
        float *rec = &values_sw[t * REC];
        sh.put_values(model, t, model.leaf_count(static_cast<int>(t)), rec);
        const size_t n0 = static_cast<size_t>(grd.off[t]), n1 = static_cast<size_t>(grd.off[t + 1]);
        if (n1 - n0 <= sh.LS()) std::memcpy(rec + sh.VT(), grd.nodes.data() + n0 * 4, (n1 - n0) * 16);
    }
}

// ---------------------------------------------------------------------------------------------------------- rate table
// Linear schedules: rate[t][optimizer] = scheduler_lr for every tree.  A tree's rate never changes, so rows are only appended -- unless the
// optimizers are not the ones the table was built from, or the ensemble has shrunk below it: then it starts over.
struct RateTable {
    std::vector<float> rate;
    std::vector<gbrl_hip_optimizer> opts;   // the optimizers the table was built from

    // `built` rows are current (and on the device); returns the first row that was (re)built
    size_t extend(const Model &model, size_t built) {
        const size_t T = model.meta.n_trees, NO = model.opts.size();
        const bool same = opts.size() == NO && std::memcmp(opts.data(), model.opts.data(), NO * sizeof(gbrl_hip_optimizer)) == 0;
        if (!same || built > T) { built = 0; opts = model.opts; }
        rate.resize(std::max<size_t>(T, 1) * NO, 0.0f);
        for (size_t t = built; t < T; ++t)
            for (size_t o = 0; o < NO; ++o) rate[t * NO + o] = scheduler_lr(model.opts[o], static_cast<int>(t));
        return built;
    }
};

// ----------------------------------------------------------------------------------------------------- packed-code book
// The code book of the packed-code predict path (kern::predict_pc, predict_reg.hip).  Every numeric condition `x > t` of the ensemble becomes
// `field < (0xffff - rank(t)) << 16`, where the field of a row is 0xffff - #{distinct thresholds of the feature below x}; every categorical
// condition `cell == category` becomes "bit `slot` of the row's inverted one-hot words is clear".  Per tree level a (word, shift, T) record,
// right-aligned like cond_ra; conditions that can never pass (threshold +inf or NaN, the padding in front of a shallow tree) are (0, 0, 0).
struct PcBook {
    bool ok = false;                   // false: the ensemble is not expressible for these feature counts
    std::vector<int32_t> cond;         // [(T + kPadTrees)][levels][3]
    std::vector<float> thr;            // per numeric feature its sorted distinct thresholds (+ one element: never empty)
    std::vector<int32_t> thr_off;      // [n_num + 1]
    std::vector<int32_t> cat_slot;     // [dict_size + 1] bit slot of a dictionary id, -1: no condition of these columns mentions it
    std::vector<int32_t> word_cols;    // per one-hot word the [first, last) categorical columns with a slot in it
    int wn = 0, nw = 0, row_words = 0, iters = 1;   // numeric words, all words, words per packed row, steps of the rank descent
};

inline PcBook build_pc_book(const Model &model, const std::vector<int32_t> &cat_ids, size_t dict_size, int n_num, int n_cat, size_t levels, int bank_words) {
    PcBook b;
    const size_t T = model.meta.n_trees, MD = model.meta.max_depth, MX = levels;
    if (MX == 0 || T == 0) return b;
    auto never = [](float v) { return v != v || v == std::numeric_limits<float>::infinity(); };
    std::vector<std::vector<float>> thr(n_num);
    std::vector<std::vector<int32_t>> ids(n_cat);
    for (size_t t = 0; t < T; ++t) {
        const size_t depth = static_cast<size_t>(model.depths[t]);
        if (depth > MX) return b;
        for (size_t d = 0; d < depth; ++d) {
            const size_t c = t * MD + d;
            const int f = model.feature_indices[c];
            if (model.is_numerics[c]) {
                if (f < 0 || f >= n_num) return b;
                const float v = model.feature_values[c];
                if (!never(v)) thr[f].push_back(v == 0.0f ? 0.0f : v);   // -0 and +0 are one threshold
            } else {
                if (f < 0 || f >= n_cat || cat_ids[c] <= 0) return b;
                ids[f].push_back(cat_ids[c]);
            }
        }
    }
    b.thr_off.assign(n_num + 1, 0);
    size_t max_m = 1;
    for (int f = 0; f < n_num; ++f) {
        std::sort(thr[f].begin(), thr[f].end());
        thr[f].erase(std::unique(thr[f].begin(), thr[f].end()), thr[f].end());
        if (thr[f].size() > 65534) return b;
        max_m = std::max(max_m, thr[f].size());
        b.thr.insert(b.thr.end(), thr[f].begin(), thr[f].end());
        b.thr_off[f + 1] = static_cast<int32_t>(b.thr.size());
    }
    b.thr.push_back(0.0f);   // never empty
    while ((size_t(1) << b.iters) <= max_m) ++b.iters;   // 2^iters > max_m: the descent can reach every count 0..max_m
    b.cat_slot.assign(dict_size + 1, -1);
    std::vector<int32_t> col_first_slot(n_cat + 1, 0);
    int n_slots = 0;
    for (int c = 0; c < n_cat; ++c) {
        std::sort(ids[c].begin(), ids[c].end());
        ids[c].erase(std::unique(ids[c].begin(), ids[c].end()), ids[c].end());
        col_first_slot[c] = n_slots;
        for (int32_t id : ids[c]) {
            if (id >= static_cast<int32_t>(b.cat_slot.size())) return b;
            b.cat_slot[id] = n_slots++;
        }
    }
    col_first_slot[n_cat] = n_slots;
    const int cw = (n_slots + 31) / 32;
    b.wn = (n_num + 1) / 2; b.nw = b.wn + cw; b.row_words = (b.nw + 3) & ~3;
    if (b.row_words > bank_words || b.row_words == 0) return b;
    b.word_cols.assign(2 * std::max(cw, 1), 0);
    for (int q = 0; q < cw; ++q) {
        int first = n_cat, last = 0;
        for (int c = 0; c < n_cat; ++c)
            if (col_first_slot[c + 1] > 32 * q && col_first_slot[c] < 32 * (q + 1) && col_first_slot[c + 1] > col_first_slot[c]) { first = std::min(first, c); last = std::max(last, c + 1); }
        b.word_cols[2 * q] = first; b.word_cols[2 * q + 1] = std::max(first, last);
    }
    b.cond.assign((T + kPadTrees) * MX * 3, 0);
    for (size_t t = 0; t < T; ++t) {
        const size_t depth = static_cast<size_t>(model.depths[t]);
        int32_t *r = &b.cond[(t * MX + (MX - depth)) * 3];
        for (size_t d = 0; d < depth; ++d, r += 3) {
            const size_t c = t * MD + d;
            const int f = model.feature_indices[c];
            if (model.is_numerics[c]) {
                const float v0 = model.feature_values[c];
                if (never(v0)) continue;   // (0, 0, 0): never true
                const float v = v0 == 0.0f ? 0.0f : v0;
                const size_t k = static_cast<size_t>(std::lower_bound(thr[f].begin(), thr[f].end(), v) - thr[f].begin());
                r[0] = f >> 1;
                r[1] = (f & 1) ? 0 : 16;
                r[2] = static_cast<int32_t>(static_cast<uint32_t>(0xffffu - k) << 16);
            } else {
                const int slot = b.cat_slot[cat_ids[c]];
                r[0] = b.wn + (slot >> 5);
                r[1] = 31 - (slot & 31);
                r[2] = static_cast<int32_t>(0x80000000u);
            }
        }
    }
    b.ok = true;
    return b;
}

}  // namespace detail
}  // namespace gbrl
