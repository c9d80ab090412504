// cat_candidates_host.h -- the host half of a step's categorical split candidates (A5): no device, no HIP header, plain C++17.
//   - the reference's own rule on every cell of a batch (categorical_candidates: processCategoricalCandidates, split_candidate_generator.cpp:117-163);
//   - the same result from the list of DISTINCT cells a device scan publishes (feature, row of first occurrence, raw hash, the 128 bytes,
//     and count / float32 row-order total of the squared gradient norms when there are more of them than candidates are kept):
//     first_occurrence_order -> CatMemory::replay -> keep_top_by_mean -> assign_classes.
// tests/cxx/cat_candidates_check.cpp runs the second against the first on random batches (compiled and run by tests/test_host.py).
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "hash_order_replay.h"

namespace gbrl {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };

namespace detail {

constexpr int kCell = 128;   // bytes of a categorical cell (GBRL_HIP_MAX_CHAR_SIZE, types.h:55-58)

// a categorical split candidate: class `cls` of feature `feat` is the category `name` (the raw 128-byte cell, types.h:55-58)
struct CatCandidate {
    int feat;
    std::array<char, kCell> name;
    int cls;
    CatCandidate(int f, const char *cell, int c) : feat(f), cls(c) { std::memcpy(name.data(), cell, kCell); }
};
// A distinct (categorical feature, cell) pair the engine has met in some step: the hash of its key in the reference's candidate
// container (std::hash of cell + "_" + feature, split_candidate_generator.cpp:121) is computed once.
struct CatItem { int feat; int next; uint64_t lhash; size_t std_hash; char name[kCell]; };

inline std::string cat_key(const char *cell, int feat) {   // the reference's container key
    std::string key(cell, kCell);
    key += "_" + std::to_string(feat);
    return key;
}

// calculate_squared_norm (math_ops.cpp:726-749), contracted like the reference build
inline std::vector<float> squared_norms(const float *grads, int N, int D) {
    std::vector<float> norms(N, 0.0f);
    for (int i = 0; i < N; ++i) {
        float acc = 0.0f;
        for (int d = 0; d < D; ++d) { const float g = grads[static_cast<size_t>(i) * D + d]; acc = fmaf(g, g, acc); }
        norms[i] = acc;
    }
    return norms;
}

// split_candidate_generator.cpp:131-150: more (key, mean) pairs than candidates are kept -- std::sort by descending mean, the first `keep`
// survive.  The comparator reads the means only, so the element moves (and with them the order among equal means, which the reference's
// candidate order depends on) are the same whatever the key is: the reference's string, or an index standing for it.  Not a stable sort.
template <class Key>
void keep_top_by_mean(std::vector<std::pair<Key, float>> &vec, size_t keep) {
    if (vec.size() <= keep) return;
    std::sort(vec.begin(), vec.end(), [](const std::pair<Key, float> &a, const std::pair<Key, float> &b) { return a.second > b.second; });
    vec.resize(keep);
}

// split_candidate_generator.cpp:151-161: the kept candidates, in their order, are numbered 1.. within their feature.  kept(k) = (feature,
// cell bytes) of the k-th; each(k, cls) is told its class (where the caller books the class of a cell).
template <class Kept, class Each>
void assign_classes(size_t n, Kept kept, std::vector<CatCandidate> &cat_cands, std::vector<int> &cat_classes, Each each) {
    cat_cands.reserve(cat_cands.size() + n);
    for (size_t k = 0; k < n; ++k) {
        const std::pair<int, const char *> fc = kept(k);
        const int cls = ++cat_classes[fc.first];
        if (cls > 65534) throw Unsupported("more than 65534 candidate categories in one feature");
        cat_cands.emplace_back(fc.first, fc.second, cls);
        each(k, cls);
    }
}

// ---- A5 on every cell of the batch, exactly as processCategoricalCandidates (split_candidate_generator.cpp:117-163): same container, same
// insertion order => same candidate order (Q8).  cat_classes[f] = number of candidate categories of feature f (class ids 1..),
// h_catcodes[i*Fc+f] = class of the cell (0: not a candidate).
inline void categorical_candidates(const char *hcat, const float *hgrads, int N, int Fc, int D, int B, std::vector<CatCandidate> &cat_cands,
                                   std::vector<uint16_t> &h_catcodes, std::vector<int> &cat_classes) {
    struct Info { float total = 0.f; int count = 0; int feat = 0; std::string name; };
    const std::vector<float> norms = squared_norms(hgrads, N, D);
    std::unordered_map<std::string, Info> uniq;
    for (int f = 0; f < Fc; ++f)
        for (int i = 0; i < N; ++i) {
            std::string name(hcat + (static_cast<size_t>(i) * Fc + f) * kCell, kCell);
            Info &ci = uniq[name + "_" + std::to_string(f)];
            ci.total += norms[i];
            ci.count += 1;
            ci.feat = f;
            ci.name = name;
        }
    std::vector<std::pair<std::string, float>> vec;
    for (const auto &kv : uniq) vec.emplace_back(kv.first, kv.second.total / kv.second.count);
    keep_top_by_mean(vec, static_cast<size_t>(Fc) * B);
    std::unordered_map<std::string, int> cls_of;  // key -> class id within its feature
    assign_classes(vec.size(), [&](size_t k) { const Info &ci = uniq[vec[k].first]; return std::make_pair(ci.feat, ci.name.data()); },
                   cat_cands, cat_classes, [&](size_t k, int cls) { cls_of[vec[k].first] = cls; });
    h_catcodes.assign(static_cast<size_t>(N) * Fc, 0);
    for (int i = 0; i < N; ++i)
        for (int f = 0; f < Fc; ++f) {
            auto it = cls_of.find(cat_key(hcat + (static_cast<size_t>(i) * Fc + f) * kCell, f));
            if (it != cls_of.end()) h_catcodes[static_cast<size_t>(i) * Fc + f] = static_cast<uint16_t>(it->second);
        }
}

// The reference's insertion order of n distinct cells: feature-major, then row of first occurrence -- one LSD radix sort (11-bit digits) of
// feature * N + first row with the list index in the low 21 bits (std::sort of the per-feature buckets: 30 us at 64 columns x 4096 rows).
// max_per_feature: the largest distinct count of one feature (the table-size hint of the next scan).
struct FirstOccurrence { std::vector<int> order; int max_per_feature = 1; };
inline FirstOccurrence first_occurrence_order(const int32_t *lfeat, const int32_t *lfirst, int n, int N, int Fc) {
    if (n > (1 << 21)) throw Unsupported("more than 2^21 distinct categorical cells in one step");   // (the list index rides in the key's low 21 bits)
    FirstOccurrence fo;
    std::vector<int> per_feat(Fc, 0);
    for (int q = 0; q < n; ++q) ++per_feat[lfeat[q]];
    for (int f = 0; f < Fc; ++f) fo.max_per_feature = std::max(fo.max_per_feature, per_feat[f]);
    std::vector<uint64_t> ka(n), kb(n);
    for (int q = 0; q < n; ++q)
        ka[q] = ((static_cast<uint64_t>(lfeat[q]) * static_cast<uint64_t>(N) + static_cast<uint64_t>(lfirst[q])) << 21) | static_cast<uint64_t>(q);
    int key_bits = 1;
    while (key_bits < 43 && (static_cast<uint64_t>(Fc) * static_cast<uint64_t>(N)) >> key_bits) ++key_bits;
    for (int sh = 21; sh < 21 + key_bits; sh += 11) {
        uint32_t cnt[2049] = {0};
        for (int q = 0; q < n; ++q) ++cnt[((ka[q] >> sh) & 2047u) + 1];
        for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
        for (int q = 0; q < n; ++q) kb[cnt[(ka[q] >> sh) & 2047u]++] = ka[q];
        ka.swap(kb);
    }
    fo.order.resize(n);
    for (int q = 0; q < n; ++q) fo.order[q] = static_cast<int>(ka[q] & ((1u << 21) - 1));
    return fo;
}

// Every distinct (feature, cell) the engine has met, and the replay of the reference's candidate container (std::unordered_map<std::string,
// ...> keyed by cell + "_" + feature, split_candidate_generator.cpp:117-130) over them: its ITERATION order is the candidate order (Q8).  The
// order of a libstdc++ hash table is a function of the keys' hash values and of the insertion sequence only, so the replay inserts the keys'
// std::hash values -- computed once per remembered cell -- instead of building and hashing 130-byte strings every step.
class CatMemory {
   public:
    // cand_item: the list index of every candidate, in candidate order; item_of_q: list index -> remembered item
    struct Replay { std::vector<int> cand_item, item_of_q; };

    const CatItem &item(int id) const { return items_[id]; }
    size_t size() const { return items_.size(); }
    size_t pending() const { return pending_.size(); }

    // The remembered item of (feature, cell), met now for the first time or before; h = cat_cell_hash_raw of the cell.  defer: the bytes
    // are costly to read now (device-written pinned memory) -- exactly one remembered cell with this (feature, hash): take it and compare the
    // bytes later (verify_pending); several (two different cells that share a 64-bit hash have been met): compare now.
    int item_of(int feat, uint64_t h, const char *cell, bool defer) {
        if (2 * (items_.size() + 1) > tab_key_.size()) reserve(items_.size() + 1);   // (never inside replay(), which reserves for its whole list)
        const uint64_t key = h * 0x9E3779B97F4A7C15ull + static_cast<uint64_t>(feat);
        const size_t slot = tab_slot(key);
        const int head = tab_id_[slot];
        if (defer) {
            int hit = -1, hits = 0;
            for (int id = head; id >= 0; id = items_[id].next)
                if (items_[id].feat == feat && items_[id].lhash == h) { hit = id; ++hits; }
            if (hits == 1) { pending_.emplace_back(hit, cell); return hit; }
        }
        for (int id = head; id >= 0; id = items_[id].next) {
            const CatItem &ci = items_[id];
            if (ci.feat == feat && std::memcmp(ci.name, cell, kCell) == 0) return id;
        }
        CatItem ci;
        ci.feat = feat;
        ci.lhash = h;
        std::memcpy(ci.name, cell, kCell);
        ci.std_hash = std::hash<std::string>{}(cat_key(cell, feat));
        ci.next = head;
        const int id = static_cast<int>(items_.size());
        items_.push_back(ci);
        tab_key_[slot] = key;
        tab_id_[slot] = id;
        return id;
    }

    // Inserts the cells order[0], order[1], ... of a published list (lfeat / lhash / names, n entries) into the container and reads its
    // iteration order back (hash_order_replay.h).  A key met twice in one replay (the lists of several ranks) is inserted once, as
    // emplace() does.  items_done (measurement): the time between the two halves.
    Replay replay(const std::vector<int> &order, const int32_t *lfeat, const uint64_t *lhash, const char *names, int n, bool defer,
                  std::chrono::steady_clock::time_point *items_done = nullptr) {
        if (items_.size() > (1u << 18)) forget();
        reserve(items_.size() + static_cast<size_t>(n));
        pending_.clear();
        Replay r;
        r.item_of_q.assign(static_cast<size_t>(std::max(1, n)), -1);
        r.cand_item.reserve(n);
        std::vector<size_t> hcode;
        std::vector<int> node_q;
        hcode.reserve(n); node_q.reserve(n);
        if (++seen_tag_ == 0) { std::fill(seen_.begin(), seen_.end(), 0u); seen_tag_ = 1; }
        for (int q : order) {
            const int id = item_of(lfeat[q], lhash[q], names + static_cast<size_t>(q) * kCell, defer);
            r.item_of_q[q] = id;
            if (static_cast<size_t>(id) >= seen_.size()) seen_.resize(std::max<size_t>(2 * seen_.size(), static_cast<size_t>(id) + 1), 0);
            if (seen_[id] == seen_tag_) continue;      // key already in the container: emplace() finds it, inserts nothing
            seen_[id] = seen_tag_;
            hcode.push_back(items_[id].std_hash);
            node_q.push_back(q);
        }
        if (items_done) *items_done = std::chrono::steady_clock::now();
        for (int k : libstdcxx_unique_insert_order(hcode)) r.cand_item.push_back(node_q[k]);   // the container's iteration order (Q8)
        return r;
    }

    // The deferred comparisons of the last replay, made while the published bytes are still where they were: true = a remembered cell's
    // bytes differ from the published ones, i.e. two categories of one feature share a 64-bit hash.  test_clash: pretend one differs.
    bool verify_pending(bool test_clash) {
        bool clash = false;
        for (const auto &pq : pending_) clash = clash || std::memcmp(items_[pq.first].name, pq.second, kCell) != 0;
        if (!pending_.empty() && test_clash) clash = true;
        pending_.clear();
        return clash;
    }

    // Forget every remembered cell (a clash, or 2^18 of them).  The per-replay tags go with them: a tag only matters within its own replay.
    void forget() {
        items_.clear(); tab_key_.clear(); tab_id_.clear(); pending_.clear();
        std::fill(seen_.begin(), seen_.end(), 0u);
    }

   private:
    // (raw hash, feature) -> head of the chain through CatItem::next: open addressing, linear probing, at most half full
    // (std::unordered_map cost 2 000 node lookups = 40 us per 4096-row step with 64 categorical columns)
    size_t tab_slot(uint64_t key) const {
        const size_t mask = tab_key_.size() - 1;
        size_t i = static_cast<size_t>(key ^ (key >> 29)) & mask;
        while (tab_id_[i] >= 0 && tab_key_[i] != key) i = (i + 1) & mask;
        return i;
    }
    void reserve(size_t n_items) {
        if (!tab_key_.empty() && 2 * n_items <= tab_key_.size()) return;
        size_t cap = 4096;
        while (cap < 4 * n_items) cap <<= 1;
        std::vector<uint64_t> ok; std::vector<int32_t> oi;
        ok.swap(tab_key_); oi.swap(tab_id_);
        tab_key_.assign(cap, 0); tab_id_.assign(cap, -1);
        for (size_t i = 0; i < ok.size(); ++i)
            if (oi[i] >= 0) { const size_t j = tab_slot(ok[i]); tab_key_[j] = ok[i]; tab_id_[j] = oi[i]; }
    }

    std::vector<CatItem> items_;                              // every distinct (feature, cell) met so far
    std::vector<uint64_t> tab_key_;                           // open-addressed table (keys | item ids, -1 = empty)
    std::vector<int32_t> tab_id_;
    std::vector<uint32_t> seen_;                              // per item: tag of the last replay that inserted it
    uint32_t seen_tag_ = 0;
    std::vector<std::pair<int, const char *>> pending_;       // (item, published cell) pairs whose bytes are still to be compared
};

// The replay leans on libstdc++ internals: the string-keyed container itself, filled in the same order, must iterate as cand_item does.
inline bool replay_matches_container(const std::vector<int> &order, const int32_t *lfeat, const char *names, const std::vector<int> &cand_item) {
    std::unordered_map<std::string, int> ref_map;
    for (int q : order) ref_map.emplace(cat_key(names + static_cast<size_t>(q) * kCell, lfeat[q]), q);
    if (ref_map.size() != cand_item.size()) return false;
    size_t k = 0;
    for (const auto &kv : ref_map)
        if (cand_item[k++] != kv.second) return false;
    return true;
}

}  // namespace detail
}  // namespace gbrl
