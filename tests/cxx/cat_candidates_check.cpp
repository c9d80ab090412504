// Host-only check of gbrl_amd/csrc/cat_candidates_host.h (compiled and run by tests/test_host.py): the candidates and class codes built
// from the list of distinct cells a device scan would publish -- first_occurrence_order, CatMemory::replay, keep_top_by_mean,
// assign_classes -- against categorical_candidates (the reference's rule on every cell) on the same random batches.
#include "cat_candidates_host.h"
#include "cat_hash.h"
#include <cstdio>
#include <random>
using namespace gbrl;
using namespace gbrl::detail;

struct Batch { int N, Fc, D, B; std::vector<char> cells; std::vector<float> grads; };

// what the scan publishes: one record per distinct (feature, raw 128 bytes), in no particular order
struct Published {
    std::vector<int32_t> feat, first, count;
    std::vector<uint64_t> hash;
    std::vector<float> total;
    std::vector<char> names;
    std::vector<int> q_of_cell;   // [N][Fc] -> record
};

static Published publish(const Batch &b, std::mt19937_64 &rng) {
    Published p;
    const std::vector<float> norms = squared_norms(b.grads.data(), b.N, b.D);
    std::unordered_map<std::string, int> id;
    p.q_of_cell.resize(static_cast<size_t>(b.N) * b.Fc);
    for (int f = 0; f < b.Fc; ++f)
        for (int i = 0; i < b.N; ++i) {
            const char *cell = &b.cells[(static_cast<size_t>(i) * b.Fc + f) * kCell];
            auto it = id.emplace(cat_key(cell, f), static_cast<int>(p.feat.size()));
            if (it.second) {
                uint64_t w[16];
                std::memcpy(w, cell, kCell);
                p.feat.push_back(f); p.first.push_back(i); p.count.push_back(0); p.total.push_back(0.0f); p.hash.push_back(cat_cell_hash_raw(w));
            }
            const int q = it.first->second;
            p.count[q] += 1;
            p.total[q] += norms[i];   // float32, row order
            p.q_of_cell[static_cast<size_t>(i) * b.Fc + f] = q;
        }
    // the device appends records in the order its atomics land: shuffle
    const int n = static_cast<int>(p.feat.size());
    std::vector<int> perm(n), inv(n);
    for (int q = 0; q < n; ++q) perm[q] = q;
    std::shuffle(perm.begin(), perm.end(), rng);
    Published s = p;
    s.names.resize(static_cast<size_t>(n) * kCell);
    for (int q = 0; q < n; ++q) {
        const int o = perm[q];
        inv[o] = q;
        s.feat[q] = p.feat[o]; s.first[q] = p.first[o]; s.count[q] = p.count[o]; s.total[q] = p.total[o]; s.hash[q] = p.hash[o];
        std::memcpy(&s.names[static_cast<size_t>(q) * kCell], &b.cells[(static_cast<size_t>(p.first[o]) * b.Fc + p.feat[o]) * kCell], kCell);
    }
    for (int &q : s.q_of_cell) q = inv[q];
    return s;
}

static Batch make_batch(int rep, std::mt19937_64 &rng) {
    Batch b;
    b.N = rep < 8 ? rep + 1 : 1 + static_cast<int>(rng() % 3000);
    b.Fc = 1 + static_cast<int>(rng() % 8);
    b.D = 1 + static_cast<int>(rng() % 4);
    const int bins[5] = {1, 4, 32, 256, 4096};
    b.B = bins[rng() % 5];
    b.cells.assign(static_cast<size_t>(b.N) * b.Fc * kCell, 0);
    b.grads.resize(static_cast<size_t>(b.N) * b.D);
    const bool coarse = rep % 3 == 0;   // few distinct gradient values: equal means, the order among ties counts
    for (float &g : b.grads) g = coarse ? 0.5f * static_cast<float>(static_cast<int>(rng() % 3) - 1) : static_cast<float>(static_cast<double>(rng() % 20001) / 10000.0 - 1.0);
    for (int f = 0; f < b.Fc; ++f) {
        const int mode = static_cast<int>(rng() % 4);   // cardinality: 1, a few dozen, ~N/2, every row its own cell
        const int card = mode == 0 ? 1 : mode == 1 ? 1 + static_cast<int>(rng() % 40) : mode == 2 ? 1 + b.N / 2 : 0;
        for (int i = 0; i < b.N; ++i) {
            char *cell = &b.cells[(static_cast<size_t>(i) * b.Fc + f) * kCell];
            const long long v = card ? static_cast<long long>(rng() % card) : i;
            std::snprintf(cell, kCell, "c%lld", v + 1000ll * (rep % 5));   // (shared with other batches and features: remembered cells)
            if (rng() % 4 == 0) cell[100 + rng() % 28] = static_cast<char>('a' + rng() % 3);   // differs only behind the first NUL
        }
    }
    return b;
}

int main() {
    std::mt19937_64 rng(11);
    CatMemory mem;
    int bad = 0, batches = 0, overflowed = 0, remembered = 0;
    for (int rep = 0; rep < 160; ++rep) {
        const Batch b = make_batch(rep, rng);
        std::vector<CatCandidate> want_c, got_c;
        std::vector<uint16_t> want_codes;
        std::vector<int> want_cls(b.Fc, 0), got_cls(b.Fc, 0);
        categorical_candidates(b.cells.data(), b.grads.data(), b.N, b.Fc, b.D, b.B, want_c, want_codes, want_cls);

        const Published p = publish(b, rng);
        const int n = static_cast<int>(p.feat.size());
        const size_t keep = static_cast<size_t>(b.Fc) * b.B;
        const FirstOccurrence fo = first_occurrence_order(p.feat.data(), p.first.data(), n, b.N, b.Fc);
        int mx = 1;
        for (int f = 0; f < b.Fc; ++f) mx = std::max(mx, static_cast<int>(std::count(p.feat.begin(), p.feat.end(), f)));
        bad += fo.max_per_feature != mx;
        const bool defer = rep % 2 == 0;
        const size_t before = mem.size();
        CatMemory::Replay r = mem.replay(fo.order, p.feat.data(), p.hash.data(), p.names.data(), n, defer);
        remembered += mem.size() < before + static_cast<size_t>(n);
        bad += !replay_matches_container(fo.order, p.feat.data(), p.names.data(), r.cand_item);
        bad += !defer && mem.pending() != 0;
        bad += mem.verify_pending(false);   // no two of these cells share a hash
        if (r.cand_item.size() > keep) {
            ++overflowed;
            std::vector<std::pair<int, float>> vec;
            for (int q : r.cand_item) vec.emplace_back(q, p.total[q] / static_cast<float>(p.count[q]));
            keep_top_by_mean(vec, keep);
            r.cand_item.resize(keep);
            for (size_t k = 0; k < keep; ++k) r.cand_item[k] = vec[k].first;
        }
        std::vector<int> cls_of_q(std::max(1, n), 0);
        assign_classes(r.cand_item.size(), [&](size_t k) { const int q = r.cand_item[k]; return std::make_pair(static_cast<int>(p.feat[q]), static_cast<const char *>(mem.item(r.item_of_q[q]).name)); },
                       got_c, got_cls, [&](size_t k, int cls) { cls_of_q[r.cand_item[k]] = cls; });
        bool same = got_c.size() == want_c.size() && got_cls == want_cls;
        for (size_t k = 0; same && k < got_c.size(); ++k) same = got_c[k].feat == want_c[k].feat && got_c[k].cls == want_c[k].cls && got_c[k].name == want_c[k].name;
        for (size_t c = 0; same && c < want_codes.size(); ++c) same = want_codes[c] == cls_of_q[p.q_of_cell[c]];
        bad += !same;
        ++batches;
        if (rep % 37 == 36) mem.forget();   // and the batches behind it meet an empty memory
    }
    // two different cells of one feature under one (chosen) hash: the second is taken for the first, and verify_pending reports it
    {
        char a[kCell] = "left", c[kCell] = "right";
        const uint64_t h = 0x1234567890abcdefull;
        const int ia = mem.item_of(3, h, a, true);
        bad += mem.pending() != 0;                       // new: nothing deferred
        const int ic = mem.item_of(3, h, c, true);
        bad += ic != ia || mem.pending() != 1;
        bad += !mem.verify_pending(false);
        bad += mem.pending() != 0 || mem.verify_pending(true);   // nothing pending: the test hook alone reports nothing
        const int ic2 = mem.item_of(3, h, c, false);     // compared at once: a second item under the same (feature, hash)
        bad += ic2 == ia;
        bad += mem.item_of(3, h, c, true) != ic2 || mem.pending() != 0;   // two remembered cells share the hash: compared now
        (void)mem.item_of(3, h, a, false);
        const int again = mem.item_of(4, h, a, true);    // another feature: a new item
        bad += again == ia || mem.pending() != 0;
        (void)mem.item_of(4, h, a, true);
        bad += mem.pending() != 1 || !mem.verify_pending(true) || mem.pending() != 0;   // the hook with a (matching) pending pair
        mem.forget();
        bad += mem.size() != 0;
    }
    std::printf("%d batches (%d with more distinct cells than candidates, %d with remembered cells), %d mismatches\n", batches, overflowed, remembered, bad);
    return bad || !overflowed || !remembered ? 1 : 0;
}
