// Host-only check of gbrl_amd/csrc/mirror_records.h (compiled with the address and undefined-behaviour sanitizers and run by
// tests/test_host.py): the records the predict kernels read, built from random Models, against the model's own rules restated here --
// the per-leaf conditions of a greedy tree, the [worker][leaf][DMAX/4] layout of the value records, the row side of the packed-code book --
// and records built incrementally, with the upload marks the engine keeps, against records built in one go.
#include "mirror_records.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

using namespace gbrl;
using namespace gbrl::detail;

static const char *g_section = "";
static uint64_t g_seed = 0;
[[noreturn]] static void fail(const char *what, long tree, long index) {
    std::printf("%s: MISMATCH model seed %llu, tree %ld, index %ld: %s\n", g_section, static_cast<unsigned long long>(g_seed), tree, index, what);
    std::exit(1);
}
#define CHECK(cond, what, tree, index) do { if (!(cond)) fail(what, static_cast<long>(tree), static_cast<long>(index)); } while (0)

using Rng = std::mt19937_64;
static size_t pick(Rng &rng, size_t n) { return static_cast<size_t>(rng() % n); }
static const float kInf = std::numeric_limits<float>::infinity();
static const float kPool[] = {-1.5f, -0.0f, 0.0f, 0.25f, 1.0f, 2.5f, 7.0f};   // thresholds and row values meet here
static const int kNames = 6, kRowNames = 8;                                      // categories the conditions / the rows draw from

// the shapes kern::obl2_levels / kern::obl2_padded_outputs give the engine
static size_t levels_of(int md) { return md <= 4 ? 4 : md <= 6 ? 6 : 8; }
static size_t padded_outputs(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }

// ------------------------------------------------------------------------------------------------------- random models
struct Spec { bool greedy; int MD, D, n_num, n_cat; bool specials; };   // specials: +inf and NaN thresholds
struct Cond { bool num; int f; float v; int name; };

static Model new_model(const Spec &s) {
    Model m;
    m.meta.max_depth = s.MD; m.meta.output_dim = s.D; m.meta.n_num_features = s.n_num; m.meta.n_cat_features = s.n_cat;
    m.meta.input_dim = s.n_num + s.n_cat;
    m.meta.grow_policy = s.greedy ? GBRL_HIP_GROW_GREEDY : GBRL_HIP_GROW_OBLIVIOUS;
    m.bias.assign(s.D, 0.0f);
    return m;
}

static Cond random_cond(Rng &rng, const Spec &s) {
    Cond c{true, 0, 0.0f, 0};
    c.num = s.n_cat == 0 || (s.n_num > 0 && pick(rng, 5) < 3);
    if (c.num) {
        c.f = static_cast<int>(pick(rng, s.n_num));
        const size_t k = pick(rng, 10);
        c.v = k < 7 ? kPool[k] : (s.specials && k == 7) ? kInf : (s.specials && k == 8) ? std::nanf("") : static_cast<float>(static_cast<int>(pick(rng, 2000)) - 1000) / 64.0f;
    } else {
        c.f = static_cast<int>(pick(rng, s.n_cat));
        c.name = static_cast<int>(pick(rng, kNames));
    }
    return c;
}

static void cell_of(int name, char *cell) {
    std::memset(cell, 0, kCat);
    std::snprintf(cell, kCat, "category-%d", name);
}

static void add_split_row(Model &m) {
    const size_t MD = m.meta.max_depth, S = m.depths.size() + 1;
    m.depths.push_back(0);
    m.feature_indices.resize(S * MD, 0);
    m.feature_values.resize(S * MD, 0.0f);
    m.is_numerics.resize(S * MD, 1);
    m.categorical_values.resize(S * MD * kCat, 0);
}
static void put_cond(Model &m, size_t c, const Cond &k) {
    m.feature_indices[c] = k.f;
    m.feature_values[c] = k.num ? k.v : 0.0f;
    m.is_numerics[c] = k.num ? 1 : 0;
    if (!k.num) cell_of(k.name, &m.categorical_values[c * kCat]);
}
static size_t add_leaf(Model &m, Rng &rng) {
    const size_t MD = m.meta.max_depth, D = m.meta.output_dim, l = static_cast<size_t>(m.meta.n_leaves++);
    for (size_t j = 0; j < D; ++j) m.values.push_back(static_cast<float>(static_cast<int>(pick(rng, 4001)) - 2000) / 128.0f + 0.001f * static_cast<float>(l + 1));
    m.inequality_directions.resize((l + 1) * MD, 0);
    return l;
}

static void add_oblivious_tree(Model &m, Rng &rng, const Spec &s, int depth) {
    const size_t MD = s.MD, t = static_cast<size_t>(m.meta.n_trees++);
    m.tree_indices.push_back(m.meta.n_leaves);
    add_split_row(m);
    m.depths[t] = depth;
    for (int d = 0; d < depth; ++d) put_cond(m, t * MD + d, random_cond(rng, s));
    for (size_t leaf = 0; leaf < (size_t(1) << depth); ++leaf) {
        const size_t l = add_leaf(m, rng);
        for (int d = 0; d < depth; ++d) m.inequality_directions[l * MD + d] = (leaf >> (depth - 1 - d)) & 1;
    }
    ++m.version;
}

// a random proper binary shape, its leaves written out depth-first and left first; every leaf carries the conditions of its path
static void grow_greedy(Model &m, Rng &rng, const Spec &s, std::vector<Cond> &path, std::vector<uint8_t> &dirs, int min_depth) {
    const int d = static_cast<int>(path.size());
    if (d == s.MD || (d >= min_depth && pick(rng, 3) == 0)) {
        add_split_row(m);
        const size_t l = add_leaf(m, rng), MD = s.MD;
        m.depths[l] = d;
        for (int k = 0; k < d; ++k) { put_cond(m, l * MD + k, path[k]); m.inequality_directions[l * MD + k] = dirs[k]; }
        return;
    }
    path.push_back(random_cond(rng, s));
    for (uint8_t dir = 0; dir < 2; ++dir) {
        dirs.push_back(dir);
        grow_greedy(m, rng, s, path, dirs, dir == 0 ? min_depth : 1);   // (min_depth > 1 forces at least three leaves, along the left spine)
        dirs.pop_back();
    }
    path.pop_back();
}
static void add_greedy_tree(Model &m, Rng &rng, const Spec &s, int min_depth) {
    ++m.meta.n_trees;
    m.tree_indices.push_back(m.meta.n_leaves);
    std::vector<Cond> path;
    std::vector<uint8_t> dirs;
    grow_greedy(m, rng, s, path, dirs, min_depth);
    ++m.version;
}

static void add_tree(Model &m, Rng &rng, const Spec &s) {
    if (s.greedy) add_greedy_tree(m, rng, s, 1);
    else add_oblivious_tree(m, rng, s, pick(rng, 4) == 0 ? static_cast<int>(pick(rng, 2)) : static_cast<int>(pick(rng, s.MD + 1)));
}

static const int kDepths[] = {1, 3, 4, 5, 6, 8}, kDims[] = {1, 3, 4, 5, 8, 17};
static Spec random_spec(Rng &rng, bool greedy, bool specials) {
    Spec s{greedy, kDepths[pick(rng, 6)], kDims[pick(rng, 6)], 1 + static_cast<int>(pick(rng, 5)), static_cast<int>(pick(rng, 4)), specials};
    if (greedy && s.MD == 8 && pick(rng, 2)) s.MD = 6;   // (deep random shapes are large: keep most of them smaller)
    return s;
}
static Model random_model(uint64_t seed, const Spec &s, int trees) {
    Rng rng(seed);
    Model m = new_model(s);
    for (int t = 0; t < trees; ++t) add_tree(m, rng, s);
    return m;
}

// ----------------------------------------------------------------------------------------------------------- random rows
struct Row { std::vector<float> x; std::vector<int> name; };   // a numeric value and a category per column
static Row random_row(Rng &rng, const Spec &s) {
    Row r;
    for (int f = 0; f < s.n_num; ++f) {
        const size_t k = pick(rng, 12);
        r.x.push_back(k < 7 ? kPool[k] : k == 7 ? kInf : k == 8 ? -kInf : static_cast<float>(static_cast<int>(pick(rng, 2000)) - 1000) / 64.0f);
    }
    for (int f = 0; f < s.n_cat; ++f) r.name.push_back(static_cast<int>(pick(rng, kRowNames)));   // (names 6 and 7: no condition mentions them)
    return r;
}
// the model's own condition c on a row
static bool holds(const Model &m, size_t c, const Row &r) {
    if (m.is_numerics[c]) return r.x[m.feature_indices[c]] > m.feature_values[c];
    char cell[kCat];
    cell_of(r.name[m.feature_indices[c]], cell);
    return std::memcmp(cell, &m.categorical_values[c * kCat], kCat) == 0;
}
// what the device sees of the categorical columns: dictionary ids, 0 for a category no condition mentions
static std::vector<int32_t> row_ids(const CatDict &dict, const Row &r) {
    std::vector<int32_t> ids(r.name.size(), 0);
    for (size_t f = 0; f < r.name.size(); ++f) {
        char cell[kCat];
        cell_of(r.name[f], cell);
        for (size_t z = 0; z < dict.size(); ++z)
            if (dict[z].first == static_cast<int>(f) && dict[z].second == std::string(cell, kCat)) ids[f] = static_cast<int32_t>(z) + 1;
    }
    return ids;
}

static bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }
template <typename T>
static long first_difference(const std::vector<T> &a, const std::vector<T> &b) {
    if (a.size() != b.size()) return static_cast<long>(std::min(a.size(), b.size()));
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) return static_cast<long>(i);
    return -1;
}

// ===================================================================================================== greedy descent
static void check_greedy_descent() {
    g_section = "greedy descent";
    long walks = 0;
    for (uint64_t seed = 1; seed <= 60; ++seed) {
        g_seed = seed;
        Rng rng(seed * 7919);
        const Spec s = random_spec(rng, true, true);
        const int T = 1 + static_cast<int>(pick(rng, 40));
        const Model m = random_model(seed, s, T);
        CatDict dict;
        std::vector<int32_t> ids;
        extend_cat_ids(m, 0, dict, ids);
        GreedyNodes g;
        g.reset();
        for (int t = 0; t < T; ++t) g.append_tree(m, ids, t);
        CHECK(g.ok, "a proper ensemble was refused", -1, -1);
        CHECK(g.off.size() == static_cast<size_t>(T) + 1 && g.off[0] == 0, "one offset per tree", -1, g.off.size());
        int max_nodes = 0, max_leaves = 1;
        for (int t = 0; t < T; ++t) {
            const int n_leaves = static_cast<int>(m.leaf_count(t));
            CHECK(g.off[t + 1] - g.off[t] == n_leaves - 1, "a binary tree has one node less than leaves", t, g.off[t + 1] - g.off[t]);
            max_nodes = std::max(max_nodes, n_leaves - 1);
            max_leaves = std::max(max_leaves, n_leaves);
        }
        CHECK(g.off[T] * 4 == static_cast<int>(g.nodes.size()), "node array size", -1, g.nodes.size());
        CHECK(g.max_nodes == max_nodes, "max_nodes", -1, g.max_nodes);
        CHECK(g.max_leaves == max_leaves, "max_leaves", -1, g.max_leaves);
        const size_t MD = s.MD;
        for (int i = 0; i < 24; ++i) {
            const Row r = random_row(rng, s);
            const std::vector<int32_t> rid = row_ids(dict, r);
            for (int t = 0; t < T; ++t) {
                const size_t l0 = m.first_leaf(t), nl = m.leaf_count(t);
                long want = -1;
                for (size_t l = 0; l < nl; ++l) {
                    bool all = true;
                    for (int d = 0; d < m.depths[l0 + l] && all; ++d) all = holds(m, (l0 + l) * MD + d, r) == (m.inequality_directions[(l0 + l) * MD + d] != 0);
                    if (all) { CHECK(want < 0, "two leaves take the row", t, l); want = static_cast<long>(l); }
                }
                CHECK(want >= 0, "no leaf takes the row", t, i);
                const int32_t *nodes = &g.nodes[static_cast<size_t>(g.off[t]) * 4];
                int node = 0, hops = 0;
                while (node >= 0) {
                    CHECK(node < g.off[t + 1] - g.off[t] && ++hops <= static_cast<int>(MD), "the descent leaves the tree", t, node);
                    const int32_t *nd = nodes + 4 * node;
                    float thr;
                    std::memcpy(&thr, &nd[1], 4);
                    const bool right = nd[0] >= 0 ? r.x[nd[0]] > thr : rid[~nd[0]] == nd[1];
                    node = right ? nd[3] : nd[2];
                }
                CHECK(~node == want, "the descent ends at another leaf than the leaf-path rule", t, ~node);
                ++walks;
            }
        }
    }
    std::printf("greedy descent: 60 ensembles, %ld walks equal the leaf-path rule\n", walks);
}

// =================================================================================================== malformed shapes
static void swap_leaves(Model &m, size_t a, size_t b) {
    const size_t MD = m.meta.max_depth, D = m.meta.output_dim;
    std::swap(m.depths[a], m.depths[b]);
    for (size_t d = 0; d < MD; ++d) {
        std::swap(m.feature_indices[a * MD + d], m.feature_indices[b * MD + d]);
        std::swap(m.feature_values[a * MD + d], m.feature_values[b * MD + d]);
        std::swap(m.is_numerics[a * MD + d], m.is_numerics[b * MD + d]);
        std::swap(m.inequality_directions[a * MD + d], m.inequality_directions[b * MD + d]);
        std::swap_ranges(&m.categorical_values[(a * MD + d) * kCat], &m.categorical_values[(a * MD + d + 1) * kCat], &m.categorical_values[(b * MD + d) * kCat]);
    }
    std::swap_ranges(&m.values[a * D], &m.values[(a + 1) * D], &m.values[b * D]);
}

static void check_malformed() {
    g_section = "malformed shapes";
    static const char *kinds[] = {"two leaves swapped", "a right leaf in front of a left one", "a leaf's depth disagrees with its path",
                                  "two siblings with different conditions", "a one-leaf tree"};
    for (int kind = 0; kind < 5; ++kind)
        for (uint64_t seed = 1; seed <= 12; ++seed) {
            g_seed = seed * 100 + kind;
            Rng rng(g_seed);
            const Spec s{true, 3 + static_cast<int>(pick(rng, 4)), kDims[pick(rng, 6)], 2, 2, false};
            const int T = 3 + static_cast<int>(pick(rng, 8)), bad = 1 + static_cast<int>(pick(rng, T - 2));   // in the middle
            Model m = new_model(s);
            for (int t = 0; t < T; ++t) {
                if (t == bad && kind == 4) {   // a single leaf of depth 0
                    ++m.meta.n_trees; m.tree_indices.push_back(m.meta.n_leaves);
                    add_split_row(m); add_leaf(m, rng);
                } else {
                    add_greedy_tree(m, rng, s, t == bad ? 2 : 1);
                }
            }
            const size_t MD = s.MD, l0 = m.first_leaf(bad), nl = m.leaf_count(bad);
            size_t sib = l0;   // the first of the deepest leaves: the left one of two sibling leaves
            for (size_t l = l0; l < l0 + nl; ++l) if (m.depths[l] > m.depths[sib]) sib = l;
            const size_t last = kind == 4 ? 0 : static_cast<size_t>(m.depths[sib]) - 1;
            if (kind == 0) swap_leaves(m, l0, l0 + nl - 1);
            if (kind == 1) { m.inequality_directions[sib * MD + last] = 1; m.inequality_directions[(sib + 1) * MD + last] = 0; }
            if (kind == 2) m.depths[l0 + pick(rng, nl)] += pick(rng, 2) ? 1 : -1;
            if (kind == 3) { m.is_numerics[(sib + 1) * MD + last] = 1; m.feature_values[(sib + 1) * MD + last] = m.feature_values[sib * MD + last] + 1.0f; m.feature_indices[(sib + 1) * MD + last] = m.feature_indices[sib * MD + last]; m.is_numerics[sib * MD + last] = 1; }
            CatDict dict;
            std::vector<int32_t> ids;
            extend_cat_ids(m, 0, dict, ids);
            GreedyNodes g;
            g.reset();
            for (int t = 0; t < bad; ++t) g.append_tree(m, ids, t);
            CHECK(g.ok, "the trees in front of the malformed one are proper", bad, -1);
            const GreedyNodes before = g;
            g.append_tree(m, ids, bad);
            CHECK(!g.ok, kinds[kind], bad, -1);
            CHECK(g.nodes.size() == before.nodes.size(), "the node array is not back at the tree's base", bad, g.nodes.size());
            CHECK(first_difference(g.nodes, before.nodes) < 0, "the trees in front were touched", bad, first_difference(g.nodes, before.nodes));
            CHECK(g.off.size() == static_cast<size_t>(bad) + 2 && g.off.back() == before.off.back(), "the refused tree's offset", bad, g.off.size());
            CHECK(same_bytes(g.off.data(), before.off.data(), before.off.size() * 4), "the offsets in front were touched", bad, -1);
            for (int t = bad + 1; t < T; ++t) g.append_tree(m, ids, t);
            CHECK(!g.ok && g.off.size() == static_cast<size_t>(T) + 1, "one offset per tree, refused for the whole ensemble", T, g.off.size());
            for (int t = 0; t < T; ++t) CHECK(g.off[t + 1] - g.off[t] == (t == bad ? 0 : static_cast<int>(m.leaf_count(t)) - 1), "node count of a tree", t, g.off[t + 1] - g.off[t]);
        }
    std::printf("malformed shapes: 5 kinds x 12 ensembles refused, the tree's nodes dropped, the trees in front untouched\n");
}

// ============================================================================================= records, un-swizzled
// record layout restated: [worker w < DMAX / DW][leaf < LS][DW] holds output w * DW + k of the leaf
static void check_values_unswizzled(const Model &m, const RecordShape &sh, int t, size_t n_leaves, const float *rec) {
    const size_t D = m.meta.output_dim, DW = sh.DMAX / 4, LS = size_t(1) << sh.MX, l0 = m.first_leaf(t);
    for (size_t i = 0; i < LS * sh.DMAX; ++i) {
        const size_t w = i / (LS * DW), leaf = i % (LS * DW) / DW, j = w * DW + i % DW;
        const float want = (leaf < n_leaves && j < D) ? m.values[(l0 + leaf) * D + j] : 0.0f;
        CHECK(same_bytes(&rec[i], &want, 4), "value record", t, i);
    }
}
static void check_never(const int32_t *pair, long tree, long index) {
    CHECK(pair[0] == 0 && pair[1] == 0x7f800000, "a padding condition is not (0, +inf)", tree, index);
}

static void check_oblivious_records() {
    g_section = "oblivious records";
    long trees = 0;
    for (uint64_t seed = 1; seed <= 48; ++seed) {
        g_seed = seed;
        Rng rng(seed * 104729);
        const Spec s = random_spec(rng, false, true);
        const int T = 1 + static_cast<int>(pick(rng, 40));
        const Model m = random_model(seed, s, T);
        CatDict dict;
        std::vector<int32_t> ids, pack, cond_ra;
        std::vector<float> sw;
        extend_cat_ids(m, 0, dict, ids);
        extend_cond_pack(m, ids, 0, pack);
        const RecordShape sh{levels_of(s.MD), padded_outputs(s.D), false};
        extend_oblivious_records(m, pack, sh, 0, 0, cond_ra, sw);
        const size_t MX = sh.MX, VT = (size_t(1) << MX) * sh.DMAX, MD = s.MD;
        CHECK(sh.rec() == VT && sh.pad() == 32 * VT + 16384, "shape", -1, sh.pad());
        CHECK(cond_ra.size() == (T + 32) * 2 * MX, "condition records and 32 padding trees", -1, cond_ra.size());
        CHECK(sw.size() == T * VT + 32 * VT + 16384, "value records and their padding", -1, sw.size());
        for (int t = 0; t < T; ++t, ++trees) {
            const size_t depth = m.depths[t];
            const int32_t *cr = &cond_ra[t * 2 * MX];
            for (size_t d = 0; d < MX - depth; ++d) check_never(cr + 2 * d, t, d);
            for (size_t d = 0; d < depth; ++d) {
                const size_t c = t * MD + d;
                const int32_t key = m.is_numerics[c] ? m.feature_indices[c] : ~m.feature_indices[c];
                int32_t arg = ids[c];
                if (m.is_numerics[c]) std::memcpy(&arg, &m.feature_values[c], 4);
                CHECK(!m.is_numerics[c] ? ids[c] >= 1 : true, "a categorical condition without a dictionary id", t, d);
                CHECK(cr[2 * (MX - depth + d)] == key && cr[2 * (MX - depth + d) + 1] == arg, "right-aligned condition", t, d);
                CHECK(pack[2 * c] == key && pack[2 * c + 1] == arg, "packed condition", t, d);
            }
            check_values_unswizzled(m, sh, t, size_t(1) << depth, &sw[t * VT]);
        }
        for (size_t p = T * MX; p < (T + 32) * MX; ++p) check_never(&cond_ra[2 * p], T, p);
        for (size_t i = T * VT; i < sw.size(); ++i) CHECK(sw[i] == 0.0f && !std::signbit(sw[i]), "value padding", T, i);
    }
    std::printf("oblivious records: 48 ensembles, %ld trees un-swizzled, conditions right-aligned, padding in place\n", trees);
}

static void check_greedy_records() {
    g_section = "greedy records";
    long trees = 0, too_large = 0;
    for (uint64_t seed = 1; seed <= 48; ++seed) {
        g_seed = seed;
        Rng rng(seed * 1299709);
        const Spec s = random_spec(rng, true, false);
        const int T = 1 + static_cast<int>(pick(rng, 40));
        const Model m = random_model(seed, s, T);
        CatDict dict;
        std::vector<int32_t> ids;
        extend_cat_ids(m, 0, dict, ids);
        GreedyNodes g;
        g.reset();
        for (int t = 0; t < T; ++t) g.append_tree(m, ids, t);
        // the engine's shape, and one with fewer levels than the trees have: its records hold the first 2^levels leaves and no node of a larger tree
        for (const size_t MX : {levels_of(s.MD), size_t(2)}) {
            const RecordShape sh{MX, padded_outputs(s.D), true};
            const size_t LS = size_t(1) << MX, VT = LS * sh.DMAX, REC = VT + LS * 4;
            std::vector<float> sw;
            extend_greedy_records(m, g, sh, 0, 0, sw);
            CHECK(sh.rec() == REC && sh.pad() == 32 * REC + 16384, "shape", -1, sh.pad());
            CHECK(sw.size() == T * REC + 32 * REC + 16384, "records and their padding", -1, sw.size());
            for (int t = 0; t < T; ++t, ++trees) {
                check_values_unswizzled(m, sh, t, m.leaf_count(t), &sw[t * REC]);
                const size_t n0 = g.off[t], n = g.off[t + 1] - g.off[t];
                const char *np = reinterpret_cast<const char *>(&sw[t * REC + VT]);
                const std::vector<char> zero(LS * 16, 0);
                if (n <= LS) {
                    CHECK(same_bytes(np, &g.nodes[n0 * 4], n * 16), "node part", t, n);
                    CHECK(same_bytes(np + n * 16, zero.data(), (LS - n) * 16), "node part padding", t, n);
                } else {
                    CHECK(same_bytes(np, zero.data(), LS * 16), "the node part of a tree with more nodes than slots", t, n);
                    ++too_large;
                }
            }
            for (size_t i = T * REC; i < sw.size(); ++i) CHECK(sw[i] == 0.0f && !std::signbit(sw[i]), "record padding", T, i);
        }
    }
    CHECK(too_large > 0, "no tree with more nodes than slots was drawn", -1, -1);
    std::printf("greedy records: 48 ensembles x 2 shapes, %ld records (%ld with more nodes than slots) un-swizzled, node parts byte-equal\n", trees, too_large);
}

// ===================================================================================== incremental equals from scratch
// The host arrays, the marks the engine keeps over them, and what a device would hold after the engine's appends: a buffer that never moves and
// whose new elements are garbage until something is copied there (so a slice or a piece of padding that is not sent shows).
constexpr size_t kNoRedo = ~static_cast<size_t>(0);
struct Mirror {
    size_t up_trees = 0, up_leaves = 0, up_splits = 0, redo = kNoRedo, grd_up_nodes = 0, rate_trees = 0, dict_splits = 0;
    CatDict dict;
    std::vector<int32_t> ids, pack, cond_ra;
    std::vector<float> sw;
    GreedyNodes grd;
    RateTable rate;
    std::vector<int32_t> d_pack, d_cond_ra, d_nodes, d_off;
    std::vector<float> d_values, d_sw, d_rate;
    bool sw_built = false;

    template <typename T>
    static void grow(std::vector<T> &dev, size_t n) {
        T junk;
        std::memset(&junk, 0xa5, sizeof(T));
        if (dev.size() < n) dev.resize(n, junk);
        dev.resize(n);
    }
    template <typename T>
    static void append(std::vector<T> &dev, const std::vector<T> &host, size_t old_n, size_t new_n) {
        grow(dev, new_n);
        std::copy(host.begin() + old_n, host.begin() + new_n, dev.begin() + old_n);
    }
    static void append_padded(std::vector<float> &dev, const std::vector<float> &host, size_t old_recs, size_t new_recs, size_t rec, size_t pad) {
        grow(dev, new_recs * rec + pad);
        auto copy = [&](size_t a, size_t b) { std::copy(host.begin() + a, host.begin() + b, dev.begin() + a); };
        if (old_recs == 0 || old_recs > new_recs) copy(old_recs * rec, new_recs * rec + pad);
        else if (new_recs > old_recs) { copy(old_recs * rec, new_recs * rec); copy(old_recs * rec + pad, new_recs * rec + pad); }
    }

    void sync(const Model &m, const Spec &s) {
        const size_t T = m.meta.n_trees, L = m.meta.n_leaves, S = m.split_rows(), MD = s.MD, D = s.D;
        extend_cat_ids(m, dict_splits, dict, ids);
        dict_splits = S;
        extend_cond_pack(m, ids, up_splits, pack);
        append(d_pack, pack, up_splits * MD * 2, S * MD * 2);
        append(d_values, m.values, up_leaves * D, L * D);
        const size_t vt0 = std::min(up_trees, redo);
        if (!s.greedy) {
            const RecordShape sh{levels_of(s.MD), padded_outputs(s.D), false};
            extend_oblivious_records(m, pack, sh, up_trees, vt0, cond_ra, sw);
            append(d_cond_ra, cond_ra, up_trees * 2 * sh.MX, (T + kPadTrees) * 2 * sh.MX);
            append_padded(d_sw, sw, vt0, T, sh.rec(), sh.pad());
            sw_built = true;
        } else {
            if (up_trees == 0) grd.reset();
            for (size_t t = up_trees; t < T; ++t) grd.append_tree(m, ids, t);
            append(d_nodes, grd.nodes, grd_up_nodes * 4, grd.nodes.size());
            append(d_off, grd.off, 0, grd.off.size());
            if (grd.ok) {
                const RecordShape sh{levels_of(s.MD), padded_outputs(s.D), true};
                extend_greedy_records(m, grd, sh, up_trees, vt0, sw);
                append_padded(d_sw, sw, vt0, T, sh.rec(), sh.pad());
                sw_built = true;
            }
        }
        const size_t from = rate.extend(m, rate_trees), NO = m.opts.size();
        append(d_rate, rate.rate, from * NO, T * NO);
        up_trees = T; up_leaves = L; up_splits = S; redo = kNoRedo; grd_up_nodes = grd.nodes.size() / 4; rate_trees = T;
    }
    void rewind_values(const Model &m, int t) { up_leaves = std::min(up_leaves, m.first_leaf(t)); redo = std::min(redo, static_cast<size_t>(t)); }
    void invalidate() { up_trees = up_leaves = up_splits = 0; redo = kNoRedo; grd_up_nodes = 0; rate_trees = 0; }
};

static void compare_with_scratch(const Mirror &inc, const Model &m, const Spec &s, int step) {
    Mirror one;
    one.sync(m, s);
    const size_t T = m.meta.n_trees;
#define SAME(field) CHECK(first_difference(inc.field, one.field) < 0, "incremental and from-scratch differ in " #field, step, first_difference(inc.field, one.field))
    SAME(ids); SAME(pack); SAME(cond_ra); SAME(grd.nodes); SAME(grd.off); SAME(rate.rate);
    SAME(d_pack); SAME(d_cond_ra); SAME(d_nodes); SAME(d_off); SAME(d_values);
    if (inc.sw_built) { SAME(sw); SAME(d_sw); }
#undef SAME
    CHECK(inc.grd.ok == one.grd.ok && inc.grd.max_nodes == one.grd.max_nodes && inc.grd.max_leaves == one.grd.max_leaves, "greedy summary", step, -1);
    CHECK(first_difference(inc.d_values, m.values) < 0, "the device values are not the model's", step, first_difference(inc.d_values, m.values));
    CHECK(first_difference(inc.d_pack, inc.pack) < 0 && first_difference(inc.d_cond_ra, inc.cond_ra) < 0 && first_difference(inc.d_nodes, inc.grd.nodes) < 0,
          "a device array is not its host array", step, -1);
    if (inc.sw_built) CHECK(first_difference(inc.d_sw, inc.sw) < 0, "the device records are not the host records", step, first_difference(inc.d_sw, inc.sw));
    CHECK(same_bytes(inc.d_rate.data(), inc.rate.rate.data(), T * m.opts.size() * 4), "the device rate table", step, -1);
}

static void check_incremental() {
    g_section = "incremental equals from scratch";
    long syncs = 0;
    for (uint64_t seed = 1; seed <= 40; ++seed) {
        g_seed = seed;
        Rng rng(seed * 15485863);
        const Spec s = random_spec(rng, seed % 2 == 0, true);
        Model m = new_model(s);
        gbrl_hip_optimizer o{};
        o.scheduler = GBRL_HIP_SCHED_LINEAR; o.init_lr = 0.5f; o.stop_lr = 0.01f; o.stop_idx = s.D; o.T = 50;
        m.opts.push_back(o);
        Mirror inc;
        const int steps = 4 + static_cast<int>(pick(rng, 9));
        const int invalidate_at = seed % 5 == 0 ? static_cast<int>(pick(rng, steps)) : -1;
        for (int step = 0; step < steps && m.meta.n_trees < 40; ++step, ++syncs) {
            for (size_t k = 1 + pick(rng, 3); k > 0 && m.meta.n_trees < 40; --k) add_tree(m, rng, s);
            inc.sync(m, s);
            compare_with_scratch(inc, m, s, step);
            const int mode = step == invalidate_at ? 2 : static_cast<int>(pick(rng, 3));
            if (mode == 0) continue;
            // values change: one tree and rewind_values (a few times: the marks take the minimum), or any trees and invalidate_mirror
            for (size_t k = 1 + pick(rng, 3); k > 0; --k) {
                const int t = static_cast<int>(pick(rng, m.meta.n_trees));
                for (size_t i = m.first_leaf(t) * s.D; i < (m.first_leaf(t) + m.leaf_count(t)) * s.D; ++i) m.values[i] += 1.0f;
                if (mode == 1) inc.rewind_values(m, t);
            }
            if (mode == 2) inc.invalidate();
            ++m.version;
            if (pick(rng, 2)) { inc.sync(m, s); compare_with_scratch(inc, m, s, step); ++syncs; }   // (else the next step's trees join first)
        }
    }
    std::printf("incremental equals from scratch: 40 ensembles, %ld synchronisations, every array and its device image byte-equal\n", syncs);
}

// ========================================================================================================= rate table
static void check_rate_table() {
    g_section = "rate table";
    g_seed = 1;
    const Spec s{false, 3, 4, 2, 0, false};
    Rng rng(99);
    Model m = new_model(s);
    gbrl_hip_optimizer a{}, b{}, c{};
    a.scheduler = GBRL_HIP_SCHED_LINEAR; a.init_lr = 0.3f; a.stop_lr = 0.02f; a.start_idx = 0; a.stop_idx = 1; a.T = 17;
    b.scheduler = GBRL_HIP_SCHED_CONST; b.init_lr = 0.7f; b.start_idx = 1; b.stop_idx = 3;
    c.scheduler = GBRL_HIP_SCHED_LINEAR; c.init_lr = 1.0f; c.stop_lr = 0.5f; c.start_idx = 3; c.stop_idx = 4; c.T = 1000;
    m.opts = {a, b, c};
    auto all_rows = [&](const RateTable &r, size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t)
            for (size_t o = 0; o < 3; ++o) {
                const float want = scheduler_lr(m.opts[o], static_cast<int>(t));
                CHECK(same_bytes(&r.rate[t * 3 + o], &want, 4), "an entry is not scheduler_lr", t, o);
            }
    };
    RateTable r;
    for (int t = 0; t < 25; ++t) add_tree(m, rng, s);
    CHECK(r.extend(m, 0) == 0 && r.rate.size() == 25 * 3, "first build", -1, r.rate.size());
    all_rows(r, 0, 25);
    for (int t = 0; t < 15; ++t) add_tree(m, rng, s);
    std::fill(r.rate.begin(), r.rate.begin() + 25 * 3, -1.0f);   // (marks the rows an append must leave alone)
    CHECK(r.extend(m, 25) == 25 && r.rate.size() == 40 * 3, "append", -1, r.rate.size());
    for (size_t i = 0; i < 25 * 3; ++i) CHECK(r.rate[i] == -1.0f, "appending trees touched an earlier row", i / 3, i % 3);
    all_rows(r, 25, 40);
    m.opts[1].init_lr = 0.6f;
    CHECK(r.extend(m, 40) == 0, "a changed optimizer rebuilds from tree 0", -1, -1);
    all_rows(r, 0, 40);
    m.opts.pop_back();
    CHECK(r.extend(m, 40) == 0 && r.opts.size() == 2, "fewer optimizers rebuild from tree 0", -1, -1);
    m.opts.push_back(c);
    CHECK(r.extend(m, 40) == 0, "more optimizers rebuild from tree 0", -1, -1);
    all_rows(r, 0, 40);
    m.meta.n_trees = 10;   // a shrunken ensemble
    CHECK(r.extend(m, 40) == 0 && r.rate.size() == 10 * 3, "a shrunken ensemble rebuilds from tree 0", -1, r.rate.size());
    all_rows(r, 0, 10);
    m.meta.n_trees = 0;
    CHECK(r.extend(m, 0) == 0 && r.rate.size() == 3, "an empty ensemble keeps one row", -1, r.rate.size());
    std::printf("rate table: every entry is scheduler_lr, appended rows only, rebuilt for other optimizers and a shrunken ensemble\n");
}

// ==================================================================================================== packed-code book
// the row side (k_pack_codes): a numeric field is 0xffff - #{distinct thresholds of the feature below x}, two fields per word (the even feature
// in the low half); a categorical word starts as all ones and loses bit `slot & 31` of word wn + slot / 32 when the cell is that category
static std::vector<uint32_t> pack_row(const Model &m, const PcBook &b, const Spec &s, const Row &r, const std::vector<int32_t> &rid) {
    std::vector<uint32_t> row(b.row_words, 0);
    std::vector<std::set<float>> distinct(s.n_num);
    for (int t = 0; t < m.meta.n_trees; ++t)
        for (int d = 0; d < m.depths[t]; ++d) {
            const size_t c = static_cast<size_t>(t) * s.MD + d;
            const float v = m.feature_values[c];
            if (m.is_numerics[c] && v == v && v != kInf) distinct[m.feature_indices[c]].insert(v == 0.0f ? 0.0f : v);
        }
    for (int f = 0; f < s.n_num; ++f) {
        uint32_t below = 0;
        for (float v : distinct[f]) below += r.x[f] > v;
        CHECK(b.thr_off[f + 1] - b.thr_off[f] == static_cast<int>(distinct[f].size()), "distinct thresholds of a feature", -1, f);
        CHECK(std::equal(distinct[f].begin(), distinct[f].end(), b.thr.begin() + b.thr_off[f]), "sorted thresholds of a feature", -1, f);
        CHECK((size_t(1) << b.iters) > distinct[f].size(), "2^iters does not exceed the thresholds of a feature", -1, f);
        row[f >> 1] |= (0xffffu - below) << ((f & 1) ? 16 : 0);
    }
    if (s.n_num & 1) row[s.n_num >> 1] |= 0xffff0000u;
    for (int w = b.wn; w < b.nw; ++w) row[w] = 0xffffffffu;
    for (int f = 0; f < s.n_cat; ++f) {
        const int slot = b.cat_slot[rid[f]];
        if (slot >= 0) row[b.wn + slot / 32] &= ~(1u << (slot & 31));
    }
    // the kernel visits only the columns word_cols names for a word: they must hold every column with a slot in it
    for (int w = b.wn; w < b.nw; ++w) {
        uint32_t word = 0xffffffffu;
        for (int c = b.word_cols[2 * (w - b.wn)]; c < b.word_cols[2 * (w - b.wn) + 1]; ++c) {
            const int slot = b.cat_slot[rid[c]];
            if (slot >= 0 && slot / 32 == w - b.wn) word &= ~(1u << (slot & 31));
        }
        CHECK(word == row[w], "word_cols leaves out a column of a one-hot word", -1, w);
    }
    return row;
}

static Model threshold_model(int distinct) {   // one feature, 8192 trees of depth 8: 65536 conditions over `distinct` thresholds
    const Spec s{false, 8, 1, 1, 0, false};
    Model m = new_model(s);
    const size_t T = 8192, MD = 8;
    m.meta.n_trees = T; m.meta.n_leaves = 0;
    m.depths.assign(T, 8);
    m.tree_indices.assign(T, 0);
    m.feature_indices.assign(T * MD, 0);
    m.is_numerics.assign(T * MD, 1);
    m.feature_values.resize(T * MD);
    for (size_t c = 0; c < T * MD; ++c) m.feature_values[c] = static_cast<float>(static_cast<int>(c % distinct)) * 0.5f;
    return m;
}

static void check_pc_book() {
    g_section = "packed-code book";
    long conds = 0;
    for (uint64_t seed = 1; seed <= 40; ++seed) {
        g_seed = seed;
        Rng rng(seed * 32452843);
        Spec s = random_spec(rng, false, true);
        s.n_num = static_cast<int>(pick(rng, 7)); s.n_cat = s.n_num == 0 ? 1 + static_cast<int>(pick(rng, 3)) : static_cast<int>(pick(rng, 4));
        if (seed % 8 == 0) s.n_cat = 12;   // (more than 32 slots: two one-hot words)
        const int T = 1 + static_cast<int>(pick(rng, 40));
        const Model m = random_model(seed, s, T);
        CatDict dict;
        std::vector<int32_t> ids;
        extend_cat_ids(m, 0, dict, ids);
        const size_t MX = levels_of(s.MD), MD = s.MD;
        const PcBook b = build_pc_book(m, ids, dict.size(), s.n_num, s.n_cat, MX, 160);
        CHECK(b.ok, "an expressible ensemble was refused", -1, -1);
        int slots = 0;
        for (int32_t sl : b.cat_slot) slots += sl >= 0;
        CHECK(b.wn == (s.n_num + 1) / 2 && b.nw == b.wn + (slots + 31) / 32 && b.row_words == ((b.nw + 3) & ~3), "row shape", -1, b.nw);
        CHECK(b.cond.size() == (T + 32) * MX * 3 && b.cat_slot.size() == dict.size() + 1 && b.cat_slot[0] == -1, "array sizes", -1, b.cond.size());
        CHECK(b.thr.size() == static_cast<size_t>(b.thr_off[s.n_num]) + 1, "threshold table", -1, b.thr.size());
        for (size_t i = T * MX * 3; i < b.cond.size(); ++i) CHECK(b.cond[i] == 0, "padding trees", T, i);
        for (int i = 0; i < 24; ++i) {
            const Row r = random_row(rng, s);
            const std::vector<int32_t> rid = row_ids(dict, r);
            const std::vector<uint32_t> row = pack_row(m, b, s, r, rid);
            for (int t = 0; t < T; ++t) {
                const size_t depth = m.depths[t];
                for (size_t d = 0; d < MX; ++d, ++conds) {
                    const int32_t *rec = &b.cond[(t * MX + d) * 3];
                    CHECK(rec[0] >= 0 && rec[0] < b.row_words && rec[1] >= 0 && rec[1] < 32, "a record points outside the row", t, d);
                    const bool pass = (row[rec[0]] << rec[1]) < static_cast<uint32_t>(rec[2]);
                    if (d < MX - depth) { CHECK(rec[0] == 0 && rec[1] == 0 && rec[2] == 0 && !pass, "the padding in front of a shallow tree", t, d); continue; }
                    const size_t c = t * MD + (d - (MX - depth));
                    CHECK(pass == holds(m, c, r), "the book's test disagrees with the condition", t, d);
                    const float v = m.feature_values[c];
                    if (m.is_numerics[c] && (v != v || v == kInf)) CHECK(rec[0] == 0 && rec[1] == 0 && rec[2] == 0, "a +inf / NaN threshold is not (0, 0, 0)", t, d);
                }
            }
        }
    }
    // every refusal
    g_seed = 0;
    Rng rng(5);
    const Spec s{false, 4, 3, 3, 2, false};
    Model m = new_model(s);
    add_oblivious_tree(m, rng, s, 2);
    put_cond(m, 0, Cond{true, 2, 1.0f, 0});
    put_cond(m, 1, Cond{false, 1, 0.0f, 3});
    add_oblivious_tree(m, rng, s, 0);
    CatDict dict;
    std::vector<int32_t> ids;
    extend_cat_ids(m, 0, dict, ids);
    CHECK(build_pc_book(m, ids, dict.size(), 3, 2, 4, 160).ok, "the plain case", -1, -1);
    CHECK(!build_pc_book(m, ids, dict.size(), 2, 2, 4, 160).ok, "a numeric feature out of range", -1, -1);
    CHECK(!build_pc_book(m, ids, dict.size(), 3, 1, 4, 160).ok, "a categorical feature out of range", -1, -1);
    { Model neg = m; neg.feature_indices[0] = -1; CHECK(!build_pc_book(neg, ids, dict.size(), 3, 2, 4, 160).ok, "a negative feature", -1, -1); }
    { std::vector<int32_t> z = ids; z[1] = 0; CHECK(!build_pc_book(m, z, dict.size(), 3, 2, 4, 160).ok, "a category id of 0", -1, -1); }
    CHECK(!build_pc_book(m, ids, dict.size() - 1, 3, 2, 4, 160).ok, "an id beyond the dictionary", -1, -1);
    CHECK(!build_pc_book(m, ids, dict.size(), 3, 2, 1, 160).ok, "a depth above the levels", -1, -1);
    CHECK(build_pc_book(m, ids, dict.size(), 3, 2, 4, 4).ok && !build_pc_book(m, ids, dict.size(), 3, 2, 4, 3).ok, "row_words above the bank", -1, -1);
    CHECK(!build_pc_book(m, ids, dict.size(), 3, 2, 0, 160).ok, "no levels", -1, -1);
    { Model none = new_model(s); CHECK(!build_pc_book(none, {}, 0, 3, 2, 4, 160).ok, "no trees", -1, -1); }
    { const Spec e{false, 4, 3, 0, 0, false}; Model flat = new_model(e); add_oblivious_tree(flat, rng, e, 0);
      CHECK(!build_pc_book(flat, std::vector<int32_t>(4, 0), 0, 0, 0, 4, 160).ok, "row_words of 0", -1, -1); }
    { const Model many = threshold_model(65535), most = threshold_model(65534);
      const std::vector<int32_t> none(8192 * 8, 0);
      CHECK(!build_pc_book(many, none, 0, 1, 0, 8, 160).ok, "more than 65534 thresholds", -1, -1);
      const PcBook b = build_pc_book(most, none, 0, 1, 0, 8, 160);
      CHECK(b.ok && b.iters == 16 && b.thr_off[1] == 65534, "65534 thresholds are expressible", -1, b.iters); }
    std::printf("packed-code book: 40 ensembles, %ld book tests equal the conditions, every refusal\n", conds);
}

int main() {
    check_greedy_descent();
    check_malformed();
    check_oblivious_records();
    check_greedy_records();
    check_incremental();
    check_rate_table();
    check_pc_book();
    std::printf("mirror records: all sections passed\n");
    return 0;
}
