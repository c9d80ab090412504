// shapx_core.h -- exact SHAP interaction values of the ensemble, the rule written once for host and device (engine_shapx.hip calls it,
// shap_interactions.hip has the kernels, explain.cpp the host evaluation; the host half needs no device and no HIP header).
//
// The rule (path-wise, leaf by leaf).  The value explained is ensemble_shap's: raw leaf values, no learning rate, sign or bias.  The background is
// the model's own cover: "feature absent" at a node follows both children, weighted by the stored edge weights.  For a leaf l of tree t:
//   U_l      the conditions of its root-to-leaf path merged by feature, in the order of first appearance; n = |U_l| (<= kShapxMaxN)
//   z_e      the float64 product, in depth order, of the path's edge weights at e's conditions
//   o_e      1 when the row satisfies ALL of e's conditions on the path, else 0 (bit e of the PATTERN o; on a data set: code > bin against the direction)
//   c_k(P)   = sum over S in U_l \ P, |S| = k, of prod_{e in S} o_e * prod_{e in U_l \ P \ S} z_e.  Because o_e is 0 or 1 this is
//              Z0(P) * q_k(P): Z0 the product of z_e over the COLD (o_e = 0) features outside P, q(P) the coefficients of prod (z_e + x) over the HOT
//              ones outside P.  q is extended once (O(n^2)) and a hot feature is removed by the top-down unwind q'[k-1] = q[k] - z * q'[k], which
//              never divides: O(n) per removed feature, O(n^3) per leaf and pattern (shapx_leaf_weights; every operation and its order is there).
//   W(k, n)  = k! (n - k - 1)! / n!  (shapx_w_table: W(0, n) = 1 / n, W(k, n) = W(k - 1, n) * k / (n - k); built on the host, read by both sides)
//   a_i      = ((o_i - z_i) * Z0({i})) * sum_k W(k, n) q_k({i})                                  the leaf's SHAP weight of feature i
//   w_ij     = ((0.5 * ((o_i - z_i) * (o_j - z_j))) * Z0({i, j})) * sum_k W(k, n - 1) q_k({i, j})   i < j, used for both halves
// The tree's matrix T^t starts at 0.0; leaf by leaf, ascending, T[i][i][d] += v[d] * a_i and T[i][j][d], T[j][i][d] += v[d] * w_ij (the product rounded,
// then the add: shapx_add).  After the tree's last leaf T[i][i][d] = phi_i - T[i][j0][d] - T[i][j1][d] ... (j ascending in the tree's own features, j != i;
// one subtraction each), so a row of T^t sums to the tree's SHAP value.  A row's result is the float64 sum of the T^t in tree order, rounded to float32
// once when stored.  A greedy leaf of depth 0 contributes nothing (Q7: it never passes) and an entry no tree touches stays +0.0.
//   expected[d] = sum_t sum_l v_l[d] * prod_{e in U_l} z_e, leaves ascending inside the tree sum, trees ascending, float64.
// The answer is indexed by the features the walked trees test: features = the ascending distinct feature indices of the conditions of the trees
// [0, n_trees), K of them; values float32 [m][K][K][D].
//
//   ShapxRecords   the row-independent half, built on the host per call: per leaf its merged set (tree-local slots, z), per condition its merged index,
//                  per tree its own features; the streaming kernel's table offsets and item list
//   shapx_row      one row through the trees: the host evaluation and the one-thread-per-row kernel are this function
//   shapx_plan     rows per block and LDS of the streaming kernel, or its refusal
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "leaf_accum.h"
#include "model.h"
#include "shap_core.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GBRL_SHAPX_HD __host__ __device__
#else
#define GBRL_SHAPX_HD
#endif

namespace gbrl {
namespace kern {

constexpr int kShapxMaxN = 30;                               // merged features of a path: a model file holds max_depth <= 30
constexpr int kShapxStreamN = 8;                             // ... of the streaming kernel: its table has 2^n patterns per leaf
constexpr int kShapxStreamRows = 64;                         // rows of a block's code tile
constexpr size_t kShapxTableBudget = size_t(256) << 20;      // bytes of the streaming kernel's weight table
constexpr size_t kShapxScratchBudget = kShapScratchBudget;   // bytes of float64 scratch a launch of the one-thread-per-row kernel may fill

struct ShapxLeafRec { int32_t n, first, tab, pad; };   // merged features, offset of its merged entries, offset (doubles) of its table or -1
struct ShapxTreeRec { int32_t nt, first; };            // the tree's own features, offset of their slots in tmap

GBRL_SHAPX_HD inline int shapx_weights_len(int n) { return n + n * (n - 1) / 2; }
GBRL_SHAPX_HD inline int shapx_pair(int i, int j, int n) { return n + i * n - i * (i + 1) / 2 + (j - i - 1); }   // i < j
GBRL_SHAPX_HD inline double shapx_add(double acc, double v, double w) {
#pragma clang fp contract(off)
    const double term = v * w;
    return acc + term;
}

// wtab[n * kShapxMaxN + k] = W(k, n), 1 <= n <= kShapxMaxN, k < n
inline std::vector<double> shapx_w_table() {
#pragma clang fp contract(off)
    std::vector<double> w(static_cast<size_t>(kShapxMaxN + 1) * kShapxMaxN, 0.0);
    for (int n = 1; n <= kShapxMaxN; ++n) {
        double *row = &w[static_cast<size_t>(n) * kShapxMaxN];
        row[0] = 1.0 / static_cast<double>(n);
        for (int k = 1; k < n; ++k) row[k] = row[k - 1] * static_cast<double>(k) / static_cast<double>(n - k);
    }
    return w;
}

// out[i] = a_i (i < n), out[shapx_pair(i, j, n)] = w_ij (i < j): the weights of one leaf for the pattern o
GBRL_SHAPX_HD inline void shapx_leaf_weights(int n, const double *z, uint32_t o, const double *wtab, double *out) {
#pragma clang fp contract(off)
    double q[kShapxMaxN + 1], qi[kShapxMaxN + 1], qj[kShapxMaxN + 1];
    int h = 0;
    q[0] = 1.0;
    for (int e = 0; e < n; ++e)   // extend: q(x) *= (z_e + x) for every hot e
        if ((o >> e) & 1u) {
            q[h + 1] = q[h];
            for (int k = h; k >= 1; --k) q[k] = q[k] * z[e] + q[k - 1];
            q[0] = q[0] * z[e];
            ++h;
        }
    const double *wn = wtab + static_cast<size_t>(n) * kShapxMaxN, *wp = wtab + static_cast<size_t>(n > 1 ? n - 1 : 1) * kShapxMaxN;
    for (int i = 0; i < n; ++i) {
        const bool hot_i = ((o >> i) & 1u) != 0;
        int hi = h;
        if (hot_i) {   // unwind z_i
            hi = h - 1;
            if (hi >= 0) qi[hi] = q[h];
            for (int k = hi; k >= 1; --k) qi[k - 1] = q[k] - z[i] * qi[k];
        } else {
            for (int k = 0; k <= h; ++k) qi[k] = q[k];
        }
        double z0 = 1.0, s = 0.0;
        for (int e = 0; e < n; ++e)
            if (e != i && !((o >> e) & 1u)) z0 = z0 * z[e];
        for (int k = 0; k <= hi; ++k) s = s + wn[k] * qi[k];
        const double di = (hot_i ? 1.0 : 0.0) - z[i];
        out[i] = (di * z0) * s;
        for (int j = i + 1; j < n; ++j) {
            const bool hot_j = ((o >> j) & 1u) != 0;
            int hj = hi;
            if (hot_j) {
                hj = hi - 1;
                if (hj >= 0) qj[hj] = qi[hi];
                for (int k = hj; k >= 1; --k) qj[k - 1] = qi[k] - z[j] * qj[k];
            } else {
                for (int k = 0; k <= hi; ++k) qj[k] = qi[k];
            }
            double z2 = 1.0, s2 = 0.0;
            for (int e = 0; e < n; ++e)
                if (e != i && e != j && !((o >> e) & 1u)) z2 = z2 * z[e];
            for (int k = 0; k <= hj; ++k) s2 = s2 + wp[k] * qj[k];
            const double dj = (hot_j ? 1.0 : 0.0) - z[j];
            out[shapx_pair(i, j, n)] = ((0.5 * (di * dj)) * z2) * s2;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the records
struct ShapxRecords {
    std::vector<int32_t> features;       // [K] ascending
    std::vector<ShapxLeafRec> leaf;      // [leaves of the trees [0, stop)]
    std::vector<int32_t> mslot;          // per merged entry: the feature's slot among the tree's own features
    std::vector<double> mz;              // per merged entry: z_e
    std::vector<uint8_t> cond_e;         // [leaves][max_depth]: the merged index of the condition at depth d
    std::vector<uint16_t> ent;           // per leaf, shapx_weights_len(n) items at leaf.first-relative offset ent_first: (slot a << 8) | slot b
    std::vector<int32_t> ent_first;      // [leaves]
    std::vector<ShapxTreeRec> tree;      // [stop]
    std::vector<int32_t> tmap;           // a tree's own features as slots of `features`
    std::vector<double> expected;        // [D]
    int n_max = 0, nt_max = 0;
    size_t table_doubles = 0;            // the streaming table: per leaf 2^n * shapx_weights_len(n); 0 when some n > kShapxStreamN

    static int leaf_end(const Model &m, int t) { return t + 1 < m.meta.n_trees ? m.tree_indices[t + 1] : m.meta.n_leaves; }

    void build(const Model &m, int stop) {
#pragma clang fp contract(off)
        const size_t MD = m.meta.max_depth, D = m.meta.output_dim;
        const int F = m.meta.n_num_features, L = stop > 0 ? leaf_end(m, stop - 1) : 0;
        const bool obl = m.oblivious();
        std::vector<int32_t> slot_of(static_cast<size_t>(std::max(F, 0)), -1), local(static_cast<size_t>(std::max(F, 0)), -1);
        for (int t = 0; t < stop; ++t)
            for (int l = m.tree_indices[t]; l < leaf_end(m, t); ++l) {
                const size_t row = obl ? static_cast<size_t>(t) : static_cast<size_t>(l);
                for (int d = 0; d < m.depths[row]; ++d) slot_of[m.feature_indices[row * MD + d]] = 0;
            }
        for (int f = 0; f < F; ++f)
            if (slot_of[f] == 0) { slot_of[f] = static_cast<int32_t>(features.size()); features.push_back(f); }
        leaf.assign(static_cast<size_t>(L), ShapxLeafRec{0, 0, -1, 0});
        cond_e.assign(static_cast<size_t>(L) * MD, 0);
        ent_first.assign(static_cast<size_t>(L), 0);
        expected.assign(D, 0.0);
        bool table_ok = true;
        for (int t = 0; t < stop; ++t) {
            const int l0 = m.tree_indices[t], l1 = leaf_end(m, t);
            ShapxTreeRec tr{0, static_cast<int32_t>(tmap.size())};
            std::vector<double> et(D, 0.0);
            for (int l = l0; l < l1; ++l) {
                const size_t row = obl ? static_cast<size_t>(t) : static_cast<size_t>(l);
                const int depth = m.depths[row];
                ShapxLeafRec &rec = leaf[l];
                rec.first = static_cast<int32_t>(mslot.size());
                if (depth == 0 && !obl) continue;   // Q7: never reached, nothing explained, nothing expected
                std::vector<int32_t> feats;
                for (int d = 0; d < depth; ++d) {
                    const int32_t f = m.feature_indices[row * MD + d];
                    const double w = static_cast<double>(m.edge_weights[static_cast<size_t>(l) * MD + d]);
                    size_t e = std::find(feats.begin(), feats.end(), f) - feats.begin();
                    if (e == feats.size()) {
                        feats.push_back(f);
                        if (local[f] < tr.first || local[f] >= tr.first + tr.nt || tmap[local[f]] != slot_of[f]) {   // new to this tree
                            local[f] = tr.first + tr.nt++;
                            tmap.push_back(slot_of[f]);
                        }
                        mslot.push_back(local[f] - tr.first);
                        mz.push_back(w);
                    } else {
                        mz[rec.first + e] = mz[rec.first + e] * w;
                    }
                    cond_e[static_cast<size_t>(l) * MD + d] = static_cast<uint8_t>(e);
                }
                rec.n = static_cast<int32_t>(feats.size());
                n_max = std::max(n_max, rec.n);
                double p = 1.0;
                for (int e = 0; e < rec.n; ++e) p = p * mz[rec.first + e];
                for (size_t d = 0; d < D; ++d) et[d] = et[d] + static_cast<double>(m.values[static_cast<size_t>(l) * D + d]) * p;
                if (rec.n > kShapxStreamN) table_ok = false;
                if (table_ok && rec.n > 0) {
                    rec.tab = static_cast<int32_t>(table_doubles);
                    table_doubles += (size_t(1) << rec.n) * shapx_weights_len(rec.n);
                    if (table_doubles * sizeof(double) > kShapxTableBudget) table_ok = false;
                }
            }
            for (size_t d = 0; d < D; ++d) expected[d] = expected[d] + et[d];
            nt_max = std::max(nt_max, tr.nt);
            tree.push_back(tr);
        }
        if (!table_ok) {
            table_doubles = 0;
            for (ShapxLeafRec &rec : leaf) rec.tab = -1;
        }
        for (int l = 0; l < L; ++l) {   // the items of the streaming kernel (slots fit a byte there: shapx_plan declines nt_max > 255)
            const ShapxLeafRec &rec = leaf[l];
            ent_first[l] = static_cast<int32_t>(ent.size());
            ent.resize(ent.size() + shapx_weights_len(rec.n), 0);
            uint16_t *e = ent.data() + ent_first[l];
            for (int i = 0; i < rec.n; ++i) {
                const int a = mslot[rec.first + i] & 255;
                e[i] = static_cast<uint16_t>((a << 8) | a);
                for (int j = i + 1; j < rec.n; ++j) e[shapx_pair(i, j, rec.n)] = static_cast<uint16_t>((a << 8) | (mslot[rec.first + j] & 255));
            }
        }
        // (no vector is left empty: each has a device copy)
        if (mslot.empty()) { mslot.push_back(0); mz.push_back(1.0); }
        if (ent.empty()) ent.push_back(0);
        if (tmap.empty()) tmap.push_back(0);
        if (cond_e.empty()) cond_e.push_back(0);
    }
};

// what shapx_row reads: the model's arrays and the records (host vectors, or their device copies)
struct ShapxView {
    const int32_t *tree_indices, *depths, *feature_indices;
    const uint8_t *directions;
    const float *values;
    const ShapxLeafRec *leaf;
    const int32_t *mslot;
    const double *mz;
    const uint8_t *cond_e;
    const ShapxTreeRec *tree;
    const int32_t *tmap;
    const double *wtab;
    int n_leaves, n_trees_model, max_depth, D, K, oblivious;
};

// whether the row agrees with the path of `leaf` at every condition of merged feature e, for every e: the pattern o.  pass(c, f): the row's cell of
// feature f is above the threshold of condition slot c
template <typename Pass>
GBRL_SHAPX_HD inline uint32_t shapx_pattern(const ShapxView &v, int t, int leaf, int n, Pass pass) {
    const int md = v.max_depth;
    const size_t row = v.oblivious ? static_cast<size_t>(t) : static_cast<size_t>(leaf);
    const int depth = v.depths[row], l = leaf - v.tree_indices[t];
    uint32_t o = (1u << n) - 1u;
    for (int d = 0; d < depth; ++d) {
        const int c = static_cast<int>(row) * md + d;
        const bool dir = v.oblivious ? ((l >> (depth - 1 - d)) & 1) != 0 : v.directions[static_cast<size_t>(leaf) * md + d] != 0;
        if (pass(c, v.feature_indices[c]) != dir) o &= ~(1u << v.cond_e[static_cast<size_t>(leaf) * md + d]);
    }
    return o;
}

// a tree's matrix T [nt][nt][D] after its last leaf: the diagonal, then the add into phi [K][K][D]
GBRL_SHAPX_HD inline void shapx_finish_tree(const ShapxView &v, const ShapxTreeRec &tr, double *T, double *phi) {
#pragma clang fp contract(off)
    const int nt = tr.nt, D = v.D, K = v.K;
    const int32_t *km = v.tmap + tr.first;
    for (int a = 0; a < nt; ++a)
        for (int d = 0; d < D; ++d) {
            double dg = T[(a * nt + a) * D + d];
            for (int b = 0; b < nt; ++b)
                if (b != a) dg = dg - T[(a * nt + b) * D + d];
            T[(a * nt + a) * D + d] = dg;
        }
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b)
            for (int d = 0; d < D; ++d) {
                double *p = phi + (static_cast<size_t>(km[a]) * K + km[b]) * D + d;
                *p = *p + T[(a * nt + b) * D + d];
            }
}

// one row through the trees [0, n_trees): phi [K][K][D] (zeroed here), T [nt_max][nt_max][D] and w [shapx_weights_len(n_max)] are the caller's scratch
template <typename Pass>
GBRL_SHAPX_HD inline void shapx_row(const ShapxView &v, int n_trees, Pass pass, double *phi, double *T, double *w) {
    const int D = v.D;
    for (int i = 0; i < v.K * v.K * D; ++i) phi[i] = 0.0;
    for (int t = 0; t < n_trees; ++t) {
        const ShapxTreeRec tr = v.tree[t];
        const int nt = tr.nt;
        if (nt == 0) continue;
        for (int i = 0; i < nt * nt * D; ++i) T[i] = 0.0;
        const int l1 = t + 1 < v.n_trees_model ? v.tree_indices[t + 1] : v.n_leaves;
        for (int leaf = v.tree_indices[t]; leaf < l1; ++leaf) {
            const ShapxLeafRec rec = v.leaf[leaf];
            const int n = rec.n;
            if (n == 0) continue;
            shapx_leaf_weights(n, v.mz + rec.first, shapx_pattern(v, t, leaf, n, pass), v.wtab, w);
            const int32_t *sl = v.mslot + rec.first;
            const float *val = v.values + static_cast<size_t>(leaf) * D;
            for (int i = 0; i < n; ++i) {
                for (int d = 0; d < D; ++d) {
                    double *p = T + (sl[i] * nt + sl[i]) * D + d;
                    *p = shapx_add(*p, static_cast<double>(val[d]), w[i]);
                }
                for (int j = i + 1; j < n; ++j)
                    for (int d = 0; d < D; ++d) {
                        double *p = T + (sl[i] * nt + sl[j]) * D + d, *q = T + (sl[j] * nt + sl[i]) * D + d;
                        *p = shapx_add(*p, static_cast<double>(val[d]), w[shapx_pair(i, j, n)]);
                        *q = shapx_add(*q, static_cast<double>(val[d]), w[shapx_pair(i, j, n)]);
                    }
            }
        }
        shapx_finish_tree(v, tr, T, phi);
    }
}

// ------------------------------------------------------------------------------------------------------------ the launch plans
// LDS of a block of the streaming kernel: phi [rows][K * K * D] and T [rows][nt_max^2 * D] float64, the code tile of 64 rows, a pattern and the
// decision bits per row.  rows is what fits, at most 64; 0 declines: n_max above the table's, a table over its budget, slots that do not fit a byte
struct ShapxPlan { bool fits; int rows; size_t lds, row_doubles; };
inline ShapxPlan shapx_plan(int K, int nt_max, int n_max, int G, int D, size_t table_doubles, size_t budget = kStreamLdsBudget) {
    ShapxPlan p{false, 0, 0, 0};
    p.row_doubles = (static_cast<size_t>(K) * K + static_cast<size_t>(nt_max) * nt_max) * static_cast<size_t>(std::max(D, 1));
    const size_t fixed = static_cast<size_t>(kShapxStreamRows) * (((static_cast<size_t>(G) * 8) | 1) + 2) * sizeof(uint32_t);
    if (K < 1 || n_max < 1 || n_max > kShapxStreamN || nt_max > 255 || table_doubles == 0 || fixed + p.row_doubles * sizeof(double) > budget) return p;
    p.fits = true;
    p.rows = static_cast<int>(std::min<size_t>((budget - fixed) / (p.row_doubles * sizeof(double)), kShapxStreamRows));
    p.lds = fixed + static_cast<size_t>(p.rows) * p.row_doubles * sizeof(double);
    return p;
}

// rows per launch of the one-thread-per-row kernel: their float64 scratch (phi, T, w per row) within the budget, and at least one
inline size_t shapx_general_row_doubles(int K, int nt_max, int n_max, int D) {
    return (static_cast<size_t>(K) * K + static_cast<size_t>(nt_max) * nt_max) * static_cast<size_t>(D) + static_cast<size_t>(shapx_weights_len(n_max));
}
inline int shapx_general_rows(size_t row_doubles, size_t budget = kShapxScratchBudget) {
    return static_cast<int>(std::min<size_t>(std::max<size_t>(budget / (std::max<size_t>(row_doubles, 1) * sizeof(double)), 1), size_t(1) << 24));
}

// ---- the argument checks that need no device: an empty string, or the refusal's text behind "<call>: "
inline std::string shapx_model_error(const Model &m, int n_trees) {
    if (m.meta.n_cat_features > 0) return "not available on a model with categorical columns";
    if (m.meta.n_trees == 0) return "the model has no trees";
    if (n_trees != -1 && (n_trees < 1 || n_trees > m.meta.n_trees))
        return "n_trees " + std::to_string(n_trees) + " is outside [1, " + std::to_string(m.meta.n_trees) + "], the model's trees (None / -1: all)";
    if (m.meta.max_depth > kShapxMaxN) return "max_depth above " + std::to_string(kShapxMaxN);
    return std::string();
}
inline std::string shapx_width_error(int K, int D) {
    if (static_cast<unsigned long long>(K) * static_cast<unsigned long long>(K) * static_cast<unsigned long long>(D) >= (1ull << 31))
        return "a row of the matrix, " + std::to_string(K) + " x " + std::to_string(K) + " features x " + std::to_string(D) + " outputs, has 2^31 elements or more";
    return std::string();
}
inline std::string shapx_matrix_error(long long m, int K, int D) {
    if (static_cast<unsigned long long>(m) * static_cast<unsigned long long>(K) * static_cast<unsigned long long>(K) * static_cast<unsigned long long>(D) >= (1ull << 31))
        return "the matrix of " + std::to_string(m) + " rows x " + std::to_string(K) + " x " + std::to_string(K) + " features x " + std::to_string(D) +
               " outputs has 2^31 elements or more: pass rows= to explain fewer rows, or use shap_interaction_importance_prepared";
    return std::string();
}

}  // namespace kern
}  // namespace gbrl
