// shap.hip -- Linear TreeSHAP on the device (inspection row f4 of SURVEY.md section 8; semantics: shap.cpp:257-364).
//
// Every sample walks ALL nodes of a tree in the same order, so the walk is a uniform program (ShapOp list, built on the host
// from explain.cpp's ShapTree) that every thread executes without divergence; what differs per thread is data: which side of a
// condition the sample is on and the edge probabilities derived from it.  One thread = one (sample, output); its two coefficient
// stacks C, G [max_depth+1][max_depth] live in LDS with the thread as the fastest index (conflict-free); node records and the
// polynomial vectors are uniform reads (scalar cache).  The arithmetic is the host evaluation's, rounding for rounding
// (explain.cpp Walker: same order of additions, same two fused multiply-adds, IEEE divisions), so both give the same bits.
//
// k_shap is a template over what a sample's numeric cells are read through: the float observations (tree_shap / ensemble_shap), or a prepared
// data set's bin codes (shap_prepared / shap_importance_prepared), where the node records hold the bin and the decision is code > bin.  The body
// is one text; everything but the decision is the same instructions.  k_shap_tile_sums / k_shap_finish reduce a chunk of values to the float64
// column sums of shap_core.h's rule.
#include "kernels.h"
#include "kernels_common.h"
#include "shap_core.h"

#pragma clang fp contract(off)

namespace gbrl {
namespace kern {

namespace {

constexpr int kShapMaxThreads = 256;

// ---- what k_shap reads a sample's numeric cells through: `x[feature] > nd.threshold` is the only expression that touches them
// the observations themselves, float32 [n_samples][n_num] (null: a model without numeric features)
struct ShapFloatRows {
    const float *obs;
    int n_num;
    using Row = const float *;
    __device__ __forceinline__ Row row(long long s) const { return obs ? obs + s * n_num : nullptr; }
};
// a prepared data set's bin codes: sample s is data set row rows[row0 + s] (or row0 + s), its cell of feature f the 2-byte code at
// [f / 16][row][f % 16].  The node records of this form hold the condition's bin in the four bytes of `threshold` (bit cast), and
// `x[f] > nd.threshold` is `code > bin` -- the same answer as the float comparison for every float (engine_codes.hip has the rule).
// All D lanes of a sample read the same address.
struct ShapCode {
    int code;
    __device__ __forceinline__ bool operator>(float bin_bits) const { return code > __float_as_int(bin_bits); }
};
struct ShapCodeRow {
    const uint16_t *rec;     // the row's record of group 0
    size_t group_stride;     // n_rows * 16
    __device__ __forceinline__ ShapCode operator[](int f) const { return ShapCode{static_cast<int>(rec[static_cast<size_t>(f >> 4) * group_stride + (f & 15)])}; }
};
struct ShapCodeRows {
    CodeRows cr;
    using Row = ShapCodeRow;
    __device__ __forceinline__ Row row(long long s) const {
        const size_t src = static_cast<size_t>(cr.rows ? cr.rows[cr.row0 + s] : cr.row0 + s);
        return ShapCodeRow{cr.codes + src * kCodeGroup, static_cast<size_t>(cr.n_rows) * kCodeGroup};
    }
};

template <typename Rows>
__global__ __launch_bounds__(kShapMaxThreads) void k_shap(const ShapOp *__restrict__ ops, int n_ops, const ShapNodeRec *__restrict__ nodes,
                                                       const float *__restrict__ leaf_value, const Rows rows, int n_num,
                                                       const int32_t *__restrict__ cat_ids, int n_cat, int n_samples, int D, int md,
                                                       const float *__restrict__ norm, const float *__restrict__ base,
                                                       const float *__restrict__ offset, float *__restrict__ out) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, nt = blockDim.x;
    const int per_block = nt / D;                 // samples per block
    const int s_local = t / D, j = t - s_local * D;
    const long long s = static_cast<long long>(blockIdx.x) * per_block + s_local;
    const bool live = s_local < per_block && s < n_samples;
    // LDS: C [(md+1)*md][nt], G [(md+1)*md][nt], Q [md+1][nt], QA [md+1][nt]
    const int tile = (md + 1) * md;
    float *C = lds + t, *G = lds + tile * nt + t;
    float *Q = lds + 2 * tile * nt + t, *QA = Q + (md + 1) * nt;
    auto at = [nt](float *p, int idx) -> float & { return p[idx * nt]; };
    const typename Rows::Row x = rows.row(live ? s : 0);
    const int32_t *xc = cat_ids ? cat_ids + (live ? s : 0) * n_cat : nullptr;
    float *phi = out + (live ? s : 0) * static_cast<long long>(n_num + n_cat) * D + j;
    uint32_t act = 0, pass = 0;      // bit k: state of the open node at level k (at most one node per level is open)

    for (int o = 0; o < n_ops; ++o) {
        const ShapOp op = ops[o];
        const ShapNodeRec nd = nodes[op.node];
        const int k = op.level;
        const bool tied = nd.flags & 2, leaf = nd.flags & 4;
        if (op.kind == SHAP_ENTER) {
            bool a = false;
            if (k > 0) { const bool par_pass = (pass >> (k - 1)) & 1u; a = (nd.flags & 8) ? par_pass : !par_pass; }   // flag 8: right child
            float q_anc = 0.0f;
            if (tied) {
                const bool ap = (act >> (k - 1)) & 1u;
                a = a && ap && nd.weight > 0.0f;
                if (ap) q_anc = nd.weight_parent > 0.0f ? __fdiv_rn(1.0f, nd.weight_parent) : 0.0f;
            }
            act = a ? (act | (1u << k)) : (act & ~(1u << k));
            float q = 0.0f;
            if (op.via >= 0) {
                if (a) q = nd.weight > 0.0f ? __fdiv_rn(1.0f, nd.weight) : 0.0f;
                for (int i = 0; i < md; ++i) {
                    float c = at(C, (k - 1) * md + i) * (base[i] + q);
                    if (tied) c = __fdiv_rn(c, base[i] + q_anc);
                    at(C, k * md + i) = c;
                }
            } else {
                for (int i = 0; i < md; ++i) at(C, i) = 1.0f;
            }
            at(Q, k) = q;
            at(QA, k) = q_anc;
            if (leaf) {
                const float pv = leaf_value[nd.pred + j] + 0.0f;
                for (int i = 0; i < md; ++i) at(G, k * md + i) = at(C, k * md + i) * pv;
            } else {
                const bool p = (nd.flags & 1) ? x[nd.feature] > nd.threshold : (xc[nd.feature] == nd.cat_id && nd.cat_id != 0);
                pass = p ? (pass | (1u << k)) : (pass & ~(1u << k));
            }
        } else if (op.kind == SHAP_AFTER_LEFT || op.kind == SHAP_AFTER_RIGHT) {
            const float *off = offset + (op.kind == SHAP_AFTER_LEFT ? nd.deg_left : nd.deg_right) * md;
            for (int i = 0; i < md; ++i) {
                const float g = at(G, (k + 1) * md + i) * (off[i] + 0.0f);
                at(G, (k + 1) * md + i) = g;
                at(G, k * md + i) = op.kind == SHAP_AFTER_LEFT ? g : at(G, k * md + i) + g;
            }
        } else {   // SHAP_EXIT: the edge into this node contributes to the feature it tests (Walker::edge_term)
            if (tied && !((act >> (k - 1)) & 1u)) continue;
            float acc_phi = live ? phi[static_cast<long long>(op.via) * D] : 0.0f;
            for (int pass_no = 0; pass_no < (tied ? 2 : 1); ++pass_no) {
                const int d = pass_no == 0 ? nd.n_unique : nd.n_unique_parent;
                const float qq = pass_no == 0 ? at(Q, k) : at(QA, k);
                const float *nv = norm + d * md;
                const float *off = offset + (pass_no == 0 ? 0 : (nd.n_unique_parent - nd.n_unique) * md);
                const int fused_from = d - d % 4;
                float acc = 0.0f;
                for (int i = 0; i < d; ++i) {
                    const float term = __fdiv_rn(at(G, k * md + i) * off[i], base[i] + qq);
                    if (i < fused_from) { const float pr = term * nv[i]; acc = acc + pr; }
                    else acc = __fmaf_rn(term, nv[i], acc);
                }
                acc = __fdiv_rn(acc, static_cast<float>(d));
                acc_phi = __fmaf_rn(pass_no == 0 ? acc : -acc, qq - 1.0f, acc_phi);
            }
            if (live) phi[static_cast<long long>(op.via) * D] = acc_phi;
        }
    }
}

}  // namespace

// threads per block: the largest of 256 / 128 / 64 whose coefficient stacks fit the LDS and that holds one sample's D outputs; 0 = none
int shap_block_threads(int md, int D) {
    if (md < 1 || md > 31) return 0;
    for (int nt = kShapMaxThreads; nt >= 64; nt >>= 1)
        if (nt >= D && sizeof(float) * nt * (2 * (md + 1) * md + 2 * (md + 1)) <= 156 * 1024) return nt;
    return 0;
}

namespace {

template <typename Rows>
void launch_shap(const ShapOp *ops, int n_ops, const ShapNodeRec *nodes, const float *leaf_value, const Rows &rows, int n_num, const int32_t *cat_ids,
                 int n_cat, int n_samples, int D, int md, const float *norm, const float *base, const float *offset, float *out, hipStream_t s) {
    if (n_samples <= 0 || n_ops <= 0) return;
    const int nt = shap_block_threads(md, D);
    static PerDeviceOnce attr_set;   // (one per instantiation)
    if (attr_set.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_shap<Rows>), hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024);
    }
    const int per_block = nt / D;
    const unsigned blocks = static_cast<unsigned>((n_samples + per_block - 1) / per_block);
    const size_t lds = sizeof(float) * nt * (2 * (md + 1) * md + 2 * (md + 1));
    hipLaunchKernelGGL(k_shap<Rows>, dim3(blocks), dim3(nt), lds, s, ops, n_ops, nodes, leaf_value, rows, n_num, cat_ids, n_cat, n_samples, D, md,
                       norm, base, offset, out);
}

// ---- the reduction of a [rows][C] chunk of values (shap_core.h has the rule)
constexpr int kShapSumThreads = 256;

// one thread per (column, tile): the threads of a block read consecutive columns of one row (coalesced) and walk the tile's rows in order.
// part [tiles of the call][2][C]; tile0: the first tile of this chunk
__global__ __launch_bounds__(kShapSumThreads) void k_shap_tile_sums(const float *__restrict__ phi, int rows, int C, double *__restrict__ part, int tile0) {
    const int t = blockIdx.x;
    const int r0 = t * kShapTileRows, n = min(kShapTileRows, rows - r0);
    double *dst = part + static_cast<size_t>(tile0 + t) * 2 * C;
    for (int c = blockIdx.y * kShapSumThreads + threadIdx.x; c < C; c += gridDim.y * kShapSumThreads) {
        double s, a;
        shap_tile_sums(phi + static_cast<size_t>(r0) * C + c, static_cast<size_t>(C), n, &s, &a);
        dst[c] = s;
        dst[C + c] = a;
    }
}

// one thread per (kind, column): the tile partials in ascending order.  sums [2][C]: the sums, then the sums of the absolute values
__global__ __launch_bounds__(kShapSumThreads) void k_shap_finish(const double *__restrict__ part, int tiles, int C2, double *__restrict__ sums) {
    for (int c = blockIdx.x * kShapSumThreads + threadIdx.x; c < C2; c += gridDim.x * kShapSumThreads)
        sums[c] = shap_finish_sums(part + c, static_cast<size_t>(C2), tiles);
}

}  // namespace

void shap_values(const ShapOp *ops, int n_ops, const ShapNodeRec *nodes, const float *leaf_value, const float *obs, int n_num,
                 const int32_t *cat_ids, int n_cat, int n_samples, int D, int md, const float *norm, const float *base,
                 const float *offset, float *out, hipStream_t s) {
    launch_shap(ops, n_ops, nodes, leaf_value, ShapFloatRows{obs, n_num}, n_num, cat_ids, n_cat, n_samples, D, md, norm, base, offset, out, s);
}

void shap_values_codes(const ShapOp *ops, int n_ops, const ShapNodeRec *nodes, const float *leaf_value, const CodeRows &cr, int n_features, int m, int D,
                       int md, const float *norm, const float *base, const float *offset, float *out, hipStream_t s) {
    launch_shap(ops, n_ops, nodes, leaf_value, ShapCodeRows{cr}, n_features, nullptr, 0, m, D, md, norm, base, offset, out, s);
}

void shap_reduce_tiles(const float *phi, int rows, int n_cols, double *part, int tile0, hipStream_t s) {
    if (rows <= 0 || n_cols <= 0) return;
    const unsigned col_blocks = static_cast<unsigned>(std::min<long long>(65535, (static_cast<long long>(n_cols) + kShapSumThreads - 1) / kShapSumThreads));
    hipLaunchKernelGGL(k_shap_tile_sums, dim3(static_cast<unsigned>(shap_tiles(rows)), col_blocks), dim3(kShapSumThreads), 0, s, phi, rows, n_cols, part, tile0);
}

void shap_reduce_finish(const double *part, int tiles, int n_cols, double *sums, hipStream_t s) {
    if (n_cols <= 0) return;
    const long long C2 = 2ll * n_cols;
    const unsigned blocks = static_cast<unsigned>(std::min<long long>(1 << 20, (C2 + kShapSumThreads - 1) / kShapSumThreads));
    hipLaunchKernelGGL(k_shap_finish, dim3(blocks), dim3(kShapSumThreads), 0, s, part, tiles, static_cast<int>(C2), sums);
}

}  // namespace kern
}  // namespace gbrl
