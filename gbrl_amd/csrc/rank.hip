// rank.hip -- gfx950 kernels behind GBRL::rank_gradient (rank_core.h has the rule; every figure below has the host rule's bits).  Queries are runs
// of consecutive rows, 1 to kRankMaxQuery (1024) of them, described by off int32 [Q + 1]; the shapes range from millions of queries of 2 rows to a
// few of 1024, so no kernel gives a query a block: every row kernel runs one lane per row, 256 threads, and a lane loops over the rows of its own
// query -- lanes of a wave that share a query read the same partner address (one broadcast load), lanes of small queries read neighbouring ones.
//
//   once per call (labels do not change)
//   k_rank_rows        one lane per row: the row's query by bisection of off (qid), the label check (the first bad row by an integer atomicMin),
//                      the row's slot t in the descending label order (labels above it, equal labels before it), ideal[off_q + t] = gain(l) * disc[t]
//                      (a permutation inside the query: every slot is written once), beats[i] = rows of the query with a smaller label.
//   k_rank_queries     one lane per query: maxDCG_q = the sum of ideal[off_q ..] in slot order, inv_q, and the pair count P = sum of beats by one
//                      integer atomicAdd per query (exact, order-free).
//   per gradient
//   k_rank_positions   one lane per row: pos(i) by the loop over the query's scores; a score that is not finite sets kRankBadPred; term[i] =
//                      gain(l) * disc[pos] for the DCG.
//   k_rank_pairs       <LAMBDARANK, WITH_HESS, WITH_LOSS> one lane per row: rank_accumulate over the partners in ascending row order, two float64
//                      accumulators in registers (three with the pairwise loss: the logistic row loss of the pairs the row wins, predict_loss.h's
//                      expression), g = (float)acc_g, h = (float)acc_h; the loss partial per wave of 64 rows through staged_wave_sum in the layout
//                      k_staged_finish sums.  The discount table is read from global memory (8 KiB, L1/L2-resident).
//   k_rank_ndcg        one lane per query: DCG_q = the sum of term[off_q ..] in row order, ndcg_q; one float64 partial per wave of 64 queries, the
//                      same butterfly and finish (lambdarank's loss is 1 - sum / Q).
//
// No kernel here uses scratch or LDS; there are no floating-point atomics.
#include "kernels.h"
#include "kernels_common.h"
#include "predict_loss.h"
#include "rank_core.h"

namespace gbrl {
namespace kern {

namespace {

__global__ __launch_bounds__(256) void k_rank_rows(const int32_t *__restrict__ labels, const int32_t *__restrict__ off, int n, int Q, const double *__restrict__ disc,
                                                   int ndcg_at, int32_t *__restrict__ qid, double *__restrict__ ideal, int32_t *__restrict__ beats,
                                                   unsigned long long *__restrict__ stat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = Q;   // the q with off[q] <= i < off[q + 1] (off[0] = 0, off[Q] = n, strictly ascending)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    qid[i] = lo;
    const int r0 = off[lo], r1 = off[lo + 1];
    int32_t l = labels[i];
    if (rank_bad_label(l)) {
        atomicMin(&stat[1], static_cast<unsigned long long>(i));
        l = 0;   // (the call is refused: nothing of it is used)
    }
    int slot = 0, below = 0;
    for (int j = r0; j < r1; ++j) {
        const int32_t lj = labels[j];
        slot += (lj > l || (lj == l && j < i)) ? 1 : 0;
        below += lj < l ? 1 : 0;
    }
    ideal[r0 + slot] = rank_dcg_term(l, disc, slot, ndcg_at);
    beats[i] = below;
}

__global__ __launch_bounds__(256) void k_rank_queries(const int32_t *__restrict__ off, int Q, const double *__restrict__ ideal, const int32_t *__restrict__ beats,
                                                      double *__restrict__ max_dcg, double *__restrict__ inv, unsigned long long *__restrict__ stat) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int r0 = off[q], r1 = off[q + 1];
    double acc = 0.0;
    unsigned long long pairs = 0;
    for (int j = r0; j < r1; ++j) {
        acc = rank_add(acc, ideal[j]);
        pairs += static_cast<unsigned long long>(beats[j]);
    }
    max_dcg[q] = acc;
    inv[q] = rank_inverse(acc);
    if (pairs != 0) atomicAdd(&stat[2], pairs);
}

__global__ __launch_bounds__(256) void k_rank_positions(const float *__restrict__ s, const int32_t *__restrict__ labels, const int32_t *__restrict__ off,
                                                        const int32_t *__restrict__ qid, int n, const double *__restrict__ disc, int ndcg_at,
                                                        int32_t *__restrict__ pos, double *__restrict__ term, unsigned long long *__restrict__ stat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = qid[i];
    const int r0 = off[q], r1 = off[q + 1];
    const float si = s[i];
    if (newton_bad_pred(si)) atomicOr(&stat[0], static_cast<unsigned long long>(kRankBadPred));
    int p = 0;
    for (int j = r0; j < r1; ++j) p += rank_before(s[j], j, si, i) ? 1 : 0;
    pos[i] = p;   // (< r1 - r0 <= kRankMaxQuery also with a NaN among the scores: every compare is then false)
    term[i] = rank_dcg_term(labels[i], disc, p, ndcg_at);
}

template <bool LAMBDARANK, bool WITH_HESS, bool WITH_LOSS>
__global__ __launch_bounds__(256) void k_rank_pairs(const float *__restrict__ s, const int32_t *__restrict__ labels, const int32_t *__restrict__ pos,
                                                    const int32_t *__restrict__ off, const int32_t *__restrict__ qid, const double *__restrict__ inv, int n,
                                                    const double *__restrict__ disc, int ndcg_at, float *__restrict__ g_out, float *__restrict__ h_out,
                                                    double *__restrict__ loss_part, int loss_nb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    if (!live && !WITH_LOSS) return;   // (with the loss whole waves stay for the butterfly)
    double acc_g = 0.0, acc_h = 0.0, acc_l = 0.0;
    if (live) {
        const int q = qid[i];
        const int r0 = off[q], r1 = off[q + 1];
        const float si = s[i];
        const int32_t li = labels[i];
        const int pi = LAMBDARANK ? pos[i] : 0;
        const double inv_q = LAMBDARANK ? inv[q] : 1.0;
        for (int j = r0; j < r1; ++j) {
            const int32_t lj = labels[j];
            if (lj == li) continue;   // (also j == i)
            const float sj = s[j];
            rank_accumulate<LAMBDARANK>(si, li, pi, sj, lj, LAMBDARANK ? pos[j] : 0, disc, ndcg_at, inv_q, acc_g, acc_h);
            if constexpr (WITH_LOSS)
                if (li > lj) acc_l += logistic_loss_term(__fsub_rn(si, sj), 1.0f);
        }
        if (g_out != nullptr) g_out[i] = static_cast<float>(acc_g);
        if constexpr (WITH_HESS) h_out[i] = static_cast<float>(acc_h);
    }
    if constexpr (WITH_LOSS) {
        acc_l = staged_wave_sum(acc_l);
        const int wave = i / kStagedRows;   // 256 = 4 x 64: a wave holds the rows of one partial
        if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < loss_nb) loss_part[wave] = acc_l;
    }
}

__global__ __launch_bounds__(256) void k_rank_ndcg(const int32_t *__restrict__ off, int Q, const double *__restrict__ term, const double *__restrict__ max_dcg,
                                                   const double *__restrict__ inv, double *__restrict__ ndcg, double *__restrict__ part, int nb) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;   // (whole waves stay for the butterfly)
    double v = 0.0;
    if (q < Q) {
        const int r0 = off[q], r1 = off[q + 1];
        double acc = 0.0;
        for (int j = r0; j < r1; ++j) acc = rank_add(acc, term[j]);
        v = rank_ndcg(acc, max_dcg[q], inv[q]);
        ndcg[q] = v;
    }
    v = staged_wave_sum(v);
    const int wave = q / kStagedRows;
    if ((threadIdx.x & (kStagedRows - 1)) == 0 && wave < nb) part[wave] = v;
}

}  // namespace

void rank_queries(const int32_t *labels, const int32_t *off, int n, int Q, const double *disc, int ndcg_at, int32_t *qid, double *ideal, int32_t *beats,
                  double *max_dcg, double *inv, unsigned long long *stat, hipStream_t s) {
    if (n <= 0 || Q <= 0) return;
    hipLaunchKernelGGL(k_rank_rows, dim3((n + 255) / 256), dim3(256), 0, s, labels, off, n, Q, disc, ndcg_at, qid, ideal, beats, stat);
    hipLaunchKernelGGL(k_rank_queries, dim3((Q + 255) / 256), dim3(256), 0, s, off, Q, ideal, beats, max_dcg, inv, stat);
}

void rank_rows(int objective, const float *scores, const int32_t *labels, const int32_t *off, const int32_t *qid, const double *max_dcg, const double *inv, int n,
               int Q, const double *disc, int ndcg_at, int32_t *pos, double *term, float *g_out, float *h_out, double *pair_part, double *ndcg, double *ndcg_part,
               unsigned long long *stat, hipStream_t s, int stages) {
    if (n <= 0 || Q <= 0) return;
    const dim3 rows((n + 255) / 256), block(256);
    if (stages & kRankStagePositions) hipLaunchKernelGGL(k_rank_positions, rows, block, 0, s, scores, labels, off, qid, n, disc, ndcg_at, pos, term, stat);
    if ((stages & kRankStagePairs) && (g_out != nullptr || h_out != nullptr || pair_part != nullptr)) {
        const int nb = staged_loss_partials(n);
        auto run = [&](auto lam, auto hess, auto loss) {
            hipLaunchKernelGGL((k_rank_pairs<decltype(lam)::value, decltype(hess)::value, decltype(loss)::value>), rows, block, 0, s, scores, labels, pos, off, qid, inv,
                               n, disc, ndcg_at, g_out, h_out, pair_part, nb);
        };
        auto with_flags = [&](auto lam) {
            const bool hess = h_out != nullptr, loss = pair_part != nullptr;
            if (hess && loss) run(lam, std::true_type{}, std::true_type{});
            else if (hess) run(lam, std::true_type{}, std::false_type{});
            else if (loss) run(lam, std::false_type{}, std::true_type{});
            else run(lam, std::false_type{}, std::false_type{});
        };
        if (objective == kObjLambdarank) with_flags(std::true_type{});
        else with_flags(std::false_type{});
    }
    if ((stages & kRankStageNdcg) && ndcg != nullptr) hipLaunchKernelGGL(k_rank_ndcg, dim3((Q + 255) / 256), block, 0, s, off, Q, term, max_dcg, inv, ndcg, ndcg_part, staged_loss_partials(Q));
}

}  // namespace kern
}  // namespace gbrl
