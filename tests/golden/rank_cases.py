"""Inputs and the independent NumPy walk of the ranking objectives (gbrl_amd/csrc/rank_core.h), shared by tests/test_rank_host.py and the GPU tests.

The walk takes its sigmoid and hessian bits from the logistic rules the project already has (objective_gradient_host, objective_hessian_host), its
discounts from rank_discounts(), and sums in float64 with np.cumsum in partner order; nothing of it calls the ranking code."""
import numpy as np

f32 = np.float32
LAYOUT = [1, 2, 61, 3, 64, 65, 190, 257, 1024, 5]     # 1672 rows: queries start at unaligned rows and cross 64- and 256-row boundaries


def scores_and_labels(group, seed, ties=True, max_label=4):
    rng = np.random.default_rng(seed)
    n = int(np.sum(group))
    s = (rng.standard_normal(n) * 2).astype(f32)
    if ties:
        s[rng.random(n) < 0.2] = f32(0.5)               # a fifth of the scores tied
        s[::17] = f32(-0.0)
        s[5::17] = f32(0.0)                             # both zeros
    y = rng.integers(0, max_label + 1, n).astype(np.int32)
    return s, y


DELTAS = np.array([88, -88, 95.5, -95.5, 104, -104, np.nextafter(f32(104), f32(200)), np.nextafter(f32(-104), f32(-200)), 87.3, -87.3, 120, -120, 300, -300, 1e30,
                   -1e30, 0.0, -0.0, 1e-30], f32)


def constructed():
    """(name, scores, labels, group) of the constructed cases"""
    big = np.array([0, 88, -88, 95.5, -95.5, 104, -104, 120, -120, 300, -300, 0.25], f32)
    return [
        ("bradley_terry", np.array([0.3, -1.2], f32), np.array([1, 0], np.int32), [2]),
        ("all_scores_equal", np.full(9, 0.75, f32), np.array([0, 1, 2, 3, 4, 0, 1, 2, 3], np.int32), [4, 5]),
        ("zeros_tie", np.array([0.0, -0.0, 0.0, -0.0, 1.0], f32), np.array([2, 0, 1, 3, 0], np.int32), [5]),
        ("all_labels_zero", np.array([0.1, 0.2, -0.3, 0.0], f32), np.zeros(4, np.int32), [4]),
        ("all_labels_equal", np.array([0.1, 0.2, -0.3, 0.0], f32), np.full(4, 3, np.int32), [1, 3]),
        ("labels_30_and_0", np.array([0.1, 0.2, -0.3, 0.0, 2.0, -2.0], f32), np.array([30, 0, 0, 30, 0, 30], np.int32), [6]),
        ("one_row", np.array([1.5], f32), np.array([2], np.int32), [1]),
        ("exp_branches", big, (np.arange(12) % 3).astype(np.int32), [12]),
        # queries of two with labels (1, 0) and scores (d, 0): delta is d itself, at and beyond the branches of obj_exp
        ("exp_branches_pairs", np.stack([DELTAS, np.zeros(len(DELTAS), f32)], axis=1).reshape(-1).copy(), np.tile(np.array([1, 0], np.int32), len(DELTAS)),
         [2] * len(DELTAS)),
    ]


def walk(cpp, s, y, group, objective, ndcg_at=None):
    """the rule, row by row, in NumPy: (g, h, ndcg, positions, pairs)"""
    disc = cpp.rank_discounts().copy()
    if ndcg_at:
        disc[ndcg_at:] = 0.0
    n = len(s)
    g, h = np.zeros(n, f32), np.zeros(n, f32)
    pos = np.zeros(n, np.int32)
    ndcg = np.zeros(len(group), np.float64)
    pairs = 0
    r0 = 0
    for q, m in enumerate(group):
        sq, yq = s[r0:r0 + m], y[r0:r0 + m]
        idx = np.arange(m)
        pq = np.array([np.sum((sq > sq[i]) | ((sq == sq[i]) & (idx < i))) for i in range(m)], np.int64)
        pos[r0:r0 + m] = pq
        gain = np.float64(2.0) ** yq.astype(np.float64) - 1.0
        ideal = np.sort(gain)[::-1] * disc[:m]
        max_dcg = np.cumsum(ideal)[-1]
        inv = np.float64(1.0) / max_dcg if max_dcg > 0 else np.float64(0.0)
        dcg = np.cumsum(gain * disc[pq])[-1]
        ndcg[q] = dcg * inv if max_dcg > 0 else 1.0
        pairs += int(np.sum(yq[:, None] > yq[None, :]))
        for i in range(m):
            part = np.nonzero(yq != yq[i])[0]
            if len(part) == 0:
                continue
            better = yq[i] > yq[part]
            delta = np.where(better, sq[i] - sq[part], sq[part] - sq[i]).astype(f32)     # fl32(s_hi - s_lo)
            rho = cpp.objective_gradient_host((-delta).astype(f32), np.zeros(len(part), f32), "logistic").astype(np.float64)
            eta = cpp.objective_hessian_host(delta, None, "logistic").astype(np.float64)
            if objective == "lambdarank":
                omega = (np.abs(gain[i] - gain[part]) * np.abs(disc[pq[i]] - disc[pq[part]])) * inv
                keep = omega > 0
                part, better, rho, eta, omega = part[keep], better[keep], rho[keep], eta[keep], omega[keep]
                rho, eta = rho * omega, eta * omega
            if len(part) == 0:
                continue
            g[r0 + i] = f32(np.cumsum(np.concatenate(([0.0], np.where(better, -rho, rho))))[-1])
            h[r0 + i] = f32(np.cumsum(np.concatenate(([0.0], eta)))[-1])
        r0 += m
    return g, h, ndcg, pos, pairs


def pairwise_loss(s, y, group):
    """float64 NumPy evaluation of the pairwise loss: the mean over the label-ordered pairs of max(d, 0) - d + log1p(exp(-|d|)), d = fl32(s_i - s_j)"""
    total, pairs, r0 = 0.0, 0, 0
    for m in group:
        sq, yq = s[r0:r0 + m], y[r0:r0 + m]
        d = (sq[:, None] - sq[None, :]).astype(f32).astype(np.float64)[yq[:, None] > yq[None, :]]
        total += float(np.sum(np.maximum(d, 0.0) - d + np.log1p(np.exp(-np.abs(d)))))
        pairs += d.size
        r0 += m
    return (total / pairs if pairs else 0.0), pairs
