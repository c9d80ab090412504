"""Shared by tests/test_shap_interactions_host.py and tests/test_gpu_shap_interactions.py: small models written by hand into the .gbrl_model format
(no device is needed to make one), and the brute-force float64 reference -- the cover-weighted value function f_S(x) of the ensemble from the stored
paths, and the Shapley interaction index by enumeration of the subsets of the K <= 6 used features.  Nothing here shares code with shapx_core.h."""
import itertools
import math

import numpy as np

import gbrl_amd

F, N = 6, 65          # columns; rows: a full tile of 64 and one more

# id: policy, depth, D, columns the trees may test, trees (a greedy "stump0" case gets a one-leaf tree in second place)
CASES = {"%s_d%d_D%d" % (s, d, D): (p, d, D, F, 4) for s, p in (("obl", "oblivious"), ("grd", "greedy")) for d in (1, 2, 4) for D in (1, 3)}
CASES.update({"obl_repeat": ("oblivious", 4, 3, 2, 4), "grd_repeat": ("greedy", 4, 1, 2, 4), "grd_stump0": ("greedy", 2, 3, F, 4), "obl_k1": ("oblivious", 2, 1, 1, 3),
              "grd_k1": ("greedy", 2, 3, 1, 3)})


def _trees(name, rng, threshold):
    """[(leaves: [(value [D], [(feature, threshold, direction, edge weight)])])]; threshold(f) draws a threshold of column f"""
    policy, depth, D, cols, T = CASES[name]
    trees = []
    for t in range(T):
        if policy == "oblivious":
            conds = [(f, threshold(f)) for f in rng.integers(cols, size=depth).tolist()]
            leaves = [[(f, v, (l >> (depth - 1 - j)) & 1, rng.uniform(0.1, 0.9)) for j, (f, v) in enumerate(conds)] for l in range(1 << depth)]
        elif name == "grd_stump0" and t == 1:
            leaves = [[]]
        else:
            def grow(path):   # depth-first, the left (direction 0) child first; the first path goes to full depth
                if len(path) == depth or (path and path[-1][2] == 1 and rng.random() < 0.3):
                    return [path]
                f = int(rng.integers(cols))
                v, w = threshold(f), rng.uniform(0.1, 0.9)
                return grow(path + [(f, v, 0, 1.0 - w)]) + grow(path + [(f, v, 1, w)])
            leaves = grow([])
        trees.append([(rng.standard_normal(D).astype(np.float32), path) for path in leaves])
    return trees


def hand_model(name, path, thresholds=None, seed=0):
    """the case's model, loaded from a file written here.  thresholds: float32 [F, n_bins] to draw the conditions' thresholds from (a data set's), or None"""
    policy, depth, D, cols, T = CASES[name]
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    draw = (lambda f: np.float32(rng.standard_normal())) if thresholds is None else (lambda f: thresholds[f, int(rng.integers(4, thresholds.shape[1] - 4))])
    trees = _trees(name, rng, draw)
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=32, split_score_func="L2", generator_type="Quantile", grow_policy=policy,
                      device="cpu", batch_size=64)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    assert m.save(str(path)) == 0
    raw = path.read_bytes()
    # header 24, metadata 80, two flags, the name; then 15 records (a presence byte and the payload; empty without trees), then the optimizers
    meta = np.frombuffer(raw, np.int32, 20, 24).copy()
    at = head_end = 24 + 80 + 2 + 8 + int(np.frombuffer(raw, np.uint64, 1, 24 + 80 + 2)[0])
    old = []
    for size in (4 * D, 4 * F, 0, 0, 0, 0, 0, 0, 4 * F, 4 * F, 4 * F, F, 0, 0, 0):
        old.append(raw[at:at + 1 + size])
        at += 1 + size
    obl = policy == "oblivious"
    L = sum(len(t) for t in trees)
    S = T if obl else L
    dep, fi, fv = np.zeros(S, np.int32), np.zeros((S, depth), np.int32), np.zeros((S, depth), np.float32)
    val, ew, dirs, first = np.zeros((L, D), np.float32), np.zeros((L, depth), np.float32), np.zeros((L, depth), np.uint8), []
    l = 0
    for t, leaves in enumerate(trees):
        first.append(l)
        for v, p in leaves:
            s = t if obl else l
            dep[s], val[l] = len(p), v
            for j, (f, thr, d, w) in enumerate(p):
                fi[s, j], fv[s, j], dirs[l, j], ew[l, j] = f, thr, d, w
            l += 1
    rec = lambda a: b"\x01" + np.ascontiguousarray(a).tobytes()
    new = list(old)
    new[2], new[3], new[4], new[5], new[6], new[7] = rec(np.array(first, np.int32)), rec(dep), rec(val), rec(fi), rec(fv), rec(ew)
    new[12], new[13], new[14] = rec(np.ones((S, depth), np.uint8)), rec(dirs), rec(np.zeros(S * depth * 128, np.uint8))
    meta[0], meta[1], meta[17], meta[18], meta[19] = L, T, F, 0, T
    path.write_bytes(raw[:24] + meta.tobytes() + raw[24 + 80:head_end] + b"".join(new) + raw[at:])
    return gbrl_amd.GBRL.load(str(path))


def rows_on_thresholds(m, X):
    """X with row 0 put exactly on the first tree's first threshold"""
    e = m.get_ensemble_data()
    X = X.copy()
    X[0, int(np.asarray(e["feature_indices"])[0, 0])] = np.asarray(e["feature_values"])[0, 0]
    return X


def reference(m, X, n_trees=None):
    """float64: (features [K], Phi [n, K, K, D], expected [D], reached [n, D]: the raw sum of the leaf values each row reaches)"""
    e, obl = m.get_ensemble_data(), m.get_metadata()["grow_policy"] == "Oblivious"
    ti, dep, fi, fv, dirs = (np.asarray(e[k]) for k in ("tree_indices", "depths", "feature_indices", "feature_values", "inequality_directions"))
    val, ew = np.asarray(e["values"], np.float64), np.asarray(e["edge_weights"], np.float64)
    n, D, L = len(X), val.shape[1], len(val)
    paths = []   # (value, {feature: (z, o [n])})
    for t in range(len(ti) if n_trees is None else n_trees):
        for l in range(ti[t], ti[t + 1] if t + 1 < len(ti) else L):
            s = t if obl else l
            if dep[s] == 0 and not obl:
                continue
            by = {}
            for j in range(dep[s]):
                z, o = by.get(int(fi[s, j]), (1.0, np.ones(n, bool)))
                by[int(fi[s, j])] = (z * ew[l, j], o & ((X[:, fi[s, j]] > fv[s, j]) == (dirs[l, j] != 0)))
            paths.append((val[l], by))
    features = sorted({f for _, by in paths for f in by})
    K = len(features)
    assert K <= 6

    def f_S(S):
        out = np.zeros((n, D))
        for v, by in paths:
            w = np.ones(n)
            for f, (z, o) in by.items():
                w = w * (o if S >> features.index(f) & 1 else z)
            out += w[:, None] * v
        return out

    f = [f_S(S) for S in range(1 << K)]
    Phi, fact = np.zeros((n, K, K, D)), math.factorial
    for i in range(K):
        others = [k for k in range(K) if k != i]
        phi_i = sum(fact(len(c)) * fact(K - len(c) - 1) / fact(K) * (f[sum(1 << k for k in c) | 1 << i] - f[sum(1 << k for k in c)])
                    for r in range(K) for c in itertools.combinations(others, r))
        for j in others:
            rest = [k for k in others if k != j]
            for r in range(K - 1):
                for c in itertools.combinations(rest, r):
                    S = sum(1 << k for k in c)
                    Phi[:, i, j] += fact(r) * fact(K - r - 2) / (2 * fact(K - 1)) * (f[S | 1 << i | 1 << j] - f[S | 1 << i] - f[S | 1 << j] + f[S])
        Phi[:, i, i] = phi_i - Phi[:, i, others].sum(1) if K > 1 else phi_i
    return np.array(features, np.int32), Phi, f[0][0], f[-1]
