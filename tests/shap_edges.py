"""Shared by tests/test_shap_edges_host.py (CPU: the host evaluation against the reference's values) and tests/test_gpu_shap_edges.py (k_shap
against the host evaluation, byte for byte): loading the shap_edge_*.npz fixtures (tests/golden/shap_edge_cases.py), the launch plan through
the C ABI, the SHAP calls both files compare, and the rows with edge values -- cells exactly on a threshold and one float32 ulp to either side,
NaN / inf / signed zeros / a subnormal in split features, unseen, empty and 127-byte categorical cells."""
import ctypes
import functools
import os

import numpy as np

import cases as K
import shap_edge_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOOKS = ("GBRL_HIP_SHAP_HOST", "GBRL_HIP_SHAP_DEVICE_ONLY")
MANY_ROWS = 300          # several blocks at every samples-per-block of the table (85 at most)
NEVER_SEEN, LONG_CELL = b"zz_never_trained", b"q" * 127


@functools.lru_cache(maxsize=None)
def _lib():
    import gbrl_amd
    so = ctypes.CDLL(gbrl_amd.LIB_PATH)
    so.gbrl_hip_shap_plan.restype = ctypes.c_int
    so.gbrl_hip_shap_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return so


def plan(max_depth, D):
    """(threads per block, samples per block) of k_shap for a model shape; (0, 0): the kernel declines."""
    nt, per = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib().gbrl_hip_shap_plan(max_depth, D, ctypes.byref(nt), ctypes.byref(per)) == 0
    return nt.value, per.value


@functools.lru_cache(maxsize=None)
def fixture(name):
    """case, the fixture's arrays, the case's inputs (digest checked) and the polynomial vectors of the model's max_depth; read-only."""
    with np.load(os.path.join(GOLDEN, "shap_edge_" + name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    case = S.BY_NAME[name]
    X, Xc, G, y = K.make_inputs(case)
    assert K.inputs_digest(X, Xc, G, y) == str(g["inputs_sha256"]), "input synthesis drifted from the fixture"
    base, norm, offset = K.poly_vectors(case["depth"])
    for a in (X, Xc, G, base, norm, offset) + tuple(g.values()):
        if a is not None:
            a.setflags(write=False)
    return case, g, X, Xc, G, (norm, base, offset)


def load_model(name, tmp_path):
    import gbrl_amd
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(fixture(name)[1]["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


def cycled(a, n):
    """n rows: the case's inputs over and over."""
    return None if a is None else np.ascontiguousarray(a[np.arange(n) % len(a)])


def tree_picks(T):
    return sorted({0, T // 2, T - 1})


def shap_calls(m, xs, xcs, poly):
    """[ensemble_shap, tree_shap of the first, middle and last tree]"""
    return [m.ensemble_shap(xs, xcs, *poly)] + [m.tree_shap(t, xs, xcs, *poly) for t in tree_picks(m.get_num_trees())]


def reference_values(g):
    return [g["shap_ensemble"]] + [g["shap_tree_%d" % t] for t in tree_picks(int(g["n_trees"]))]


def used_conditions(m):
    """([(numeric feature, threshold)], [(categorical feature, trained cell)]) of every condition the trees test, in storage order."""
    e = m.get_ensemble_data()
    depths, fi = np.asarray(e["depths"]), np.asarray(e["feature_indices"])
    fv, num, cv = np.asarray(e["feature_values"]), np.asarray(e["is_numerics"]), np.asarray(e["categorical_values"])
    numeric, categorical = [], []
    for r in range(len(depths)):
        for lvl in range(int(depths[r])):
            c = (int(fi[r, lvl]), np.float32(fv[r, lvl])) if num[r, lvl] else (int(fi[r, lvl]), bytes(cv[r, lvl]))
            dst = numeric if num[r, lvl] else categorical
            if c not in dst:
                dst.append(c)
    return numeric, categorical


def edge_rows(m, X, Xc, max_thresholds=16):
    """(obs, cat_obs, triples): rows that differ from the case's first row in ONE cell.  triples lists (below, on, above) row indices of
    every threshold taken: the cell one float32 ulp under the threshold, exactly on it, one ulp over it."""
    numeric, categorical = used_conditions(m)
    obs, cat, triples = [], [], []

    def add(feature=None, value=None, cat_feature=None, cell=None, base=0):
        x = None if X is None else X[base % len(X)].copy()
        c = None if Xc is None else Xc[base % len(Xc)].copy()
        if feature is not None:
            x[feature] = value
        if cat_feature is not None:
            c[cat_feature] = cell
        obs.append(x)
        cat.append(c)
        return len(obs) - 1

    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    for k, (f, t) in enumerate(numeric[:max_thresholds]):
        below, above = np.nextafter(t, lo), np.nextafter(t, hi)
        # `x > t` is the only use of the cell, so `on` and `below` must walk the same way: no other threshold of the feature separates them
        assert not any(g == f and u == below for g, u in numeric), "two adjacent thresholds on one feature"
        triples.append((add(f, below, base=k), add(f, t, base=k), add(f, above, base=k)))
    specials = [np.float32(v) for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40)]
    assert specials[-1] > 0 and specials[-1] < np.finfo(np.float32).tiny
    for f in sorted({f for f, _ in numeric}):
        for v in specials:
            add(f, v, base=f)
    if X is not None:
        for v in specials:                    # every numeric cell of the row at once
            obs.append(np.full(X.shape[1], v, np.float32))
            cat.append(None if Xc is None else Xc[0].copy())
    if Xc is not None:
        trained = sorted({c for _, c in categorical})
        assert trained, "the case has categorical columns but no categorical condition"
        cells = trained + [NEVER_SEEN, b"", LONG_CELL, trained[0] + b"x" * (127 - len(trained[0]))]   # the last: a trained token as a prefix
        for f in range(Xc.shape[1]):
            for k, cell in enumerate(cells):
                add(cat_feature=f, cell=cell, base=k)
        for cell in cells:                    # every categorical cell of the row at once
            obs.append(None if X is None else X[0].copy())
            cat.append(np.full(Xc.shape[1], cell, Xc.dtype))
    xs = None if X is None else np.ascontiguousarray(np.stack(obs), np.float32)
    xcs = None if Xc is None else np.ascontiguousarray(np.stack(cat), Xc.dtype)
    return xs, xcs, triples
