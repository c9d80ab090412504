"""`predict_continue` / `predict_continue_encoded` (include/gbrl_hip.h): a prediction the caller holds over the trees [0, a) carried through the
trees [a, b).  Per (row, output) a prediction is one chain p = fma(-lr(t), value, p) in tree order (optimizer.cpp:110-118), so continuing
the chain from a stored p gives the bits of the whole walk.  "The chain" below is `predict` under GBRL_HIP_PREDICT_GENERIC=1 (the general
kernels: always one walk over the whole range in tree order); every comparison with it is BITWISE.  Every case runs the default path (the
streaming kernel k_continue where it takes the shape) and GBRL_HIP_CONTINUE_GENERIC=1 (k_continue_general) and wants the same bits from both.

The trees are grown on 256 .. 512-row steps at depth 3 .. 4 (cheap), each step on fresh gradients so that the trees differ.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKENS = np.array(["tok%d" % i for i in range(6)], dtype="S128")


def _model(F, Fc, D, depth, policy="oblivious", opts=None, bias=None, name="cont", min_data_in_leaf=0):
    import gbrl_amd
    m = gbrl_amd.GBRL(input_dim=F + Fc, output_dim=D, policy_dim=D, max_depth=depth, min_data_in_leaf=min_data_in_leaf, n_bins=32, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy=policy,
                      verbose=0, device="cpu", learner_name=name)
    m.set_feature_weights(np.ones(F + Fc, np.float32))
    for o in (opts or [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)]):
        m.set_optimizer(**o)
    m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))
    m.set_bias(np.asarray(bias if bias is not None else 0.25 + 0.5 * np.arange(D), np.float32))
    return m


def _batch(rng, n, F, Fc, n_tokens=6):
    X = rng.standard_normal((n, F)).astype(np.float32) if F else None
    Xc = TOKENS[rng.integers(0, n_tokens, (n, Fc))] if Fc else None
    return X, Xc


def _grow(m, rng, trees, F, Fc, D, rows=384):
    for _ in range(trees):
        X, Xc = _batch(rng, rows, F, Fc)
        G = rng.standard_normal((rows, D)).astype(np.float32)
        if F:
            G[:, 0] += X[:, 0] * 2.0
        if Fc:
            G[:, -1] += (Xc[:, 0] == TOKENS[1]) * 3.0
        m.step(X, Xc, np.ascontiguousarray(G.astype(np.float32)))


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _chain(m, X, Xc, a, b):
    """predict over [a, b) by the general kernels; b > 0 (0 would mean n_trees)."""
    assert b > 0
    with _env("GBRL_HIP_PREDICT_GENERIC", "1"):
        return np.asarray(m.predict(X, Xc, a, b))


def _bias_base(m, n):
    bias = np.asarray(m.get_bias(), np.float32).reshape(-1)
    return np.ascontiguousarray(np.tile(bias, (n, 1))) if bias.size > 1 else np.full(n, bias[0], np.float32)


def _base(m, X, Xc, a):
    n = (X if X is not None else Xc).shape[0]
    return _bias_base(m, n) if a == 0 else _chain(m, X, Xc, 0, a)


def _continue_both(m, X, Xc, base, a, b, encoded=None):
    """default path and GBRL_HIP_CONTINUE_GENERIC=1: the same bits; returns them."""
    out = []
    for generic in ("0", "1"):
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            keep = base.copy()
            if encoded is None:
                got = m.predict_continue(X, Xc, base, a, b)
            else:
                got = m.predict_continue_encoded(X, encoded[0], encoded[1], base, a, b)
            assert base.tobytes() == keep.tobytes(), "a NumPy base was modified"
            out.append(np.asarray(got))
    assert out[0].dtype == np.float32 and out[0].shape == base.shape
    assert out[0].tobytes() == out[1].tobytes(), "k_continue and k_continue_general differ over [%d, %d)" % (a, b)
    return out[0]


def _numpy_walk(e, X, Xc, lr, base, start, stop):
    """tests/test_gpu_cfg5_fullsize.py::_numpy_walk restated, started from `base` instead of the bias: oblivious leaf = tree_indices[t] +
    sum_d (x[f_d] > t_d or cell == category) << (depth_t - 1 - d) (predictor.cpp:231-265), pred -= lr * value per row in tree order."""
    ti = np.asarray(e["tree_indices"]); dep = np.asarray(e["depths"]); vals = np.asarray(e["values"], np.float32)
    fi = np.asarray(e["feature_indices"]); fv = np.asarray(e["feature_values"]); isn = np.asarray(e["is_numerics"])
    cv = np.asarray(e["categorical_values"])
    n = X.shape[0]
    pred = np.asarray(base, np.float32).reshape(n, -1).copy()
    lr64 = np.float64(np.float32(lr))
    for t in range(start, stop):
        d_t = int(dep[t])
        leaf = np.full(n, int(ti[t]), np.int64)
        for d in range(d_t):
            right = (X[:, fi[t, d]] > fv[t, d]) if isn[t, d] else (Xc[:, fi[t, d]] == cv[t, d])
            leaf += right.astype(np.int64) << (d_t - 1 - d)
        # fl32(pred - lr * v): exact product in float64, the sum rounded to float64 and then to float32 (a float32 fused multiply-add except
        # on double-rounding ties, which the 1e-5 below absorbs as it does in test_gpu_cfg5_fullsize.py)
        pred = (pred.astype(np.float64) - lr64 * vals[leaf].astype(np.float64)).astype(np.float32)
    return pred


def _split_check(m, X, Xc, a, T, encoded=None):
    want = _chain(m, X, Xc, 0, T)
    base = _base(m, X, Xc, a)
    got = _continue_both(m, X, Xc, base, a, T, encoded)
    assert got.tobytes() == want.tobytes(), "continue(chain(0..%d), %d, %d) != chain(0..%d)" % (a, a, T, T)
    if a == T:
        assert got.tobytes() == base.tobytes()
    return base, got


@pytest.mark.parametrize("F", [16, 13])
@pytest.mark.parametrize("D", [1, 3, 8, 17])
def test_split_anywhere(F, D):
    T = 40
    rng = np.random.default_rng(100 * F + D)
    m = _model(F, 0, D, 4)
    _grow(m, rng, T, F, 0, D)
    assert m.get_num_trees() == T
    e = m.get_ensemble_data()
    for n in (1, 63, 64, 65, 257, 4099):
        X, _ = _batch(rng, n, F, 0)
        for a in (0, 1, 7, 39, 40):
            base, got = _split_check(m, X, None, a, T)
            want = _numpy_walk(e, X, None, 0.1, base, a, T)
            scale = max(float(np.abs(want).mean()), 1e-6)
            err = float(np.max(np.abs(got.reshape(n, -1) - want) / np.maximum(np.abs(want), scale)))
            assert err <= 1e-5, (n, a, err)
        # stop_tree_idx == 0 means n_trees
        base = _base(m, X, None, 7)
        assert _continue_both(m, X, None, base, 7, 0).tobytes() == _chain(m, X, None, 0, T).tobytes()


def test_one_tree_at_a_time_interleaved_with_growth():
    """The RL loop: step, then predict_continue(cache, T-1, T) in place on a device tensor; also the device mirror re-synced after every step."""
    import torch
    F, D, n = 16, 8, 4099
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    m = _model(F, 0, D, 4)
    Xh, _ = _batch(rng, n, F, 0)
    X = torch.from_numpy(Xh).to(dev)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    caches = {g: torch.from_numpy(_bias_base(m, n)).to(dev) for g in ("0", "1")}
    for T in range(1, 31):
        _grow(m, rng, 1, F, 0, D, rows=256)
        want = _chain(m, Xh, None, 0, T)
        for g, cache in caches.items():
            with _env("GBRL_HIP_CONTINUE_GENERIC", g):
                assert m.predict_continue(tup(X), None, tup(cache), T - 1, T) is None
            assert cache.cpu().numpy().tobytes() == want.tobytes(), "cache != chain(0..%d) (generic=%s)" % (T, g)


def test_greedy_with_categorical_columns_raw_cells_and_encoded_ids():
    F, Fc, D, T = 6, 3, 3, 24
    rng = np.random.default_rng(11)
    m = _model(F, Fc, D, 4, policy="greedy")
    _grow(m, rng, T, F, Fc, D, rows=512)
    e = m.get_ensemble_data()
    assert (np.asarray(e["is_numerics"]) == 0).any(), "no categorical condition was grown"
    for n in (1, 65, 257, 4099):
        X, Xc = _batch(rng, n, F, Fc)
        ids, token = m.encode_categorical(Xc)
        ids = np.asarray(ids)
        for a in (0, 1, 7, T - 1, T):
            base, raw = _split_check(m, X, Xc, a, T)
            enc = _continue_both(m, X, None, base, a, T, encoded=(ids, token))
            assert enc.tobytes() == raw.tobytes()


def test_a_stale_dictionary_token_is_refused():
    F, Fc, D = 4, 2, 2
    rng = np.random.default_rng(3)
    tokens20 = np.array(["c%02d" % i for i in range(20)], dtype="S128")
    m = _model(F, Fc, D, 3, policy="greedy")
    X = rng.standard_normal((512, F)).astype(np.float32)
    Xc = tokens20[rng.integers(0, 20, (512, Fc))]
    m.step(X, Xc, rng.standard_normal((512, D)).astype(np.float32))
    ids, token = m.encode_categorical(Xc)
    ids = np.asarray(ids)
    base = _base(m, X, Xc, 0)
    assert np.asarray(m.predict_continue_encoded(X, ids, token, base, 0, 1)).tobytes() == _chain(m, X, Xc, 0, 1).tobytes()
    refused = False
    for _ in range(40):
        G = rng.standard_normal((512, D)).astype(np.float32) + (Xc[:, :1] == tokens20[rng.integers(0, 20)]) * 4.0
        m.step(X, Xc, np.ascontiguousarray(G.astype(np.float32)))
        _, t2 = m.encode_categorical(Xc[:8])
        if t2 != token:
            with pytest.raises(RuntimeError, match="another category dictionary"):
                m.predict_continue_encoded(X, ids, token, base, 0, 1)
            refused = True
            break
    assert refused, "the dictionary never grew in 40 steps on 20 tokens x 2 columns"


def test_optimizers_rates_follow_the_absolute_tree_index():
    F, D, T = 16, 5, 24
    rng = np.random.default_rng(21)
    opts = [dict(algo="SGD", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=4, stop_lr=0.01, T=50),
            dict(algo="SGD", scheduler="Const", init_lr=0.05, start_idx=4, stop_idx=5)]
    m = _model(F, 0, D, 4, opts=opts)
    _grow(m, rng, T, F, 0, D)
    for n in (65, 4099):
        X, _ = _batch(rng, n, F, 0)
        for a in (1, 20):
            _split_check(m, X, None, a, T)
    # optimizers that cover outputs 0..2 of 4: output 3 comes back equal to base, whatever its bits
    D = 4
    m = _model(F, 0, D, 4, opts=[dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2),
                                 dict(algo="SGD", scheduler="Linear", init_lr=0.2, start_idx=2, stop_idx=3, stop_lr=0.02, T=30)])
    _grow(m, rng, 12, F, 0, D)
    for n in (65, 1000):
        X, _ = _batch(rng, n, F, 0)
        for a in (1, 7):
            base, got = _split_check(m, X, None, a, 12)
            assert got[:, 3].tobytes() == base[:, 3].tobytes()
        base = rng.standard_normal((n, D)).astype(np.float32)
        base[::3, 3] = -0.0
        base[1::3, 3] = np.float32("inf")
        got = _continue_both(m, X, None, base, 2, 12)
        assert got[:, 3].tobytes() == base[:, 3].tobytes()
        assert not np.array_equal(got[:, :3], base[:, :3])


def _depth0_model(policy, where, rng, F=4, D=2):
    """A depth-0 tree among normal ones, grown as tests/test_gpu_edges.py grows it: min_data_in_leaf = 60, so a step on 300 rows splits and a
    step on 100 rows cannot (no candidate leaves 60 rows on either side) and appends a single depth-0 leaf.  where = "middle": 3 trees, the
    depth-0 tree, 2 trees; "last": 3 trees, then two depth-0 trees.  A greedy depth-0 leaf never passes (Q7): the search of that tree runs on
    into the leaves of the following trees, and off the ensemble when there are none.  Returns (model, T)."""
    plan = {"middle": (300, 300, 300, 100, 300, 300), "last": (300, 300, 300, 100, 100)}[where]
    m = _model(F, 0, D, 3, policy=policy, min_data_in_leaf=60)
    for rows in plan:
        _grow(m, rng, 1, F, 0, D, rows=rows)
    T = len(plan)
    assert m.get_num_trees() == T
    e = m.get_ensemble_data()
    ti = np.asarray(e["tree_indices"]); dep = np.asarray(e["depths"])
    ends = np.append(ti[1:], np.asarray(e["values"]).shape[0])
    depths = [int(dep[t]) if policy == "oblivious" else int(dep[ti[t]:ends[t]].max()) for t in range(T)]
    assert [d == 0 for d in depths] == [rows == 100 for rows in plan], depths
    return m, T


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("where", ["middle", "last"])
def test_split_anywhere_around_a_depth0_tree(where, policy):
    """Every split point k in 0 .. T: continue(chain over [0, k), k, T) has the bits of the chain over [0, T), through both kernels."""
    rng = np.random.default_rng(61 + (where == "last") + 2 * (policy == "greedy"))
    m, T = _depth0_model(policy, where, rng)
    for n in (65, 200):
        X, _ = _batch(rng, n, 4, 0)
        for k in range(T + 1):
            _split_check(m, X, None, k, T)


def test_never_sliced():
    """300 trees: 3000 rows lie in predict's 128 .. 2048-tree slice window, 15 rows take its chain path; predict_continue is one chain at both."""
    F, D, T = 16, 3, 300
    rng = np.random.default_rng(31)
    m = _model(F, 0, D, 3)
    _grow(m, rng, T, F, 0, D, rows=256)
    for n in (3000, 15):
        X, _ = _batch(rng, n, F, 0)
        got = _continue_both(m, X, None, _bias_base(m, n), 0, T)
        assert got.tobytes() == _chain(m, X, None, 0, T).tobytes()
        for a, b in ((1, 299), (128, 300), (63, 65)):
            got = _continue_both(m, X, None, _chain(m, X, None, 0, a), a, b)
            assert got.tobytes() == _chain(m, X, None, 0, b).tobytes(), (n, a, b)


def test_fallback_shape_more_than_64_outputs():
    F, D, T, n = 16, 70, 10, 200
    rng = np.random.default_rng(41)
    m = _model(F, 0, D, 4)
    _grow(m, rng, T, F, 0, D)
    X, _ = _batch(rng, n, F, 0)
    for a in (0, 1, 7, 9, 10):
        _split_check(m, X, None, a, T)


def test_arguments():
    import torch
    F, D, T, n = 16, 3, 5, 300
    rng = np.random.default_rng(51)
    m = _model(F, 0, D, 3)
    _grow(m, rng, T, F, 0, D)
    X, _ = _batch(rng, n, F, 0)
    base = _chain(m, X, None, 0, 2)
    for a, b in ((0, T + 1), (4, 3), (T + 1, 0), (-1, 3), (1, -2)):
        with pytest.raises(RuntimeError, match="invalid tree range"):
            m.predict_continue(X, None, base, a, b)
    with pytest.raises(RuntimeError, match="Expected base of shape"):
        m.predict_continue(X, None, base[:-1], 2, T)
    with pytest.raises(RuntimeError, match="Expected base of shape"):
        m.predict_continue(X, None, np.ascontiguousarray(base[:, :2]), 2, T)
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.predict_continue(X, None, base.astype(np.float64), 2, T)
    with pytest.raises(RuntimeError, match="without base"):
        m.predict_continue(X, None, None, 2, T)
    dev = torch.device("cuda:0")
    tb = torch.from_numpy(base).to(dev)
    with pytest.raises(RuntimeError, match="torch.float32"):
        m.predict_continue(X, None, (tb.data_ptr(), tuple(tb.shape), "torch.float64", "cuda"), 2, T)
    # a NumPy base is not modified, and in place on the device equals the out-of-place result
    keep = base.copy()
    got = np.asarray(m.predict_continue(X, None, base, 2, T))
    assert base.tobytes() == keep.tobytes()
    assert got.tobytes() == _chain(m, X, None, 0, T).tobytes()
    assert m.predict_continue(X, None, (tb.data_ptr(), tuple(tb.shape), "torch.float32", "cuda"), 2, T) is None
    assert tb.cpu().numpy().tobytes() == got.tobytes()
    # start == stop returns the base
    assert np.asarray(m.predict_continue(X, None, base, 3, 3)).tobytes() == base.tobytes()
