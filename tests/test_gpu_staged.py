"""`predict_staged` / `staged_loss` (include/gbrl_hip.h): every ensemble prefix [0, stops[s]) in one walk.

The yardstick is `predict_continue(X, Xc, tiled bias, 0, k)`, which its own tests pin to the general chain and to a NumPy walk: stage s of
`predict_staged` must have ITS BYTES for stops[s] > 0 and the tiled bias for stops[s] == 0.  `staged_loss` is compared with MultiRMSE as
fit() defines it, computed in NumPy (float64, exactly summed) from those stage predictions; the allowed relative error is m * 2**-52 with
m = n * D: summing m non-negative doubles in any order costs at most (m - 1) * 2**-53, the other half covers the division and the square
root.  Every case runs the default path (the streaming kernel k_staged where it takes the shape) and GBRL_HIP_STAGED_GENERIC=1
(k_staged_general) and wants the same bytes from both, predictions and losses, and the same bytes from a second identical call.

Models are grown as tests/test_gpu_predict_continue.py grows them: 256 .. 512-row steps at depth 1 .. 4, 12 .. 20 trees.  Rows 1, 63, 64,
65, 200: a partial block, a full one, a second partial one, several loss partials."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKENS = np.array(["tok%d" % i for i in range(6)], dtype="S128")
ROWS = (1, 63, 64, 65, 200)


def _model(F, Fc, D, depth, policy="oblivious", opts=None, bias=None, device="cpu", batch_size=5000, min_data_in_leaf=0):
    import gbrl_amd
    m = gbrl_amd.GBRL(input_dim=F + Fc, output_dim=D, policy_dim=D, max_depth=depth, min_data_in_leaf=min_data_in_leaf, n_bins=32, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=batch_size, grow_policy=policy,
                      verbose=0, device=device, learner_name="staged")
    m.set_feature_weights(np.ones(F + Fc, np.float32))
    for o in (opts or [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)]):
        m.set_optimizer(**o)
    m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))
    m.set_bias(np.asarray(bias if bias is not None else 0.25 + 0.5 * np.arange(D), np.float32))
    return m


def _batch(rng, n, F, Fc):
    X = rng.standard_normal((n, F)).astype(np.float32) if F else None
    Xc = TOKENS[rng.integers(0, 6, (n, Fc))] if Fc else None
    return X, Xc


def _grow(m, rng, trees, F, Fc, D, rows=256):
    for _ in range(trees):
        X, Xc = _batch(rng, rows, F, Fc)
        G = rng.standard_normal((rows, D)).astype(np.float32)
        if F:
            G[:, 0] += X[:, 0] * 2.0
        if Fc:
            G[:, -1] += (Xc[:, 0] == TOKENS[1]) * 3.0
        m.step(X, Xc, np.ascontiguousarray(G))


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _bias_base(m, n):
    bias = np.asarray(m.get_bias(), np.float32).reshape(-1)
    return np.ascontiguousarray(np.tile(bias, (n, 1))) if bias.size > 1 else np.full(n, bias[0], np.float32)


def _stage_table(m, X, Xc, n, T):
    """want[k] = the yardstick's prediction after k trees, k = 0 .. T (computed once per batch, shared by every stops list)."""
    base = _bias_base(m, n)
    return [base] + [np.asarray(m.predict_continue(X, Xc, base, 0, k)) for k in range(1, T + 1)]


def _rmse(p, y, n):
    g = (np.asarray(p, np.float32) - np.asarray(y, np.float32)).astype(np.float32).astype(np.float64).reshape(-1)
    return math.sqrt(0.5 * math.fsum(g * g) / n)


def _check(m, X, Xc, Y, want, stops, T):
    """both paths, twice each: predictions and losses against the yardstick; returns (predictions, losses) of the default path."""
    n = (X if X is not None else Xc).shape[0]
    D = want[0].shape[1] if want[0].ndim == 2 else 1
    ks = list(range(1, T + 1)) if stops is None else list(stops)
    preds, losses = [], []
    for generic in ("0", "1"):
        with _env("GBRL_HIP_STAGED_GENERIC", generic):
            p = np.asarray(m.predict_staged(X, Xc, stops))
            p2 = np.asarray(m.predict_staged(X, Xc, stops))
            l = m.staged_loss(X, Xc, Y, stops)
            l2 = m.staged_loss(X, Xc, Y, stops=stops)
        assert p.dtype == np.float32 and p.shape == (len(ks),) + want[0].shape, (p.dtype, p.shape)
        assert isinstance(l, np.ndarray) and l.dtype == np.float64 and l.shape == (len(ks),)
        assert p.tobytes() == p2.tobytes() and l.tobytes() == l2.tobytes(), "two identical calls differ (generic=%s)" % generic
        preds.append(p)
        losses.append(l)
    assert preds[0].tobytes() == preds[1].tobytes(), "k_staged and k_staged_general predictions differ, stops=%s" % (ks,)
    assert losses[0].tobytes() == losses[1].tobytes(), "k_staged and k_staged_general losses differ, stops=%s" % (ks,)
    tol = n * D * 2.0 ** -52
    for s, k in enumerate(ks):
        assert preds[0][s].tobytes() == want[k].tobytes(), "stage %d (k = %d) of %s, n = %d" % (s, k, ks, n)
        ref = _rmse(want[k], Y, n)
        rel = abs(losses[0][s] - ref) / ref
        assert rel <= tol, "staged_loss stage %d (k = %d): %r vs %r, rel %.3e > %.3e" % (s, k, losses[0][s], ref, rel, tol)
    return preds[0], losses[0]


def _stops_lists(T):
    return [None, [0, 1, T], [3, 5, 13, T], [7], [T]]


def _sweep(m, rng, F, Fc, D, T, rows=ROWS):
    assert m.get_num_trees() == T
    for n in rows:
        X, Xc = _batch(rng, n, F, Fc)
        Y = rng.standard_normal((n, D) if D > 1 else (n,)).astype(np.float32)
        want = _stage_table(m, X, Xc, n, T)
        for stops in _stops_lists(T):
            _check(m, X, Xc, Y, want, stops, T)


# D crosses every template width of k_staged (kG = 8, 8, 4, 2, 1) and 64 | 65, the boundary to k_staged_general; F = 5: scalar staging of the
# tile, F = 8: 16-byte staging
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("F", [5, 8])
@pytest.mark.parametrize("D", [1, 3, 8, 17, 64, 65, 128])
def test_every_width_both_policies(D, F, policy):
    T = 14
    rng = np.random.default_rng(1000 * D + 10 * F + (policy == "greedy"))
    m = _model(F, 0, D, 3, policy=policy)
    _grow(m, rng, T, F, 0, D)
    _sweep(m, rng, F, 0, D, T)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("F,Fc", [(5, 2), (0, 3)])
def test_categorical_columns(F, Fc, policy):
    T, D = 16, 3
    rng = np.random.default_rng(77 + F + (policy == "greedy"))
    m = _model(F, Fc, D, 4, policy=policy)
    _grow(m, rng, T, F, Fc, D, rows=512)
    assert (np.asarray(m.get_ensemble_data()["is_numerics"]) == 0).any(), "no categorical condition was grown"
    _sweep(m, rng, F, Fc, D, T, rows=(1, 65, 200))


def test_depth_one_and_twenty_trees():
    F, D, T = 8, 3, 20
    rng = np.random.default_rng(5)
    m = _model(F, 0, D, 1)
    _grow(m, rng, T, F, 0, D, rows=384)
    _sweep(m, rng, F, 0, D, T, rows=(65, 200))


def _depth0_model(policy, where, rng, F=4, D=2):
    """tests/test_gpu_predict_continue.py::_depth0_model: min_data_in_leaf = 60, a step on 300 rows splits, a step on 100 rows appends a single
    depth-0 leaf.  where = "middle": 3 trees, the depth-0 tree, 2 trees; "last": 3 trees, then two depth-0 trees.  Returns (model, T)."""
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
def test_checkpoints_around_a_depth0_tree(where, policy):
    """A greedy depth-0 leaf never passes (Q7): the search of that tree runs on into the leaves of the following trees.  With the depth-0 trees
    last, the walk runs off the ensemble at tree 3 and the checkpoints 4 and 5 follow: the suspended walk must stay ended.  Every stage is the
    chain over its prefix (`predict` under GBRL_HIP_PREDICT_GENERIC=1, which is what the yardstick of this file is pinned to), for every tree
    count 0 .. T and for sparse subsets."""
    rng = np.random.default_rng(71 + (where == "last") + 2 * (policy == "greedy"))
    m, T = _depth0_model(policy, where, rng)
    for n in (65, 200):
        X, _ = _batch(rng, n, 4, 0)
        Y = rng.standard_normal((n, 2)).astype(np.float32)
        want = _stage_table(m, X, None, n, T)
        for k in range(1, T + 1):
            with _env("GBRL_HIP_PREDICT_GENERIC", "1"):
                assert want[k].tobytes() == np.asarray(m.predict(X, None, 0, k)).tobytes(), "the yardstick is not the chain over [0, %d)" % k
        for stops in (None, list(range(T + 1)), [0, 2, T], [1, T - 1, T], [T - 1]):
            _check(m, X, None, Y, want, stops, T)


def test_actor_and_critic_rates():
    F, D, T = 8, 8, 14
    rng = np.random.default_rng(21)
    m = _model(F, 0, D, 3, opts=[dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=6),
                                 dict(algo="SGD", scheduler="Const", init_lr=0.03, start_idx=6, stop_idx=8)])
    _grow(m, rng, T, F, 0, D)
    _sweep(m, rng, F, 0, D, T, rows=(65, 200))


def test_an_output_without_an_optimizer_keeps_the_bias_bits():
    F, D, T = 5, 4, 14
    rng = np.random.default_rng(22)
    bias = np.array([0.5, -1.0, 2.0, -0.0], np.float32)
    for policy in ("oblivious", "greedy"):
        m = _model(F, 0, D, 3, policy=policy, bias=bias, opts=[dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=3)])
        _grow(m, rng, T, F, 0, D)
        X, _ = _batch(rng, 200, F, 0)
        Y = rng.standard_normal((200, D)).astype(np.float32)
        want = _stage_table(m, X, None, 200, T)
        p, _ = _check(m, X, None, Y, want, None, T)
        assert p[:, :, 3].tobytes() == np.full((T, 200), -0.0, np.float32).tobytes()       # the sign bit too
        assert not np.array_equal(p[-1][:, :3], np.tile(bias[:3], (200, 1)))
        _check(m, X, None, Y, want, [0, 1, T], T)


def test_linear_schedule_rates_at_the_absolute_tree_index():
    F, D, T = 8, 5, 16
    rng = np.random.default_rng(23)
    opts = [dict(algo="SGD", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=4, stop_lr=0.01, T=50),
            dict(algo="SGD", scheduler="Const", init_lr=0.05, start_idx=4, stop_idx=5)]
    for policy in ("oblivious", "greedy"):
        m = _model(F, 0, D, 3, policy=policy, opts=opts)
        _grow(m, rng, T, F, 0, D)
        _sweep(m, rng, F, 0, D, T, rows=(65, 200))


def test_optimizers_sharing_an_output_take_the_general_kernel():
    F, D, T = 8, 3, 12
    rng = np.random.default_rng(24)
    m = _model(F, 0, D, 3, opts=[dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=3),
                                 dict(algo="SGD", scheduler="Const", init_lr=0.05, start_idx=1, stop_idx=2)])
    _grow(m, rng, T, F, 0, D)
    for n in (65, 200):
        X, _ = _batch(rng, n, F, 0)
        Y = rng.standard_normal((n, D)).astype(np.float32)
        want = _stage_table(m, X, None, n, T)
        for stops in (None, [0, 1, T], [5]):
            _check(m, X, None, Y, want, stops, T)


def test_stops_none_means_every_tree_and_errors_on_a_grown_model():
    F, D, T = 8, 3, 12
    rng = np.random.default_rng(25)
    m = _model(F, 0, D, 3)
    _grow(m, rng, T, F, 0, D)
    X, _ = _batch(rng, 65, F, 0)
    Y = rng.standard_normal((65, D)).astype(np.float32)
    every = list(range(1, T + 1))
    assert np.asarray(m.predict_staged(X, None)).tobytes() == np.asarray(m.predict_staged(X, None, stops=every)).tobytes()
    assert m.staged_loss(X, None, Y).tobytes() == m.staged_loss(X, None, Y, every).tobytes()
    assert np.asarray(m.predict_staged(X, None, np.array(every, np.int64))).shape == (T, 65, D)     # any integer sequence
    for bad, msg in (([], "stops is empty"), ([T + 1], "out of bounds"), ([-1, 2], "out of bounds"), ([2, 2], "strictly ascending"),
                     ([3, 1], "strictly ascending")):
        with pytest.raises(RuntimeError, match=msg):
            m.predict_staged(X, None, bad)
        with pytest.raises(RuntimeError, match=msg):
            m.staged_loss(X, None, Y, bad)
    with pytest.raises(RuntimeError, match="Expected targets of shape"):
        m.staged_loss(X, None, Y[:-1], [T])


def test_the_last_stage_is_the_loss_fit_returns():
    """fit() rounds to float32 three times after the same sum (2**-24 each, about 1.8e-7 together): 1e-6 leaves a factor of five.  Its closing
    evaluation runs the tree-order chain, so the predictions behind the two losses are the same bits."""
    F, D, T, n = 8, 3, 12, 300
    rng = np.random.default_rng(26)
    X, _ = _batch(rng, n, F, 0)
    Y = (np.tanh(X[:, :D]) + 0.1 * rng.standard_normal((n, D))).astype(np.float32)
    m = _model(F, 0, D, 3, batch_size=512)
    loss = float(m.fit(X, None, Y, iterations=T, shuffle=False))
    assert m.get_num_trees() == T
    curve = m.staged_loss(X, None, Y, [0, T])
    assert abs(curve[1] - loss) <= 1e-6 * loss, (curve[1], loss)
    assert curve[1] < curve[0]                                  # the trees fit the data they were grown on
    want = _stage_table(m, X, None, n, T)
    _check(m, X, None, Y, want, [0, T], T)


def test_device_inputs_and_a_cuda_model():
    import torch
    F, D, T, n = 8, 8, 12, 200
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(27)
    m = _model(F, 0, D, 3)
    _grow(m, rng, T, F, 0, D)
    X, _ = _batch(rng, n, F, 0)
    Y = rng.standard_normal((n, D)).astype(np.float32)
    stops = [0, 3, 5, T]
    p = np.asarray(m.predict_staged(X, None, stops))
    l = m.staged_loss(X, None, Y, stops)
    tX, tY = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    assert np.asarray(m.predict_staged(tup(tX), None, stops)).tobytes() == p.tobytes()
    assert m.staged_loss(tup(tX), None, tup(tY), stops).tobytes() == l.tobytes()
    assert m.staged_loss(X, None, tup(tY), stops).tobytes() == l.tobytes()
    # a "cuda" model hands back a DLPack capsule on its device, as predict does; the losses stay a NumPy array
    m.to_device("cuda")
    cap = m.predict_staged(tup(tX), None, stops)
    t = torch.from_dlpack(cap)
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (len(stops), n, D)
    assert t.cpu().numpy().tobytes() == p.tobytes()
    l2 = m.staged_loss(tup(tX), None, tup(tY), stops)
    assert isinstance(l2, np.ndarray) and l2.tobytes() == l.tobytes()
    # D == 1: [len(stops), n], and targets [n]
    m1 = _model(F, 0, 1, 3)
    _grow(m1, rng, T, F, 0, 1)
    y1 = rng.standard_normal(n).astype(np.float32)
    p1 = np.asarray(m1.predict_staged(X, None, stops))
    assert p1.shape == (len(stops), n)
    assert m1.staged_loss(X, None, y1, stops).tobytes() == m1.staged_loss(X, None, y1.reshape(n, 1), stops).tobytes()
