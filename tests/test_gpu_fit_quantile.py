"""fit_prepared(objective="quantile") on the GPU (include/gbrl_hip.h, "Quantile regression").  tests/test_gpu_quantile.py holds one tree's leaf quantiles
to the host rule; here
  1. the fit is byte for byte -- the saved model file, the loss, valid_loss -- the loop objective_gradient -> step_prepared -> quantile_leaves_prepared ->
     predict_continue_prepared written from the public pieces, through both kernel paths: a fresh model, a warm start, batches, row and column
     sampling, a validation set with early stopping;
  2. the same with leaf_update="gradient" against its loop (without the leaf call), one-side sampling among the cases;
  3. a fresh model's bias is the k-th smallest target of every column, k = gbrl_cpp.quantile_rank(n, alpha_d), also where a block of the count pass takes several chunks;
  4. two runs give the same bytes;
  5. at batch_size = n without sampling the loss after 10 trees is strictly below the loss of the bias alone;
  6. what is refused leaves the model as it was: a fresh model, and a warm start whose targets hold a NaN or an infinity.
"""
import os

import numpy as np
import pytest

import gbrl_amd
import quantile_cases as Q   # tests/golden (conftest.py puts it on the path)

pytestmark = pytest.mark.gpu

cpp = gbrl_amd.gbrl_cpp
f32 = np.float32


def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=3, n_bins=32, batch_size=5000):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _same_bits(a, b):
    return f32(a).tobytes() == f32(b).tobytes()


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


def _batches(n, bs, iterations):
    start = 0
    for _ in range(iterations):
        bn = bs if start + bs < n else n - start
        yield start, bn
        start += bn
        if start >= n:
            start = 0


_DATA = {}


def _data(n, F, D, seed):
    """observations and targets y = f(x) + sigma(x) * noise per output, a quarter of them rounded to halves (ties)"""
    if (n, F, D, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, F)).astype(f32)
        W = rng.standard_normal((F, D)).astype(f32)
        y = (X @ W + (0.5 + np.abs(X[:, :1])) * rng.standard_normal((n, D))).astype(f32)
        tie = rng.random((n, D)) < 0.25
        y[tie] = (np.round(y[tie] * 2) / 2).astype(f32)
        _DATA[(n, F, D, seed)] = (X, _shape(y, D))
    return _DATA[(n, F, D, seed)]


def _levels(D):
    return np.array([0.05, 0.5, 0.95], f32) if D == 3 else np.linspace(0.1, 0.9, D).astype(f32)


def _tiled(bias, n, D):
    return _shape(np.tile(np.asarray(bias, f32).reshape(1, D), (n, 1)), D)


def _manual_loop(m, ds, T, alpha, D, bs, iterations, bias, leaf, subsample=1.0, colsample=1.0, seed=0, goss=None, watch=None):
    """the held prediction advanced by predict_continue_prepared, objective_gradient, the draw, step_prepared, then (leaf == 'quantile')
    quantile_leaves_prepared on the rows the tree was grown on at the held prediction of those rows.  watch = (dsv, Tv, rounds): the validation
    losses per iteration by objective_gradient and the stopping rule.  Returns (loss, valid losses)"""
    n = ds.n_rows
    if bias is not None:
        m.set_bias(np.asarray(bias, f32))
    P = _tiled(m.get_bias(), n, D)
    T0 = m.get_num_trees()
    through = {}
    def advance(start, bn):
        sl = slice(start, start + bn)
        a, Tn = through.get(start, 0), m.get_num_trees()
        if a < Tn:
            whole = None if bn == n else np.arange(start, start + bn, dtype=np.int32)
            P[sl] = np.asarray(m.predict_continue_prepared(ds, np.ascontiguousarray(P[sl]), a, Tn, rows=whole))
        through[start] = Tn
    curve = []
    def evaluate():
        dsv, Tv, _ = watch
        base = _tiled(m.get_bias(), dsv.n_rows, D)
        Pv = base if m.get_num_trees() == 0 else np.asarray(m.predict_continue_prepared(dsv, base, 0, m.get_num_trees()))
        curve.append(m.objective_gradient(np.ascontiguousarray(Pv), Tv, "quantile", alpha=alpha)[1])
    if watch:
        evaluate()
    for start, bn in _batches(n, bs, iterations):
        sl = slice(start, start + bn)
        draw = m.get_num_trees()
        advance(start, bn)
        G, _ = m.objective_gradient(np.ascontiguousarray(P[sl]), np.ascontiguousarray(T[sl]), "quantile", alpha=alpha)
        rows = None if bn == n else np.arange(start, start + bn, dtype=np.int32)
        kw = {}
        if subsample < 1.0:
            import torch
            idx = torch.from_dlpack(ds.sample_rows(subsample, seed=seed, draw=draw, start=start, stop=start + bn)).cpu().numpy()
            if idx.size:
                rows, G = idx.astype(np.int32), np.ascontiguousarray(G[idx - start])
        if goss is not None:
            r = ds.sample_goss(np.ascontiguousarray(G), goss[0], goss[1], seed=seed, draw=draw, start=start, stop=start + bn)
            if r["rows"].size:
                rows, G = r["rows"], r["grads"]
        if colsample < 1.0:
            kw["cols"] = ds.sample_cols(colsample, seed=seed, draw=draw)
        m.step_prepared(ds, G, rows=rows, **kw)
        if leaf == "quantile":
            pred, tar = (P, T) if rows is None else (np.ascontiguousarray(P[rows]), np.ascontiguousarray(T[rows]))
            m.quantile_leaves_prepared(ds, pred, tar, alpha, rows=rows)
        if watch:
            evaluate()
            best = int(np.argmin(curve))   # (the first minimum: min_delta = 0 improves on a strictly smaller loss only)
            if watch[2] > 0 and len(curve) - 1 - best >= watch[2]:
                break
    for b0 in range(0, n, bs):
        advance(b0, min(bs, n - b0))
    assert m.get_num_trees() >= T0
    return m.objective_gradient(P, T, "quantile", alpha=alpha)[1], np.asarray(curve, np.float64)


# ---- 1. and 2. the loop a caller could write ------------------------------------------------------------------------------------------------------------
N, F, DEPTH, ITER = 300, 17, 3, 6
LOOPS = [dict(bs=N), dict(bs=128), dict(bs=N, subsample=0.5, seed=11), dict(bs=N, colsample=0.5, seed=5)]


@pytest.mark.parametrize("leaf", ["quantile", "gradient"])
@pytest.mark.parametrize("policy,score,gen,D", [("oblivious", "L2", "Quantile", 3), ("greedy", "Cosine", "Uniform", 4)])
@pytest.mark.parametrize("loop", LOOPS, ids=["whole", "batches", "subsample", "colsample"])
def test_quantile_fit_is_the_loop_a_caller_could_write(loop, policy, score, gen, D, leaf, tmp_path):
    X, T = _data(N, F, D, seed=N + F + D)
    alpha = _levels(D)
    bs = loop["bs"]
    opts = {k: v for k, v in loop.items() if k != "bs"}
    files = []
    for generic in ("0", "1"):   # the select path with the streaming walks, the sort path with the general ones: the same bytes
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            a = _model(F, D, policy=policy, score=score, gen=gen, depth=DEPTH, batch_size=bs)
            ds = a.prepare_dataset(X)
            loss_a = a.fit_prepared(ds, T, ITER, objective="quantile", alpha=alpha, leaf_update=leaf, **opts)   # a fresh model
            assert isinstance(loss_a, float) and a.get_num_trees() == ITER
            b = _model(F, D, policy=policy, score=score, gen=gen, depth=DEPTH, batch_size=bs)
            loss_b, _ = _manual_loop(b, ds, T, alpha, D, bs, ITER, np.asarray(a.get_bias(), f32), leaf, **opts)
            assert _file(a, tmp_path) == _file(b, tmp_path), "generic = %s: the saved files differ" % generic
            assert _same_bits(loss_a, loss_b), (loss_a, loss_b)
            files.append((_file(a, tmp_path), loss_a))
    assert files[0][0] == files[1][0] and _same_bits(files[0][1], files[1][1])
    # and the two leaf rules are two models
    other = "gradient" if leaf == "quantile" else "quantile"
    c = _model(F, D, policy=policy, score=score, gen=gen, depth=DEPTH, batch_size=bs)
    c.fit_prepared(c.prepare_dataset(X), T, ITER, objective="quantile", alpha=alpha, leaf_update=other, **opts)
    assert _file(c, tmp_path) != files[0][0]


@pytest.mark.parametrize("leaf", ["quantile", "gradient"])
def test_a_warm_start_continues(leaf, tmp_path):
    """3 + 3 at batch_size = n is the run of 6, and the second call is its loop from the three trees on"""
    D = 3
    X, T = _data(N, F, D, seed=N + F + D)
    alpha = _levels(D)
    kw = dict(objective="quantile", alpha=alpha, leaf_update=leaf)
    c = _model(F, D, batch_size=N)
    ds = c.prepare_dataset(X)
    c.fit_prepared(ds, T, 3, **kw)
    e = gbrl_amd.GBRL(c)   # a copy of the three trees for the hand loop
    loss_c = c.fit_prepared(ds, T, 3, **kw)
    d = _model(F, D, batch_size=N)
    loss_d = d.fit_prepared(ds, T, 6, **kw)
    assert _file(c, tmp_path) == _file(d, tmp_path) and _same_bits(loss_c, loss_d)
    loss_e, _ = _manual_loop(e, ds, T, alpha, D, N, 3, None, leaf)
    assert _file(e, tmp_path) == _file(c, tmp_path) and _same_bits(loss_e, loss_c)


def test_gradient_leaves_with_goss_are_their_loop(tmp_path):
    D = 3
    X, T = _data(N, F, D, seed=N + F + D)
    alpha = _levels(D)
    a = _model(F, D, batch_size=N)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, T, ITER, objective="quantile", alpha=alpha, goss=(0.2, 0.3), seed=9)
    b = _model(F, D, batch_size=N)
    loss_b, _ = _manual_loop(b, ds, T, alpha, D, N, ITER, np.asarray(a.get_bias(), f32), "gradient", goss=(0.2, 0.3), seed=9)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)


@pytest.mark.parametrize("generic", ["0", "1"])   # the loss tail of the streaming walk and of the general one
@pytest.mark.parametrize("leaf", ["quantile", "gradient"])
@pytest.mark.parametrize("rounds", [0, 2])
def test_validation_and_early_stopping(rounds, leaf, generic, tmp_path):
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        _validation_and_early_stopping(rounds, leaf, tmp_path)


def _validation_and_early_stopping(rounds, leaf, tmp_path):
    D, nv, iterations = 3, 130, 12
    Xa, Ta = _data(N + nv, F, D, seed=41)
    X, T, Xv, Tv = Xa[:N], np.ascontiguousarray(Ta[:N]), Xa[N:], np.ascontiguousarray(Ta[N:])
    alpha = _levels(D)
    m = _model(F, D, batch_size=N)
    ds = m.prepare_dataset(X)
    dsv = m.prepare_dataset(Xv, reference=ds)
    r = m.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, early_stopping_rounds=rounds, objective="quantile", alpha=alpha, leaf_update=leaf)
    assert sorted(r) == ["best_n_trees", "iterations", "loss", "valid_loss"] and r["valid_loss"].shape == (r["iterations"] + 1,)
    b = _model(F, D, batch_size=N)
    loss_b, curve = _manual_loop(b, ds, T, alpha, D, N, iterations, np.asarray(m.get_bias(), f32), leaf, watch=(dsv, Tv, rounds))
    assert r["iterations"] == len(curve) - 1 == b.get_num_trees() and (rounds > 0 or r["iterations"] == iterations)
    assert r["valid_loss"].tobytes() == curve.tobytes(), (r["valid_loss"], curve)
    assert r["best_n_trees"] == int(np.argmin(curve))
    assert _file(m, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], loss_b)


# ---- 3. the bias --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(200, 1), (300, 3), (4096, 8)])
def test_the_bias_is_the_order_statistic_of_every_column(n, D):
    X, T = _data(n, 9, D, seed=n + D)
    alpha = _levels(D) if D > 1 else np.array([0.3], f32)
    m = _model(9, D, batch_size=n)
    m.fit_prepared(m.prepare_dataset(X), T, 1, objective="quantile", alpha=alpha, leaf_update="quantile")
    y = T.reshape(n, D)
    want = np.array([np.sort(y[:, d])[cpp.quantile_rank(n, float(alpha[d])) - 1] for d in range(D)], f32)
    got = np.asarray(m.get_bias(), f32).reshape(D)
    assert (got + f32(0)).tobytes() == (want + f32(0)).tobytes(), (got, want)   # (+ 0: a zero of either sign is the same bias)


MAX_COUNT_BLOCKS = 32   # kMaxCountBlocks of leaf_quantile.hip: beyond 32 chunks of rows_per_chunk rows a block of the count pass takes a second chunk


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("n", [2049, 65537, 70001])
@pytest.mark.parametrize("draw", ["shared_prefix_ties", "continuous"])
def test_the_bias_where_the_count_pass_takes_more_chunks(draw, n, D):
    """one chunk and a row; 32 chunks and a row (block 0 takes two); 35 chunks (three blocks take two).  The ties are 40 targets that share
    their upper 16 bits (tests/golden/quantile_cases.py): the last two digits decide"""
    R = cpp.leaf_quantile_geometry()["rows_per_chunk"]
    assert n > R and (n == 2049 or n > MAX_COUNT_BLOCKS * R)
    X, T = _data(n, 9, D, seed=n + D)
    if draw == "shared_prefix_ties":
        T = _shape(Q.values("shared_prefix_ties", n, D, seed=n), D)
        assert all(len(np.unique(T.reshape(n, D)[:, d])) == Q.TIE_KEYS for d in range(D))
    else:   # the last row, alone in its chunk at 2049 and 65537, is the smallest target of every column: without it every rank moves
        T = T.copy()
        T[-1] = T.min(axis=0) - f32(1)
    alpha = _levels(D) if D > 1 else np.array([0.3], f32)
    m = _model(9, D, batch_size=n)
    m.fit_prepared(m.prepare_dataset(X), T, 1, objective="quantile", alpha=alpha, leaf_update="quantile")
    y = T.reshape(n, D)
    want = np.array([np.sort(y[:, d])[cpp.quantile_rank(n, float(alpha[d])) - 1] for d in range(D)], f32)
    got = np.asarray(m.get_bias(), f32).reshape(D)
    assert (got + f32(0)).tobytes() == (want + f32(0)).tobytes(), (got, want)


# ---- 4. reproducible ----------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(tmp_path):
    D = 3
    X, T = _data(N, F, D, seed=N + F + D)
    kw = dict(objective="quantile", alpha=_levels(D), leaf_update="quantile", subsample=0.7, colsample=0.8, seed=3)
    a = _model(F, D, batch_size=128)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, T, 6, **kw)
    b = _model(F, D, batch_size=128)
    loss_b = b.fit_prepared(ds, T, 6, **kw)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)


# ---- 5. the point of it -------------------------------------------------------------------------------------------------------------------------------
def test_ten_trees_are_strictly_below_the_bias_alone():
    """every leaf moves toward a minimiser of its convex pinball sum by a tenth of the way: the training loss falls"""
    n, D = 4096, 3
    X, T = _data(n, 9, D, seed=77)
    alpha = _levels(D)
    m = _model(9, D, batch_size=n)
    ds = m.prepare_dataset(X)
    start = m.fit_prepared(ds, T, 0, objective="quantile", alpha=alpha, leaf_update="quantile")
    _, loss0 = m.objective_gradient(_tiled(m.get_bias(), n, D), T, "quantile", alpha=alpha)
    assert _same_bits(start, loss0)
    loss10 = m.fit_prepared(ds, T, 10, objective="quantile", alpha=alpha, leaf_update="quantile")
    print("pinball loss: bias alone %.6f, after 10 trees %.6f" % (start, loss10))
    assert loss10 < start


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_as_it_was(tmp_path):
    D = 3
    X, T = _data(N, F, D, seed=N + F + D)
    m = _model(F, D, batch_size=N)
    ds = m.prepare_dataset(X)
    keep = _file(m, tmp_path)
    w = np.ones(N, f32)
    nan = T.copy(); nan[299, 2] = np.nan
    inf = T.copy(); inf[0, 0] = np.inf
    a = _levels(D)
    cases = [
        (T, dict(objective="quantile"), "needs alpha"),
        (T, dict(objective="rmse", alpha=a), "alpha"),
        (T, dict(objective="quantile", alpha=[0.5, 0.5, 1.0]), r"alpha\[2\]"),
        (T, dict(objective="quantile", alpha=[0.5, 0.5]), "one level per output"),
        (T, dict(objective="rmse", leaf_update="quantile"), "quantile leaf values"),
        (T, dict(objective="quantile", alpha=a, leaf_update="newton"), "hessian is zero"),
        (T, dict(objective="quantile", alpha=a, weights=w), "weights"),
        (T, dict(objective="quantile", alpha=a, valid=ds, valid_targets=T, valid_weights=w), "weights"),
        (T, dict(objective="quantile", alpha=a, valid=ds, valid_targets=T, eval_metric="error"), "metric"),
        (T, dict(objective="quantile", alpha=a, leaf_update="quantile", goss=(0.2, 0.2)), "goss"),
        (nan, dict(objective="quantile", alpha=a, leaf_update="quantile"), "not finite"),
        (inf, dict(objective="quantile", alpha=a), "not finite"),
    ]
    for Tn, kw, what in cases:
        with pytest.raises(RuntimeError, match=what):
            m.fit_prepared(ds, Tn, 2, **kw)
        assert _file(m, tmp_path) == keep and m.get_num_trees() == 0
    assert m.fit_prepared(ds, T, 1, objective="quantile", alpha=a, leaf_update="quantile") > 0.0 and m.get_num_trees() == 1


@pytest.mark.parametrize("leaf", ["quantile", "gradient"])
@pytest.mark.parametrize("generic", ["0", "1"])
def test_a_warm_start_refuses_a_target_that_is_not_finite(generic, leaf, tmp_path):
    """a model with trees: the targets are checked before the first step, so no tree is appended and the file keeps its bytes"""
    D = 3
    X, T = _data(N, F, D, seed=N + F + D)
    a = _levels(D)
    m = _model(F, D, batch_size=N)
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, T, 2, objective="quantile", alpha=a, leaf_update=leaf)
    keep = _file(m, tmp_path)
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        for row, col, v in ((299, 2, np.nan), (0, 0, np.inf), (150, 1, -np.inf)):
            bad = T.copy(); bad[row, col] = v
            with pytest.raises(RuntimeError, match="not finite"):
                m.fit_prepared(ds, bad, 2, objective="quantile", alpha=a, leaf_update=leaf)
            assert m.get_num_trees() == 2 and _file(m, tmp_path) == keep
        m.fit_prepared(ds, T, 1, objective="quantile", alpha=a, leaf_update=leaf)
    assert m.get_num_trees() == 3
