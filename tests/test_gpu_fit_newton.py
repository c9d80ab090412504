"""fit_prepared(leaf_update="newton") on the GPU (include/gbrl_hip.h, "Newton leaf values").  tests/test_gpu_newton.py holds one tree's sums and values
to NumPy; here
  1. the fit is byte for byte -- the saved model file, the loss -- the loop objective_gradient -> step_prepared -> newton_leaves_prepared ->
     predict_continue_prepared written from the public pieces, through both code-walk kernels, with batches, row and column sampling;
  2. valid_loss[k] is objective_gradient's loss of the finished model's first T0 + k trees, bit for bit;
  3. leaf_update="gradient" is the call without the keyword, and the older C spelling still gives that model;
  4. two runs give the same bytes; a warm start of 3 + 3 iterations is the run of 6;
  5. what is refused leaves the model as it was;
  6. on a noisy linear rule, 20 newton trees reach a lower validation loss than 20 gradient trees (profiles/newton.txt has both curves).
"""
import ctypes as C
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu


def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=3, n_bins=32, batch_size=5000):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
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
    return np.float32(a).tobytes() == np.float32(b).tobytes()


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
    """observations, labels = the arg-max of D noisy linear functions, and their one-hot matrix"""
    if (n, F, D, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, F)).astype(np.float32)
        W = rng.standard_normal((F, max(D, 2))).astype(np.float32)
        y = np.argmax(X @ W + 0.5 * rng.standard_normal((n, max(D, 2))), axis=1).astype(np.int32)
        onehot = (y[:, None] == np.arange(D)[None, :]).astype(np.float32)   # (D == 1: class 0 against the rest)
        _DATA[(n, F, D, seed)] = (X, y, onehot)
    return _DATA[(n, F, D, seed)]


def _targets(obj, y, onehot, D):
    return y if obj == "softmax" else _shape(onehot, D)


def _tiled(bias, n, D):
    return _shape(np.tile(np.asarray(bias, np.float32).reshape(1, D), (n, 1)), D)


def _manual_loop(m, ds, T, obj, D, bs, iterations, bias, leaf_l2, subsample=1.0, colsample=1.0, seed=0):
    """the held prediction advanced by predict_continue_prepared, objective_gradient, step_prepared, then newton_leaves_prepared on the rows the
    tree was grown on at the held prediction of those rows; returns the loss"""
    n = ds.n_rows
    if bias is not None:
        m.set_bias(np.asarray(bias, np.float32))
    P = _tiled(m.get_bias(), n, D)
    through = {}
    def advance(start, bn):
        sl = slice(start, start + bn)
        a, Tn = through.get(start, 0), m.get_num_trees()
        if a < Tn:
            whole = None if bn == n else np.arange(start, start + bn, dtype=np.int32)
            P[sl] = np.asarray(m.predict_continue_prepared(ds, np.ascontiguousarray(P[sl]), a, Tn, rows=whole))
        through[start] = Tn
    for start, bn in _batches(n, bs, iterations):
        sl = slice(start, start + bn)
        draw = m.get_num_trees()
        advance(start, bn)
        G, _ = m.objective_gradient(np.ascontiguousarray(P[sl]), np.ascontiguousarray(T[sl]), obj)
        rows = None if bn == n else np.arange(start, start + bn, dtype=np.int32)
        kw = {}
        if subsample < 1.0:
            import torch
            idx = torch.from_dlpack(ds.sample_rows(subsample, seed=seed, draw=draw, start=start, stop=start + bn)).cpu().numpy()
            if idx.size:
                rows, G = idx.astype(np.int32), np.ascontiguousarray(G[idx - start])
        if colsample < 1.0:
            kw["cols"] = ds.sample_cols(colsample, seed=seed, draw=draw)
        m.step_prepared(ds, G, rows=rows, **kw)
        pred, tar = (P, T) if rows is None else (np.ascontiguousarray(P[rows]), np.ascontiguousarray(T[rows]))
        m.newton_leaves_prepared(ds, pred, tar, obj, leaf_l2=leaf_l2, rows=rows)
    for b0 in range(0, n, bs):
        advance(b0, min(bs, n - b0))
    _, loss = m.objective_gradient(P, T, obj)
    return loss


# ---- 1. the loop a caller could write ---------------------------------------------------------------------------------------------------------------
N, F, DEPTH, ITER = 300, 17, 3, 6
LOOPS = [dict(bs=N), dict(bs=128), dict(bs=N, subsample=0.5, seed=11), dict(bs=N, colsample=0.5, seed=5)]


@pytest.mark.parametrize("obj,D", [("logistic", 3), ("softmax", 4)])
@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("loop", LOOPS, ids=["whole", "batches", "subsample", "colsample"])
def test_newton_fit_is_the_loop_a_caller_could_write(loop, policy, score, gen, obj, D, tmp_path):
    X, y, onehot = _data(N, F, D, seed=N + F + D)
    T = _targets(obj, y, onehot, D)
    bs = loop["bs"]
    opts = {k: v for k, v in loop.items() if k != "bs"}
    leaf_l2 = 1.0 if obj == "logistic" else 0.5
    files = []
    for generic in ("0", "1"):   # the streaming kernels and the general ones: the same bytes
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            a = _model(F, D, policy=policy, score=score, gen=gen, depth=DEPTH, batch_size=bs)
            ds = a.prepare_dataset(X)
            loss_a = a.fit_prepared(ds, T, ITER, objective=obj, leaf_update="newton", leaf_l2=leaf_l2, **opts)
            assert isinstance(loss_a, float) and a.get_num_trees() == ITER
            b = _model(F, D, policy=policy, score=score, gen=gen, depth=DEPTH, batch_size=bs)
            loss_b = _manual_loop(b, ds, T, obj, D, bs, ITER, np.asarray(a.get_bias(), np.float32), leaf_l2, **opts)
            assert _file(a, tmp_path) == _file(b, tmp_path), "generic = %s: the saved files differ" % generic
            assert _same_bits(loss_a, loss_b), (loss_a, loss_b)
            files.append((_file(a, tmp_path), loss_a))
    assert files[0][0] == files[1][0] and _same_bits(files[0][1], files[1][1])
    # and it is not the gradient fit
    c = _model(F, D, policy=policy, score=score, gen=gen, depth=DEPTH, batch_size=bs)
    c.fit_prepared(c.prepare_dataset(X), T, ITER, objective=obj, **opts)
    assert _file(c, tmp_path) != files[0][0]


# ---- 2. validation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj,D", [("logistic", 3), ("softmax", 4)])
def test_valid_loss_is_the_loss_of_every_prefix(obj, D, tmp_path):
    nv = 130
    Xa, ya, onehota = _data(N + nv, F, D, seed=41)
    X, y, onehot, Xv, yv, onehotv = Xa[:N], ya[:N], onehota[:N], Xa[N:], ya[N:], onehota[N:]
    T, Tv = _targets(obj, y, onehot, D), _targets(obj, yv, onehotv, D)
    m = _model(F, D, batch_size=N)
    ds = m.prepare_dataset(X)
    dsv = m.prepare_dataset(Xv, reference=ds)
    r = m.fit_prepared(ds, T, ITER, valid=dsv, valid_targets=Tv, objective=obj, leaf_update="newton")
    assert r["iterations"] == ITER and r["valid_loss"].shape == (ITER + 1,)
    base = _tiled(m.get_bias(), nv, D)
    for k, got in enumerate(r["valid_loss"]):
        P = base if k == 0 else np.asarray(m.predict_continue_prepared(dsv, base, 0, k))
        _, want = m.objective_gradient(np.ascontiguousarray(P), Tv, obj)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_loss[%d] = %r, objective_gradient's loss %r" % (k, got, want)
    # the model is the one the call without a validation set leaves, and predict on the observations reads the same values
    b = _model(F, D, batch_size=N)
    loss_b = b.fit_prepared(ds, T, ITER, objective=obj, leaf_update="newton")
    assert _file(m, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], loss_b)
    want = np.asarray(m.predict_continue_prepared(dsv, base, 0, ITER))
    assert np.asarray(m.predict(Xv, None)).tobytes() == want.tobytes()


# ---- 3. gradient is the call without the keyword; the older spelling ---------------------------------------------------------------------------------
def test_gradient_is_the_call_without_the_keyword(tmp_path):
    D, obj = 3, "logistic"
    X, y, onehot = _data(N, F, D, seed=N + F + D)
    T = _targets(obj, y, onehot, D)
    a = _model(F, D, batch_size=128)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, T, ITER, objective=obj)
    b = _model(F, D, batch_size=128)
    loss_b = b.fit_prepared(ds, T, ITER, objective=obj, leaf_update="gradient", leaf_l2=3.0)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)
    # gbrl_hip_fit_prepared_metric has no leaf arguments: the gradient model
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    vp, ci, d, u64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    lib.gbrl_hip_fit_prepared_metric.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, d, d, d, u64, ci, ci, vp, vp, vp, vp, vp]
    lib.gbrl_hip_fit_prepared_leaf.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, d, d, d, u64, ci, ci, ci, d, vp, vp, vp, vp, vp]
    c = _model(F, D, batch_size=128)
    loss, done = C.c_float(np.nan), C.c_int(-7)
    Tc = np.ascontiguousarray(T, np.float32)
    assert lib.gbrl_hip_fit_prepared_metric(c._handle(), ds._handle(), Tc.ctypes.data, 0, ITER, None, None, 0, 0, 0.0, 1.0, 1.0, 0, 1, 0, C.byref(loss), None, None,
                                            C.byref(done), None) == 0
    assert _file(c, tmp_path) == _file(a, tmp_path) and _same_bits(loss.value, loss_a) and done.value == ITER
    # ... and gbrl_hip_fit_prepared_leaf with newton is the Python call
    e = _model(F, D, batch_size=128)
    assert lib.gbrl_hip_fit_prepared_leaf(e._handle(), ds._handle(), Tc.ctypes.data, 0, ITER, None, None, 0, 0, 0.0, 1.0, 1.0, 0, 1, 0, 1, 0.5, C.byref(loss), None, None,
                                          C.byref(done), None) == 0
    f = _model(F, D, batch_size=128)
    loss_f = f.fit_prepared(ds, T, ITER, objective=obj, leaf_update="newton", leaf_l2=0.5)
    assert _file(e, tmp_path) == _file(f, tmp_path) and _same_bits(loss.value, loss_f)
    assert _file(e, tmp_path) != _file(a, tmp_path)


# ---- 4. reproducible; a warm start continues ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj,D", [("logistic", 3), ("softmax", 4)])
def test_two_runs_and_a_warm_start(obj, D, tmp_path):
    X, y, onehot = _data(N, F, D, seed=N + F + D)
    T = _targets(obj, y, onehot, D)
    kw = dict(objective=obj, leaf_update="newton", subsample=0.7, seed=3)
    a = _model(F, D, batch_size=128)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, T, 6, **kw)
    b = _model(F, D, batch_size=128)
    loss_b = b.fit_prepared(ds, T, 6, **kw)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)
    # 3 + 3 at batch_size = n (a warm start begins at row 0 again, as a run of 6 whole-data iterations does)
    kw = dict(objective=obj, leaf_update="newton")
    c = _model(F, D, batch_size=N)
    c.fit_prepared(ds, T, 3, **kw)
    loss_c = c.fit_prepared(ds, T, 3, **kw)
    d = _model(F, D, batch_size=N)
    loss_d = d.fit_prepared(ds, T, 6, **kw)
    assert _file(c, tmp_path) == _file(d, tmp_path) and _same_bits(loss_c, loss_d)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_as_it_was(tmp_path):
    D = 3
    X, y, onehot = _data(N, F, D, seed=N + F + D)
    m = _model(F, D, batch_size=N)
    ds = m.prepare_dataset(X)
    keep = _file(m, tmp_path)
    bad = onehot.copy(); bad[17, 1] = 1.5
    nan = onehot.copy(); nan[299, 2] = np.nan
    for T, kw, what in ((onehot, dict(objective="rmse", leaf_update="newton"), "rmse"), (onehot, dict(objective="logistic", leaf_update="newton", leaf_l2=-1.0), "leaf_l2"),
                        (onehot, dict(objective="logistic", leaf_update="newton", leaf_l2=float("nan")), "leaf_l2"),
                        (onehot, dict(objective="logistic", leaf_update="hessian"), "leaf_update"), (bad, dict(objective="logistic", leaf_update="newton"), "target"),
                        (nan, dict(objective="logistic", leaf_update="newton"), "target")):
        with pytest.raises(RuntimeError, match=what):
            m.fit_prepared(ds, T, 2, **kw)
        assert _file(m, tmp_path) == keep and m.get_num_trees() == 0
    # a target of 1.5 is the gradient rule's business as before
    m.fit_prepared(ds, bad, 1, objective="logistic")
    assert m.get_num_trees() == 1


# ---- 6. the point of it -----------------------------------------------------------------------------------------------------------------------------
def test_newton_reaches_a_lower_validation_loss_than_gradient():
    n, nv, Fb, iterations = 4096, 1024, 16, 20
    rng = np.random.default_rng(20251)
    X = rng.standard_normal((n + nv, Fb)).astype(np.float32)
    w = rng.standard_normal(Fb).astype(np.float32)
    y = ((X @ w + rng.standard_normal(n + nv).astype(np.float32)) > 0).astype(np.float32)   # a noisy linear rule
    curves = {}
    for rule in ("gradient", "newton"):
        m = _model(Fb, 1, depth=3, n_bins=32, batch_size=n)
        ds = m.prepare_dataset(X[:n])
        dsv = m.prepare_dataset(X[n:], reference=ds)
        r = m.fit_prepared(ds, y[:n], iterations, valid=dsv, valid_targets=y[n:], objective="logistic", leaf_update=rule, leaf_l2=1.0)
        curves[rule] = np.asarray(r["valid_loss"], np.float64)
        print(rule, " ".join("%.6f" % v for v in curves[rule]))
    assert curves["newton"][iterations] < curves["gradient"][iterations]
