"""The classification objectives on the GPU (GBRL.fit_prepared(objective=), GBRL.objective_gradient; include/gbrl_hip.h, "Classification
objectives").  tests/test_objective_host.py holds gbrl_cpp.objective_gradient_host to the formulas; here
  1. the device gradient is the host gradient byte for byte, and the device loss a float64 NumPy evaluation within the summation bound;
  2. fit_prepared(objective=) is the loop a caller could write from public calls (file bytes, the loss), through both code-walk kernels;
  3. valid_loss[k] is objective_gradient's loss of the first T0 + k trees; early stopping cuts that very run;
  4. the validation loss of the training rows falls strictly; softmax starts at the entropy of the class frequencies;
  5. objective="rmse" is the call without the keyword;
  6. row and column sampling compose with an objective;
  7. what is refused leaves the model as it was.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

host = gbrl_amd.gbrl_cpp.objective_gradient_host


# ---- helpers (tests/test_gpu_fit_prepared.py's) -----------------------------------------------------------------------------------------------------
def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, batch_size=5000):
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


def _dev(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


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
        y = np.minimum(y, max(D, 2) - 1)
        onehot = (y[:, None] == np.arange(D)[None, :]).astype(np.float32)   # (D == 1: class 0 against the rest)
        _DATA[(n, F, D, seed)] = (X, y, onehot)
    return _DATA[(n, F, D, seed)]


def _targets(obj, y, onehot, D):
    return y if obj == "softmax" else _shape(onehot, D)


def _rule_bias(obj, T, n, D):
    """the first-fit bias, restated from the header's text (float64, then one rounding to float32)"""
    if obj == "softmax":
        nc = np.bincount(T, minlength=D).astype(np.float64)
        return np.log(np.maximum(nc, 0.5) / n).astype(np.float32)
    c = np.clip(T.reshape(n, D).astype(np.float64).sum(axis=0) / n, 1.0 / (2 * n), 1.0 - 1.0 / (2 * n))
    return np.log(c / (1.0 - c)).astype(np.float32)


def _tiled(bias, n, D):
    return _shape(np.tile(np.asarray(bias, np.float32).reshape(1, D), (n, 1)), D)


def _loss64(obj, p, t):
    """the loss of the set in float64: the formulas of the header, the terms summed exactly"""
    p = p.reshape(p.shape[0], -1).astype(np.float64)
    with np.errstate(all="ignore"):
        if obj == "softmax":
            m = p.max(axis=1)
            rows = np.log(np.exp(p - m[:, None]).sum(axis=1)) + m - p[np.arange(p.shape[0]), t]
        else:
            y = t.reshape(p.shape).astype(np.float64)
            rows = (np.maximum(p, 0) - y * p + np.log1p(np.exp(-np.abs(p)))).ravel()
    return math.fsum(rows) / p.shape[0] if np.isfinite(rows).all() else float("nan")


# ---- 1. the device gradient is the host gradient ----------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 130, 4097)


def _scores(rng, n, D, specials):
    p = rng.uniform(-8, 8, (n, D)).astype(np.float32)
    p[0] = 1.5                                     # a row of equal scores
    if n > 2:
        p[1, 0] = 0.0; p[2, D - 1] = -0.0
    if specials and n > 8:
        p[3, 0] = np.inf; p[4, D - 1] = -np.inf; p[5, :] = -np.inf; p[5, 0] = 2.0; p[6, D // 2] = np.inf
    if n > 12:                                     # exponentials with a subnormal result, and the last one before +0
        p[7, 0] = -88.0; p[8, D - 1] = -95.5; p[9, 0] = -100.0; p[10, D - 1] = -103.9; p[11, 0] = -104.0; p[12, D - 1] = 88.0
    return p


WIDTHS = [1, 2, 3, 4, 8, 9, 16, 32, 33, 64, 128]   # every DMAX family of the code walk (4 8 16 32 64; 8 32 128), odd widths


@pytest.mark.parametrize("D,obj", [(D, "logistic") for D in WIDTHS] + [(D, "softmax") for D in WIDTHS if D >= 2])
def test_device_gradient_is_the_host_gradient(D, obj):
    """The loss bound (n * D + 8) * 2^-52 is that of a sum of n * D non-negative terms in any order.  It does not cover the conditioning of ONE
    softmax row whose label holds the maximum (log S with S near 1): the labels of the rows are drawn among the classes that do not."""
    m = _model(4, D)
    rng = np.random.default_rng(1000 + D)
    for n in SIZES:
        for specials in (False, True):
            p = _scores(rng, n, D, specials)
            if obj == "softmax":
                y = rng.integers(0, D, n).astype(np.int32)
                order = np.argsort(np.where(np.isfinite(p), p, np.inf), axis=1)
                y = np.where(np.isfinite(p[np.arange(n), order[:, 0]]), order[:, 0], y).astype(np.int32)   # the lowest finite score's class
                y[0] = D - 1
                t = y
            else:
                t = (rng.random((n, D)) < 0.5).astype(np.float32)
            ps, ts = _shape(p, D), (t if obj == "softmax" else _shape(t, D))
            want = host(ps, ts, obj)
            g, loss = m.objective_gradient(ps, ts, obj)
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == ps.shape and isinstance(loss, float)
            assert g.tobytes() == want.tobytes(), "n = %d, D = %d, specials = %s: %d entries differ" % (n, D, specials, (g != want).sum())
            g2, loss2 = m.objective_gradient(ps, ts, obj)
            assert g2.tobytes() == g.tobytes() and np.float64(loss2).tobytes() == np.float64(loss).tobytes()
            ref = _loss64(obj, p, t)
            if math.isfinite(ref):
                print("%s n=%d D=%d: loss %.17g reference %.17g relative difference %.3g (bound %.3g)" %
                      (obj, n, D, loss, ref, abs(loss - ref) / abs(ref), (n * D + 8) * 2.0**-52))
                assert abs(loss - ref) <= (n * D + 8) * 2.0**-52 * abs(ref)
            else:
                assert specials and not math.isfinite(loss), (n, D, loss, ref)


@pytest.mark.parametrize("obj", ["logistic", "softmax", "rmse"])
@pytest.mark.parametrize("D", [4, 8, 9])
def test_device_buffers_aligned_and_offset_by_one_element(D, obj):
    """16-byte loads where D % 4 == 0 and the addresses allow it, 4-byte loads otherwise: the same bytes"""
    import torch
    n = 130
    m = _model(4, D)
    rng = np.random.default_rng(7 + D)
    p = _scores(rng, n, D, False)
    t = rng.integers(0, D, n).astype(np.int32) if obj == "softmax" else (rng.random((n, D)) < 0.5).astype(np.float32)
    want = host(p, t, obj)
    _, want_loss = m.objective_gradient(p, t, obj)
    for off_p, off_t in ((0, 0), (0, 1), (1, 0), (1, 1)):
        dp = torch.zeros(p.size + 1, dtype=torch.float32, device="cuda")
        dp[off_p:off_p + p.size] = torch.from_numpy(p.ravel()).cuda()
        dt = torch.zeros(t.size + 1, dtype=torch.from_numpy(t).dtype, device="cuda")
        dt[off_t:off_t + t.size] = torch.from_numpy(t.ravel()).cuda()
        vp, vt = dp[off_p:off_p + p.size].view(n, D), dt[off_t:off_t + t.size].view(t.shape)
        cap, loss = m.objective_gradient(_dev(vp), _dev(vt), obj)
        g = torch.from_dlpack(cap)
        assert g.is_cuda and tuple(g.shape) == (n, D)
        assert g.cpu().numpy().tobytes() == want.tobytes(), (off_p, off_t)
        assert np.float64(loss).tobytes() == np.float64(want_loss).tobytes(), (off_p, off_t)


# ---- 2. the loop a caller could write ---------------------------------------------------------------------------------------------------------------
def _manual_loop(m, ds, T, obj, D, bs, iterations, bias, subsample=1.0, colsample=1.0, seed=0):
    """bias, then per iteration: the held prediction advanced by predict_continue_prepared, objective_gradient, step_prepared; returns the loss"""
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
    for b0 in range(0, n, bs):
        advance(b0, min(bs, n - b0))
    _, loss = m.objective_gradient(P, T, obj)
    return loss


COMBOS = [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform"), ("oblivious", "Cosine", "Uniform"), ("greedy", "L2", "Quantile")]


@pytest.mark.parametrize("obj,D", [("logistic", 3), ("logistic", 1), ("softmax", 3)])
@pytest.mark.parametrize("policy,score,gen", COMBOS)
@pytest.mark.parametrize("n,F,bs", [(65, 16, 65), (1000, 17, 1000), (1000, 16, 300)])
def test_fit_with_an_objective_is_the_loop_a_caller_could_write(n, F, bs, policy, score, gen, obj, D, tmp_path):
    iterations = 6
    X, y, onehot = _data(n, F, D, seed=n + F + D)
    T = _targets(obj, y, onehot, D)
    files = []
    for generic in ("0", "1"):   # the streaming kernel and the general one: the same bytes
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            a = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
            ds = a.prepare_dataset(X)
            loss_a = a.fit_prepared(ds, T, iterations, objective=obj)
            assert isinstance(loss_a, float) and a.get_num_trees() == iterations
            bias = _rule_bias(obj, T, n, D)
            assert np.asarray(a.get_bias(), np.float32).tobytes() == bias.tobytes(), (a.get_bias(), bias)
            b = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
            loss_b = _manual_loop(b, ds, T, obj, D, bs, iterations, bias)
            assert _file(a, tmp_path) == _file(b, tmp_path), "generic = %s: the saved files differ" % generic
            assert _same_bits(loss_a, loss_b), (loss_a, loss_b)
            files.append((_file(a, tmp_path), loss_a))
    assert files[0][0] == files[1][0] and _same_bits(files[0][1], files[1][1])
    # and it is not the rmse fit of the same targets
    if obj == "logistic":
        c = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
        c.fit_prepared(c.prepare_dataset(X), T, iterations)
        assert _file(c, tmp_path) != files[0][0]


def test_a_warm_start_keeps_its_bias_and_continues(tmp_path):
    n, F, D = 500, 16, 3
    X, y, _ = _data(n, F, D, seed=5)
    a = _model(F, D, batch_size=n)
    ds = a.prepare_dataset(X)
    a.fit_prepared(ds, y, 3, objective="softmax")
    loss_a = a.fit_prepared(ds, y, 4, objective="softmax")
    b = _model(F, D, batch_size=n)
    loss_b = b.fit_prepared(ds, y, 7, objective="softmax")
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)


# ---- 3. validation ----------------------------------------------------------------------------------------------------------------------------------
def _rule(curve, rounds, min_delta):
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_early_stop_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(curve, np.float64)
    stop, best = C.c_int(-1), C.c_int(-1)
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, len(c), rounds, min_delta, C.byref(stop), C.byref(best)) == 0
    return stop.value, best.value


@pytest.mark.parametrize("obj", ["logistic", "softmax"])
@pytest.mark.parametrize("nv", [1, 64, 200])
@pytest.mark.parametrize("generic", ["0", "1"])
def test_valid_loss_is_the_loss_of_every_prefix(nv, obj, generic, tmp_path):
    n, F, D, iterations = 500, 16, 3, 6
    Xa, ya, onehota = _data(n + nv, F, D, seed=11 + nv)   # one population: the validation rows are its last nv
    X, y, onehot, Xv, yv, onehotv = Xa[:n], ya[:n], onehota[:n], Xa[n:], ya[n:], onehota[n:]
    T, Tv = _targets(obj, y, onehot, D), _targets(obj, yv, onehotv, D)
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        m = _model(F, D, batch_size=n)
        ds = m.prepare_dataset(X)
        dsv = m.prepare_dataset(Xv, reference=ds)
        r = m.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, objective=obj)
    assert sorted(r) == ["best_n_trees", "iterations", "loss", "valid_loss"] and r["iterations"] == iterations and r["valid_loss"].shape == (iterations + 1,)
    base = _tiled(m.get_bias(), nv, D)
    for k, got in enumerate(r["valid_loss"]):
        P = base if k == 0 else np.asarray(m.predict_continue_prepared(dsv, base, 0, k))
        _, want = m.objective_gradient(np.ascontiguousarray(P), Tv, obj)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_loss[%d] = %r, objective_gradient's loss %r" % (k, got, want)
    stop_after, best = _rule(r["valid_loss"], 0, 0.0)
    assert r["best_n_trees"] == best and stop_after == iterations


@pytest.mark.parametrize("obj", ["logistic", "softmax"])
def test_early_stopping_cuts_the_same_run(obj, tmp_path):
    n, nv, F, D, iterations = 500, 200, 16, 3, 8
    Xa, ya, onehota = _data(n + nv, F, D, seed=11 + nv)   # one population: the validation rows are its last nv
    X, y, onehot, Xv, yv, onehotv = Xa[:n], ya[:n], onehota[:n], Xa[n:], ya[n:], onehota[n:]
    T, Tv = _targets(obj, y, onehot, D), _targets(obj, yv, onehotv, D)
    full = _model(F, D, batch_size=n)
    ds = full.prepare_dataset(X)
    dsv = full.prepare_dataset(Xv, reference=ds)
    rf = full.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, objective=obj)
    gains = -np.diff(rf["valid_loss"])
    delta = float(np.sort(gains)[len(gains) // 2]) if (gains > 0).all() else 0.0   # a min_delta that only some of the gains reach
    stop_after, best = _rule(rf["valid_loss"], 2, delta)
    s = _model(F, D, batch_size=n)
    rs = s.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, early_stopping_rounds=2, min_delta=delta, objective=obj)
    assert (rs["iterations"], rs["best_n_trees"]) == (stop_after, best) and s.get_num_trees() == stop_after
    assert rs["valid_loss"].tobytes() == rf["valid_loss"][:stop_after + 1].tobytes()
    cut = _model(F, D, batch_size=n)
    loss_cut = cut.fit_prepared(ds, T, stop_after, objective=obj)
    assert _file(s, tmp_path) == _file(cut, tmp_path) and _same_bits(rs["loss"], loss_cut)


# ---- 4. descent -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", ["logistic", "softmax"])
def test_the_loss_of_the_training_rows_falls(obj):
    n, F, D = 1000, 4, 3
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, F)).astype(np.float32)
    W = np.float32([[1.0, -0.5, 0.2], [0.3, 0.8, -1.0], [-0.7, 0.1, 0.6], [0.2, -0.9, 0.4]])   # three fixed linear functions
    y = np.argmax(X @ W, axis=1).astype(np.int32)
    onehot = (y[:, None] == np.arange(D)[None, :]).astype(np.float32)
    m = _model(F, D, batch_size=n)
    ds = m.prepare_dataset(X)
    r = m.fit_prepared(ds, _targets(obj, y, onehot, D), 10, valid=ds, valid_targets=_targets(obj, y, onehot, D), objective=obj)
    vl = r["valid_loss"]
    print(obj, vl.tolist())
    assert (np.diff(vl) < 0).all(), vl.tolist()
    assert _same_bits(r["loss"], vl[-1])   # the training rows are the validation rows
    if obj == "softmax":
        f = np.bincount(y, minlength=D) / n
        assert abs(vl[0] - float(-(f * np.log(f)).sum())) <= 1e-6


# ---- 5. rmse is untouched ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3])
def test_objective_rmse_is_the_call_without_the_keyword(D, tmp_path):
    n, F = 700, 16
    rng = np.random.default_rng(9)
    X = rng.standard_normal((n, F)).astype(np.float32)
    Y = _shape((np.tanh(X[:, :D]) + 0.3 * rng.standard_normal((n, D))).astype(np.float32), D)
    out = []
    for kw in ({}, dict(objective="rmse")):
        m = _model(F, D, batch_size=300)
        ds = m.prepare_dataset(X)
        m.set_profiling(2)
        loss = m.fit_prepared(ds, Y, 5, **kw)
        out.append((_file(m, tmp_path), np.float32(loss).tobytes(), sorted(m.last_phase_times())))
        m.set_profiling(0)
    assert out[0] == out[1]
    # ... and with a validation set
    curves = []
    for kw in ({}, dict(objective="rmse")):
        m = _model(F, D, batch_size=300)
        ds = m.prepare_dataset(X)
        r = m.fit_prepared(ds, Y, 5, valid=ds, valid_targets=Y, **kw)
        curves.append((r["valid_loss"].tobytes(), np.float32(r["loss"]).tobytes(), _file(m, tmp_path)))
    assert curves[0] == curves[1] and curves[0][2] == out[0][0]


# ---- 6. sampling composes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs", [(1000, 1000), (1000, 300)])
def test_sampling_composes_with_softmax(n, bs, tmp_path):
    F, D, iterations = 16, 3, 6
    X, y, _ = _data(n, F, D, seed=21)
    runs = []
    for _ in range(2):
        a = _model(F, D, batch_size=bs)
        ds = a.prepare_dataset(X)
        loss = a.fit_prepared(ds, y, iterations, subsample=0.5, colsample=0.5, seed=1, objective="softmax")
        runs.append((_file(a, tmp_path), np.float32(loss).tobytes()))
    assert runs[0] == runs[1]
    b = _model(F, D, batch_size=bs)
    ds = b.prepare_dataset(X)
    loss_b = _manual_loop(b, ds, y, "softmax", D, bs, iterations, _rule_bias("softmax", y, n, D), subsample=0.5, colsample=0.5, seed=1)
    assert _file(b, tmp_path) == runs[0][0] and np.float32(loss_b).tobytes() == runs[0][1]
    c = _model(F, D, batch_size=bs)
    c.fit_prepared(c.prepare_dataset(X), y, iterations, objective="softmax")
    assert _file(c, tmp_path) != runs[0][0]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trees", [0, 2])
def test_refusals_leave_the_model_as_it_was(trees, tmp_path):
    n, F, D = 300, 16, 3
    X, y, onehot = _data(n, F, D, seed=31)
    m = _model(F, D, batch_size=n)
    ds = m.prepare_dataset(X)
    if trees:
        m.fit_prepared(ds, y, trees, objective="softmax")
    before = _file(m, tmp_path)
    for bad in (D, -1):
        yb = y.copy(); yb[7] = bad; yb[200] = bad
        with pytest.raises(RuntimeError, match=r"label %d \(row 7\) is outside \[0, 3\)" % bad):
            m.fit_prepared(ds, yb, 3, objective="softmax")
        with pytest.raises(RuntimeError, match=r"valid_targets.*label %d \(row 7\)" % bad):
            m.fit_prepared(ds, y, 3, valid=ds, valid_targets=yb, objective="softmax")
        with pytest.raises(RuntimeError, match=r"label %d \(row 7\)" % bad):
            m.objective_gradient(onehot, yb, "softmax")
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.fit_prepared(ds, onehot, 3, objective="softmax")          # float targets where labels are wanted
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.fit_prepared(ds, y, 3, objective="logistic")              # ... and the reverse
    with pytest.raises(RuntimeError, match="int32 class labels of shape"):
        m.fit_prepared(ds, np.zeros((n, D), np.int32), 3, objective="softmax")
    with pytest.raises(RuntimeError, match="Invalid objective"):
        m.fit_prepared(ds, y, 3, objective="hinge")
    assert _file(m, tmp_path) == before and m.get_num_trees() == trees
    one = _model(F, 1, batch_size=n)
    ds1 = one.prepare_dataset(X)
    before1 = _file(one, tmp_path)
    with pytest.raises(RuntimeError, match="output_dim >= 2"):
        one.fit_prepared(ds1, np.zeros(n, np.int32), 3, objective="softmax")
    assert _file(one, tmp_path) == before1 and one.get_num_trees() == 0
