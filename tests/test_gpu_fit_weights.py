"""Row weights on the GPU (include/gbrl_hip.h, "Row weights"): fit_prepared(weights=, valid_weights=), objective_gradient(weights=) and
newton_leaves_prepared(weights=, weight_max=).  tests/test_weights_host.py holds the host rules; here
  1. all-ones weights are no weights: the saved model file, valid_loss and the loss of the call without the keyword;
  2. the weighted fit is byte for byte -- the saved model file, the loss -- the loop objective_gradient(weights=) -> step_prepared ->
     newton_leaves_prepared(weights=, weight_max=) -> predict_continue_prepared written from the public pieces, with batches, row and column sampling;
  3. the device gradient is the host rule's bytes, its loss a float64 sum's, two calls and odd buffer offsets give the same bits;
  4. the Newton sums are NumPy's integers, and integer weights are repeated rows;
  5. a zero weight silences a row's target;
  6. valid_loss[k] with valid_weights is objective_gradient(weights=)'s loss of every prefix, and early stopping cuts that very run;
  7. two runs give the same bytes, 3 + 3 iterations are a run of 6, and what is refused leaves the model as it was.
Every fit runs through the streaming kernels and, under GBRL_HIP_CONTINUE_GENERIC=1, through the general ones.  n is no multiple of 64 or 256 (a
partly filled last wave and last loss partial); D in {1, 5, 8} takes the scalar and the float4 paths, D = 68 the DMAX = 128 family and the general
Newton kernel."""
import math
import os

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
pytestmark = pytest.mark.gpu

N, F, DEPTH, BINS, ITER = 3001, 12, 3, 32, 4
N_WIDE, D_WIDE = 701, 68
POLICIES = [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")]


def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=DEPTH, n_bins=BINS, batch_size=N):
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


def _same_f64(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


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


def _data(n, D, seed=0):
    """observations; labels = the arg-max of D noisy linear functions; their one-hot matrix; real targets; weights in [0, 8] with exact zeros"""
    if (n, D, seed) not in _DATA:
        rng = np.random.default_rng(1000 * D + n + seed)
        X = rng.standard_normal((n, F)).astype(np.float32)
        Wt = rng.standard_normal((F, max(D, 2))).astype(np.float32)
        S = X @ Wt + 0.5 * rng.standard_normal((n, max(D, 2))).astype(np.float32)
        y = np.minimum(np.argmax(S, axis=1), max(D, 2) - 1).astype(np.int32)
        onehot = (y[:, None] == np.arange(D)[None, :]).astype(np.float32)   # (D == 1: class 0 against the rest)
        real = S[:, :D].astype(np.float32) if D >= 2 else S[:, :1].astype(np.float32)
        w = rng.uniform(0.0, 8.0, n).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
        w[0] = 0.0
        w[n - 1] = 8.0
        _DATA[(n, D, seed)] = dict(X=X, y=y, onehot=onehot, real=real, w=w)
    return _DATA[(n, D, seed)]


def _targets(obj, d, D):
    return d["y"] if obj == "softmax" else _shape(d["real"] if obj == "rmse" else d["onehot"], D)


def _tiled(bias, n, D):
    return _shape(np.tile(np.asarray(bias, np.float32).reshape(1, D), (n, 1)), D)


# ---- 1. ones are no weights ---------------------------------------------------------------------------------------------------------------------------
ONES = [("rmse", 1, "gradient", N), ("rmse", 8, "gradient", N // 3 + 1), ("logistic", 5, "gradient", N // 3 + 1), ("logistic", 8, "newton", N),
        ("logistic", 1, "newton", N // 3 + 1), ("softmax", 5, "newton", N), ("softmax", 8, "gradient", N // 3 + 1)]


def _ones_case(obj, D, leaf, bs, n, policy, score, gen, tmp_path):
    d = _data(n + 300, D)
    X, Xv = d["X"][:n], d["X"][n:]
    T = _targets(obj, d, D)
    T, Tv = np.ascontiguousarray(T[:n]), np.ascontiguousarray(T[n:])
    ones, onesv = np.ones(n, np.float32), np.ones(300, np.float32)
    kw = dict(objective=obj, leaf_update=leaf, leaf_l2=0.5)
    seen = []
    for generic in ("0", "1"):
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            a = _model(F, D, policy, score, gen, batch_size=bs)
            ds = a.prepare_dataset(X)
            dsv = a.prepare_dataset(Xv, reference=ds)
            b = _model(F, D, policy, score, gen, batch_size=bs)
            for start in ("fresh", "warm"):   # (the second pass continues both models from their trees)
                ra = a.fit_prepared(ds, T, ITER, valid=dsv, valid_targets=Tv, **kw)
                rb = b.fit_prepared(ds, T, ITER, valid=dsv, valid_targets=Tv, weights=ones, valid_weights=onesv, **kw)
                assert _file(a, tmp_path) == _file(b, tmp_path), "%s, generic = %s: the saved files differ" % (start, generic)
                assert _same_f64(ra["valid_loss"], rb["valid_loss"]), (start, generic)
                assert "weight_max" not in ra and rb["weight_max"] == 1.0
                la, lb = np.float32(ra["loss"]), np.float32(rb["loss"])
                if obj == "rmse":   # summed by rows, not by columns: one float32 ulp, here and nowhere else
                    assert abs(int(la.view(np.int32)) - int(lb.view(np.int32))) <= 1, (la, lb)
                else:
                    assert la.tobytes() == lb.tobytes(), (la, lb)
                # and without a validation set: the float of the call without the keyword
                c = _model(F, D, policy, score, gen, batch_size=bs)
                if start == "fresh":
                    lc = c.fit_prepared(ds, T, ITER, weights=ones, **kw)
                    assert isinstance(lc, float) and np.float32(lc).tobytes() == lb.tobytes()
            seen.append((_file(b, tmp_path), np.asarray(rb["valid_loss"]).tobytes(), np.float32(rb["loss"]).tobytes()))
    assert seen[0] == seen[1], "the two kernel families differ"


@pytest.mark.parametrize("policy,score,gen", POLICIES)
@pytest.mark.parametrize("obj,D,leaf,bs", ONES)
def test_ones_are_no_weights(obj, D, leaf, bs, policy, score, gen, tmp_path):
    _ones_case(obj, D, leaf, bs, N, policy, score, gen, tmp_path)


def test_ones_are_no_weights_wide(tmp_path):
    _ones_case("softmax", D_WIDE, "newton", N_WIDE, N_WIDE, "oblivious", "L2", "Quantile", tmp_path)


# ---- 2. the loop a caller could write -------------------------------------------------------------------------------------------------------------------
def _manual_loop(m, ds, T, w, obj, D, bs, iterations, bias, leaf, leaf_l2, subsample=1.0, colsample=1.0, seed=0):
    """tests/test_gpu_fit_newton.py's loop with weights: the held prediction advanced by predict_continue_prepared, objective_gradient(weights=),
    step_prepared, then (newton) newton_leaves_prepared on the rows the tree was grown on with the data set's largest weight; returns the loss"""
    n = ds.n_rows
    if bias is not None:
        m.set_bias(np.asarray(bias, np.float32))
    P = _tiled(m.get_bias(), n, D)
    wmax = float(w.max())
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
        G, _ = m.objective_gradient(np.ascontiguousarray(P[sl]), np.ascontiguousarray(T[sl]), obj, weights=np.ascontiguousarray(w[sl]))
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
        if leaf == "newton":
            pred, tar, wr = (P, T, w) if rows is None else (np.ascontiguousarray(P[rows]), np.ascontiguousarray(T[rows]), np.ascontiguousarray(w[rows]))
            r = m.newton_leaves_prepared(ds, pred, tar, obj, leaf_l2=leaf_l2, rows=rows, weights=wr, weight_max=wmax)
            assert r["bits"] == cpp.newton_sum_bits(len(wr), wmax)
    for b0 in range(0, n, bs):
        advance(b0, min(bs, n - b0))
    _, loss = m.objective_gradient(P, T, obj, weights=w)
    return loss


def _loop_case(obj, D, leaf, loop, n, policy, score, gen, tmp_path):
    d = _data(n, D)
    X, w, T = d["X"], d["w"], _targets(obj, d, D)
    bs = n if loop["bs"] is None else loop["bs"]
    opts = {k: v for k, v in loop.items() if k != "bs"}
    files = []
    for generic in ("0", "1"):   # the streaming kernels and the general ones: the same bytes
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            a = _model(F, D, policy, score, gen, batch_size=bs)
            ds = a.prepare_dataset(X)
            loss_a = a.fit_prepared(ds, T, ITER, objective=obj, leaf_update=leaf, leaf_l2=0.5, weights=w, **opts)
            assert isinstance(loss_a, float) and a.get_num_trees() == ITER
            b = _model(F, D, policy, score, gen, batch_size=bs)
            loss_b = _manual_loop(b, ds, T, w, obj, D, bs, ITER, np.asarray(a.get_bias(), np.float32), leaf, 0.5, **opts)
            assert _file(a, tmp_path) == _file(b, tmp_path), "generic = %s: the saved files differ" % generic
            assert _same_bits(loss_a, loss_b), (loss_a, loss_b)
            files.append((_file(a, tmp_path), loss_a))
    assert files[0][0] == files[1][0] and _same_bits(files[0][1], files[1][1])
    # and it is not the unweighted fit
    c = _model(F, D, policy, score, gen, batch_size=bs)
    c.fit_prepared(c.prepare_dataset(X), T, ITER, objective=obj, leaf_update=leaf, leaf_l2=0.5, **opts)
    assert _file(c, tmp_path) != files[0][0]


LOOPS = [dict(bs=None), dict(bs=N // 3 + 1), dict(bs=None, subsample=0.5, seed=11), dict(bs=N // 3 + 1, subsample=0.5, colsample=0.5, seed=5)]
LOOP_OBJ = [("rmse", 5, "gradient"), ("rmse", 8, "gradient"), ("logistic", 8, "gradient"), ("logistic", 1, "newton"), ("softmax", 5, "newton"), ("softmax", 8, "gradient")]


@pytest.mark.parametrize("policy,score,gen", POLICIES)
@pytest.mark.parametrize("obj,D,leaf", LOOP_OBJ)
@pytest.mark.parametrize("loop", LOOPS, ids=["whole", "batches", "subsample", "batches-subsample-colsample"])
def test_weighted_fit_is_the_loop_a_caller_could_write(loop, obj, D, leaf, policy, score, gen, tmp_path):
    _loop_case(obj, D, leaf, loop, N, policy, score, gen, tmp_path)


@pytest.mark.parametrize("obj,leaf", [("softmax", "newton"), ("logistic", "newton"), ("rmse", "gradient")])
def test_weighted_fit_is_the_loop_wide(obj, leaf, tmp_path):
    _loop_case(obj, D_WIDE, leaf, dict(bs=N_WIDE // 3 + 1), N_WIDE, "oblivious", "L2", "Quantile", tmp_path)


def test_the_fresh_bias_is_the_weighted_mean(tmp_path):
    """the rule restated in float64 (sum w y / W; its log odds, clamped by 0.5 / n; log(max(W_c, 0.5 W / n) / W)), to a few float32 ulps"""
    D = 5
    d = _data(N, D)
    w64 = d["w"].astype(np.float64)
    Wsum = math.fsum(w64)
    for obj in ("rmse", "logistic", "softmax"):
        m = _model(F, D)
        m.fit_prepared(m.prepare_dataset(d["X"]), _targets(obj, d, D), 1, objective=obj, weights=d["w"])
        if obj == "softmax":
            Wc = np.array([math.fsum(w64[d["y"] == c]) for c in range(D)])
            want = np.log(np.maximum(Wc, 0.5 * Wsum / N) / Wsum)
        else:
            Y = (d["real"] if obj == "rmse" else d["onehot"]).astype(np.float64)
            mean = np.array([math.fsum(w64 * Y[:, c]) for c in range(D)]) / Wsum
            want = mean if obj == "rmse" else np.log(np.clip(mean, 0.5 / N, 1 - 0.5 / N) / (1 - np.clip(mean, 0.5 / N, 1 - 0.5 / N)))
        got = np.asarray(m.get_bias(), np.float64)
        assert np.all(np.abs(got - want) <= 4 * 2.0**-23 * np.maximum(np.abs(want), 2.0**-10)), (obj, got, want)


# ---- 3. device equals host ------------------------------------------------------------------------------------------------------------------------------
def _loss64(obj, p, t, w):
    """the weighted loss in float64: the formulas of the header, the terms summed exactly"""
    n = p.shape[0]
    p = p.reshape(n, -1).astype(np.float64)
    w = w.astype(np.float64)
    if obj == "softmax":
        m = p.max(axis=1)
        rows = np.log(np.exp(p - m[:, None]).sum(axis=1)) + m - p[np.arange(n), t]
    elif obj == "logistic":
        y = t.reshape(p.shape).astype(np.float64)
        rows = np.array([math.fsum(r) for r in (np.maximum(p, 0) - y * p + np.log1p(np.exp(-np.abs(p))))])
    else:
        g = (p.astype(np.float32) - t.reshape(p.shape)).astype(np.float64)
        rows = np.array([math.fsum(r) for r in g * g])
    mean = math.fsum(w * rows) / math.fsum(w)
    return math.sqrt(0.5 * mean) if obj == "rmse" else mean


@pytest.mark.parametrize("n,D,obj", [(n, D, obj) for n, D in ((N, 1), (N, 5), (N, 8), (N_WIDE, D_WIDE), (63, 5)) for obj in ("rmse", "logistic", "softmax")
                                     if not (obj == "softmax" and D == 1)])
def test_device_gradient_and_loss_are_the_host_rule(n, D, obj):
    """The loss bound is tests/test_gpu_objective.py's with one more rounding per row, under the caveats stated there: the softmax labels are drawn
    among the classes that do not hold the row's maximum."""
    m = _model(4, D)
    rng = np.random.default_rng(31 * n + D)
    p = rng.uniform(-8, 8, (n, D)).astype(np.float32)
    w = rng.uniform(0.0, 8.0, n).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.0
    w[0], w[n - 1] = 65536.0, 1.0
    t = np.argmin(p, axis=1).astype(np.int32) if obj == "softmax" else (rng.random((n, D)) < 0.5).astype(np.float32) if obj == "logistic" else rng.standard_normal((n, D)).astype(np.float32)
    ps, ts = _shape(p, D), (t if obj == "softmax" else _shape(t, D))
    want = cpp.objective_gradient_host(ps, ts, obj, weights=w)
    g, loss = m.objective_gradient(ps, ts, obj, weights=w)
    assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == ps.shape and isinstance(loss, float)
    assert g.tobytes() == want.tobytes(), "%d entries differ" % (g != want).sum()
    g2, loss2 = m.objective_gradient(ps, ts, obj, weights=w)
    assert g2.tobytes() == g.tobytes() and _same_f64(loss, loss2)
    ref = _loss64(obj, p, t, w)
    bound = (n * D + n + 8) * 2.0**-52
    print("%s n=%d D=%d: loss %.17g reference %.17g relative difference %.3g (bound %.3g)" % (obj, n, D, loss, ref, abs(loss - ref) / abs(ref), bound))
    assert abs(loss - ref) <= bound * abs(ref)
    # all-ones weights: the unweighted gradient bytes (the loss is the unweighted one too: W == n exactly)
    g1, loss1 = m.objective_gradient(ps, ts, obj, weights=np.ones(n, np.float32))
    g0, loss0 = m.objective_gradient(ps, ts, obj)
    assert g1.tobytes() == g0.tobytes() and _same_f64(loss1, loss0)


@pytest.mark.parametrize("obj", ["rmse", "logistic", "softmax"])
@pytest.mark.parametrize("D", [8, 5])
def test_device_buffers_offset_by_one_element(D, obj):
    """16-byte loads where D % 4 == 0 and the addresses allow it, 4-byte loads otherwise: the same bytes"""
    import torch
    n = 333
    m = _model(4, D)
    rng = np.random.default_rng(7 + D)
    p = rng.uniform(-8, 8, (n, D)).astype(np.float32)
    w = rng.uniform(0.0, 8.0, n).astype(np.float32)
    t = rng.integers(0, D, n).astype(np.int32) if obj == "softmax" else (rng.random((n, D)) < 0.5).astype(np.float32)
    want = cpp.objective_gradient_host(p, t, obj, weights=w)
    _, want_loss = m.objective_gradient(p, t, obj, weights=w)
    for off_p, off_t, off_w in ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        def place(a, off):
            buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
            buf[off:off + a.size] = torch.from_numpy(a.ravel()).cuda()
            return buf, buf[off:off + a.size].view(a.shape)
        (kp, vp), (kt, vt), (kw_, vw) = place(p, off_p), place(t, off_t), place(w, off_w)
        cap, loss = m.objective_gradient(_dev(vp), _dev(vt), obj, weights=_dev(vw))
        g = torch.from_dlpack(cap)
        assert g.is_cuda and tuple(g.shape) == (n, D)
        assert g.cpu().numpy().tobytes() == want.tobytes(), (off_p, off_t, off_w)
        assert _same_f64(loss, want_loss), (off_p, off_t, off_w)


# ---- 4. the Newton sums are exact -------------------------------------------------------------------------------------------------------------------------
def _grown(obj, D, policy, score, gen, n):
    """a model with one tree grown on the weighted gradient at the bias, its data set, the bias prediction"""
    d = _data(n, D)
    T = _targets(obj, d, D)
    m = _model(F, D, policy, score, gen, batch_size=n)
    ds = m.prepare_dataset(d["X"])
    first = _model(F, D, policy, score, gen, batch_size=n)
    first.fit_prepared(ds, T, 1, objective=obj, weights=d["w"])   # (for its bias)
    m.set_bias(np.asarray(first.get_bias(), np.float32))
    P = _tiled(m.get_bias(), n, D)
    G, _ = m.objective_gradient(P, T, obj, weights=d["w"])
    m.step_prepared(ds, G)
    return m, ds, P, T, d


@pytest.mark.parametrize("policy,score,gen", POLICIES)
@pytest.mark.parametrize("obj,D,n", [("logistic", 1, N), ("logistic", 8, N), ("softmax", 5, N), ("softmax", D_WIDE, N_WIDE)])
def test_newton_sums_are_numpys_integers(obj, D, n, policy, score, gen):
    m, ds, P, T, d = _grown(obj, D, policy, score, gen, n)
    w = d["w"]
    ens = m.get_ensemble_data()
    NL = int(np.asarray(ens["values"]).reshape(-1, D).shape[0])
    leaves = np.asarray(m.predict_leaves(d["X"], None, 0, 1)).reshape(n)
    gw = cpp.objective_gradient_host(P, T, obj, weights=w).reshape(n, D)
    hw = cpp.objective_hessian_host(P, None, obj, weights=w).reshape(n, D)
    for wmax, e in ((None, 3), (8.0, 3), (9.0, 4), (65536.0, 16)):   # (the largest weight is 8)
        bits = min(40, 62 - int(n).bit_length() - e)
        assert bits == cpp.newton_sum_bits(n, float(w.max()) if wmax is None else wmax)
        q = lambda x: np.rint(x.astype(np.float64) * 2.0 ** bits).astype(np.int64)
        sums = np.zeros((NL, 2 * D + 1), np.int64)
        np.add.at(sums[:, :D], leaves, q(gw))
        np.add.at(sums[:, D:2 * D], leaves, q(hw))
        np.add.at(sums[:, 2 * D], leaves, 1)
        for generic in ("0", "1"):
            with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
                r = m.newton_leaves_prepared(ds, P, T, obj, leaf_l2=1.0, weights=w, weight_max=wmax)
            assert r["bits"] == bits
            assert r["sums"].tobytes() == sums.tobytes(), "weight_max = %r, generic = %s: the sums differ from NumPy's" % (wmax, generic)
    assert float(w.max()) == 8.0 and cpp.newton_sum_bits(n, 65536.0) < 40   # the last case really summed in a coarser quantum


@pytest.mark.parametrize("obj,D", [("logistic", 8), ("softmax", 5)])
def test_integer_weights_are_repeated_rows(obj, D):
    """weights from {0, 1, 2, 4}: w * g is exact, and bits is 40 with and without them at these sizes, so Sg and Sh are those of the unweighted call
    on rows= with every row repeated w times"""
    m, ds, P, T, d = _grown(obj, D, "oblivious", "L2", "Quantile", N)
    rng = np.random.default_rng(5)
    w = rng.choice(np.float32([0, 1, 2, 4]), N).astype(np.float32)
    rows = np.repeat(np.arange(N, dtype=np.int32), w.astype(np.int64))
    assert cpp.newton_sum_bits(N, 4.0) == 40 == cpp.newton_sum_bits(len(rows))
    for generic in ("0", "1"):
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            a = m.newton_leaves_prepared(ds, P, T, obj, leaf_l2=1.0, weights=w)
            b = m.newton_leaves_prepared(ds, np.ascontiguousarray(P[rows]), np.ascontiguousarray(T[rows]), obj, leaf_l2=1.0, rows=rows)
        assert a["bits"] == b["bits"] == 40
        assert a["sums"][:, :2 * D].tobytes() == b["sums"][:, :2 * D].tobytes()
        assert int(a["sums"][:, 2 * D].sum()) == N and int(b["sums"][:, 2 * D].sum()) == len(rows)   # cnt counts rows, not weight


# ---- 5. a zero weight silences a row ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj,D,leaf", [("rmse", 5, "gradient"), ("logistic", 8, "newton"), ("logistic", 1, "gradient"), ("softmax", 5, "newton")])
def test_a_zero_weight_silences_a_row(obj, D, leaf, tmp_path):
    n, nv = N, 300
    d = _data(n + nv, D)
    X, Xv, w, wv = d["X"][:n], d["X"][n:], d["w"][:n].copy(), d["w"][n:].copy()
    T = _targets(obj, d, D)
    rng = np.random.default_rng(77)
    other = T.copy()
    off = np.concatenate([w, wv]) == 0.0
    assert off[:n].sum() > 100 and off[n:].sum() > 10
    if obj == "softmax":
        other[off] = (T[off] + 1 + rng.integers(0, D - 1, off.sum())) % D          # another label in range
    elif obj == "logistic":
        other[off] = np.float32(1.0) - T[off]                                      # the other class, still in [0, 1]
    else:
        other[off] = T[off] + rng.standard_normal(T[off].shape).astype(np.float32) * 100
    assert not np.array_equal(other, T)
    seen = []
    for generic in ("0", "1"):
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            for tar in (T, other):
                m = _model(F, D, batch_size=n // 3 + 1)
                ds = m.prepare_dataset(X)
                dsv = m.prepare_dataset(Xv, reference=ds)
                r = m.fit_prepared(ds, np.ascontiguousarray(tar[:n]), ITER, valid=dsv, valid_targets=np.ascontiguousarray(tar[n:]), objective=obj, leaf_update=leaf,
                                   weights=w, valid_weights=wv)
                seen.append((_file(m, tmp_path), np.float32(r["loss"]).tobytes(), np.asarray(r["valid_loss"], np.float64).tobytes()))
    assert seen[0] == seen[1] == seen[2] == seen[3]


# ---- 6. validation ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", ["0", "1"])
@pytest.mark.parametrize("obj,D", [("rmse", 5), ("logistic", 8), ("softmax", 5), ("softmax", D_WIDE)])
def test_valid_loss_is_the_weighted_loss_of_every_prefix(obj, D, generic, tmp_path):
    n, nv = (N_WIDE, 203) if D == D_WIDE else (N, 333)
    d = _data(n + nv, D)
    X, Xv, w, wv = d["X"][:n], d["X"][n:], d["w"][:n].copy(), d["w"][n:].copy()
    T = _targets(obj, d, D)
    T, Tv = np.ascontiguousarray(T[:n]), np.ascontiguousarray(T[n:])
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        m = _model(F, D, batch_size=n)
        ds = m.prepare_dataset(X)
        dsv = m.prepare_dataset(Xv, reference=ds)
        m.fit_prepared(ds, T, 2, objective=obj, weights=w)   # T0 = 2: the curve starts at the trees the model has
        r = m.fit_prepared(ds, T, ITER, valid=dsv, valid_targets=Tv, objective=obj, weights=w, valid_weights=wv)
        assert r["iterations"] == ITER and r["valid_loss"].shape == (ITER + 1,) and r["weight_max"] == float(w.max())
        base = _tiled(m.get_bias(), nv, D)
        for k, got in enumerate(r["valid_loss"]):
            P = np.asarray(m.predict_continue_prepared(dsv, base, 0, 2 + k))
            _, want = m.objective_gradient(np.ascontiguousarray(P), Tv, obj, weights=wv)
            assert _same_f64(got, want), "valid_loss[%d] = %r, objective_gradient's loss %r" % (k, got, want)
        # the unweighted curve is another one
        _, plain = m.objective_gradient(np.ascontiguousarray(P), Tv, obj)
        assert not _same_f64(plain, r["valid_loss"][ITER])
        # the model is the one the call without a validation set leaves
        b = _model(F, D, batch_size=n)
        b.fit_prepared(ds, T, 2, objective=obj, weights=w)
        loss_b = b.fit_prepared(ds, T, ITER, objective=obj, weights=w)
        assert _file(m, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], loss_b)


def test_early_stopping_cuts_the_same_weighted_run(tmp_path):
    obj, D, n, nv, iters = "logistic", 1, N, 333, 12
    d = _data(n + nv, D)
    rng = np.random.default_rng(3)
    X, Xv, w, wv = d["X"][:n], d["X"][n:], d["w"][:n].copy(), d["w"][n:].copy()
    T = _targets(obj, d, D)
    T, Tv = np.ascontiguousarray(T[:n]), rng.permutation(np.ascontiguousarray(T[n:]))   # shuffled validation targets: the curve turns early
    a = _model(F, D, batch_size=n)
    ds = a.prepare_dataset(X)
    dsv = a.prepare_dataset(Xv, reference=ds)
    full = a.fit_prepared(ds, T, iters, valid=dsv, valid_targets=Tv, objective=obj, weights=w, valid_weights=wv)
    b = _model(F, D, batch_size=n)
    cut = b.fit_prepared(ds, T, iters, valid=dsv, valid_targets=Tv, objective=obj, weights=w, valid_weights=wv, early_stopping_rounds=2)
    k = cut["iterations"]
    assert k < iters, "the curve never turned: %r" % (full["valid_loss"],)
    assert _same_f64(cut["valid_loss"], full["valid_loss"][:k + 1])
    best = int(np.argmin(full["valid_loss"][:k + 1]))
    assert cut["best_n_trees"] == best and k - best >= 2
    c = _model(F, D, batch_size=n)
    loss_c = c.fit_prepared(ds, T, k, objective=obj, weights=w)
    assert _file(b, tmp_path) == _file(c, tmp_path) and _same_bits(cut["loss"], loss_c)


# ---- 7. determinism and refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj,D,leaf", [("rmse", 8, "gradient"), ("logistic", 5, "newton"), ("softmax", 5, "newton")])
def test_two_runs_and_a_warm_start(obj, D, leaf, tmp_path):
    d = _data(N, D)
    X, w, T = d["X"], d["w"], _targets(obj, d, D)
    kw = dict(objective=obj, leaf_update=leaf, subsample=0.7, seed=3, weights=w)
    a = _model(F, D, batch_size=N // 3 + 1)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, T, 6, **kw)
    b = _model(F, D, batch_size=N // 3 + 1)
    loss_b = b.fit_prepared(ds, T, 6, **kw)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)
    # 3 + 3 at batch_size = n (a warm start begins at row 0 again, as a run of 6 whole-data iterations does)
    kw = dict(objective=obj, leaf_update=leaf, weights=w)
    c = _model(F, D, batch_size=N)
    c.fit_prepared(ds, T, 3, **kw)
    loss_c = c.fit_prepared(ds, T, 3, **kw)
    e = _model(F, D, batch_size=N)
    loss_e = e.fit_prepared(ds, T, 6, **kw)
    assert _file(c, tmp_path) == _file(e, tmp_path) and _same_bits(loss_c, loss_e)


@pytest.mark.parametrize("trees", [0, 2])
def test_refusals_leave_the_model_as_it_was(trees, tmp_path):
    D, obj, n, nv = 5, "softmax", N, 300
    d = _data(n + nv, D)
    X, Xv, w, wv = d["X"][:n], d["X"][n:], d["w"][:n].copy(), d["w"][n:].copy()
    T, Tv = np.ascontiguousarray(d["y"][:n]), np.ascontiguousarray(d["y"][n:])
    m = _model(F, D, batch_size=n)
    ds = m.prepare_dataset(X)
    dsv = m.prepare_dataset(Xv, reference=ds)
    if trees:
        m.fit_prepared(ds, T, trees, objective=obj, weights=w)
    keep = _file(m, tmp_path)

    def bad(at, value, base=w):
        out = base.copy()
        out[at] = value
        return out
    valid = dict(valid=dsv, valid_targets=Tv)
    cases = [(dict(weights=bad(n - 1, np.nan)), r"row %d\)" % (n - 1)), (dict(weights=bad(64, -1.0)), r"row 64\)"), (dict(weights=bad(0, np.inf)), r"row 0\)"),
             (dict(weights=bad(1000, 65537.0)), r"row 1000\)"), (dict(weights=bad([7, 2000], -np.inf)), r"row 7\)"), (dict(weights=np.zeros(n, np.float32)), "sum to 0"),
             (dict(weights=w[:-1].copy()), "weights"), (dict(weights=w.astype(np.float64)), "format"), (dict(weights=np.ones((n, 1), np.float32)), "weights"),
             (dict(weights=w, valid_weights=wv), "valid_weights need a validation set"),
             (dict(weights=w, valid_weights=bad(299, np.nan, wv), **valid), r"valid_weights\).*row 299\)"), (dict(valid_weights=np.zeros(nv, np.float32), **valid), "sum to 0"),
             (dict(valid_weights=wv[:-1].copy(), **valid), "valid_weights"), (dict(valid_weights=wv, eval_metric="error", **valid), "not supported")]
    for kw, what in cases:
        with pytest.raises(RuntimeError, match=what):
            m.fit_prepared(ds, T, 2, objective=obj, **kw)
        assert _file(m, tmp_path) == keep and m.get_num_trees() == trees, what
    # device vectors are refused alike
    import torch
    tw = torch.from_numpy(bad(2999, -3.0)).cuda()
    with pytest.raises(RuntimeError, match=r"row 2999\)"):
        m.fit_prepared(ds, T, 2, objective=obj, weights=_dev(tw))
    assert _file(m, tmp_path) == keep
    # the stand-alone pieces
    P = _tiled(m.get_bias(), n, D)
    for kw, what in ((dict(weights=bad(5, np.nan)), r"row 5\)"), (dict(weights=np.zeros(n, np.float32)), "sum to 0"), (dict(weights=w[:-1].copy()), "weights")):
        with pytest.raises(RuntimeError, match=what):
            m.objective_gradient(P, T, obj, **kw)
    if trees:
        for kw, what in ((dict(weights=bad(5, -1.0)), r"row 5\)"), (dict(weights=w, weight_max=4.0), "below the largest"), (dict(weights=w, weight_max=65537.0), "65536"),
                         (dict(weight_max=8.0), "weight_max needs weights"), (dict(weights=w[:-1].copy()), "weights")):
            with pytest.raises(RuntimeError, match=what):
                m.newton_leaves_prepared(ds, P, T, obj, **kw)
            assert _file(m, tmp_path) == keep, what
    # training weights with a metric are fine, and so is everything refused above once it is put right
    r = m.fit_prepared(ds, T, 1, objective=obj, weights=w, eval_metric="error", **valid)
    assert m.get_num_trees() == trees + 1 and r["valid_metric"].shape == (2,)
