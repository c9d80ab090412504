"""fit_prepared growing every tree on a one-side sample of its batch, on the GPU (GBRL.fit_prepared(ds, T, iterations, goss=(top_rate, other_rate),
seed=); include/gbrl_hip.h, "One-side sampling").  Every comparison is exact (file bytes, the bits of the loss):
  * against the loop a caller could write from public calls: predict_continue_prepared of a held prediction, objective_gradient, ds.sample_goss at
    draw = the tree count (the whole batch, unamplified, when no row is kept), step_prepared(ds, grads, rows=rows), with leaf_update='newton'
    newton_leaves_prepared(rows=rows, weights=fl32(w * factor), weight_max=fl32(wmax * amp)) -- for rmse, logistic and softmax (whose first tree is
    all ties), with weights=, Newton leaves and colsample=;
  * with a validation set valid_loss is staged_loss's bits; a warm start continues the sequence of draws;
  * a data set so small that draws keep no row; goss=None is the call without the keyword and records no sampler phase; the refusals.
"""
import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
pytestmark = pytest.mark.gpu

F = 7
GOSS_STREAM = 0x676F737372657374
POLICIES = [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")]
SHAPES = [(4096, 5000, 6), (1000, 384, 7), (4100, 4096, 5)]


def _model(D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, batch_size=5000, n_features=F):
    m = gbrl_amd.GBRL(input_dim=n_features, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(n_features, np.float32))
    m.set_feature_mapping(np.arange(n_features, dtype=np.int32), np.ones(n_features, dtype=bool))
    return m


_DATA = {}


def _data(n, D, n_features=F):
    """observations; labels = the arg-max of noisy linear functions, their one-hot matrix, real targets; weights in [0, 8] with exact zeros"""
    if (n, D, n_features) not in _DATA:
        rng = np.random.default_rng(1000 * D + n)
        X = rng.standard_normal((n, n_features)).astype(np.float32)
        C = max(D, 2)
        S = (X @ rng.standard_normal((n_features, C)).astype(np.float32) + 0.5 * rng.standard_normal((n, C))).astype(np.float32)
        y = np.argmax(S, axis=1).astype(np.int32)
        onehot = (y[:, None] == np.arange(D)[None, :]).astype(np.float32)
        w = rng.uniform(0.0, 8.0, n).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
        w[n - 1] = 8.0
        _DATA[(n, D, n_features)] = dict(X=X, y=y, onehot=onehot, real=np.tanh(S[:, :D]).astype(np.float32), w=w)
    return _DATA[(n, D, n_features)]


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


def _targets(obj, d, D):
    return d["y"] if obj == "softmax" else _shape(d["real"] if obj == "rmse" else d["onehot"], D)


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def _batches(n, bs, iterations):
    start = 0
    for _ in range(iterations):
        bn = bs if start + bs < n else n - start
        yield start, bn
        start += bn
        if start >= n:
            start = 0


def _amp(goss):
    return np.float32((1.0 - np.float64(goss[0])) / np.float64(goss[1]))


def _manual_loop(m, ds, T, w, obj, D, bs, iterations, bias, goss, seed, leaf="gradient", leaf_l2=0.5, colsample=1.0):
    """the loop a caller could write; returns (the loss, the draws it saw as (draw, rows kept, top rows))"""
    n = ds.n_rows
    if bias is not None:
        m.set_bias(np.asarray(bias, np.float32))
    P = _shape(np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (n, 1)), D)
    wmax = np.float32(1.0) if w is None else np.float32(w.max())
    through, seen = {}, []

    def advance(start, bn):
        a, Tn = through.get(start, 0), m.get_num_trees()
        if a < Tn:
            whole = None if bn == n else np.arange(start, start + bn, dtype=np.int32)
            P[start:start + bn] = np.asarray(m.predict_continue_prepared(ds, np.ascontiguousarray(P[start:start + bn]), a, Tn, rows=whole))
        through[start] = Tn

    for start, bn in _batches(n, bs, iterations):
        sl = slice(start, start + bn)
        draw = m.get_num_trees()
        advance(start, bn)
        G, _ = m.objective_gradient(np.ascontiguousarray(P[sl]), np.ascontiguousarray(T[sl]), obj, weights=None if w is None else np.ascontiguousarray(w[sl]))
        r = ds.sample_goss(np.ascontiguousarray(G), goss[0], goss[1], seed=seed, draw=draw, start=start, stop=start + bn)
        seen.append((draw, r["rows"].size, int((r["factor"] == np.float32(1.0)).sum())))
        kept = r["rows"].size > 0
        rows = r["rows"] if kept else (None if bn == n else np.arange(start, start + bn, dtype=np.int32))
        kw = {}
        if colsample < 1.0:
            kw["cols"] = ds.sample_cols(colsample, seed=seed, draw=draw)
        m.step_prepared(ds, r["grads"] if kept else G, rows=rows, **kw)
        if leaf == "newton":
            pred, tar = (P, T) if rows is None else (np.ascontiguousarray(P[rows]), np.ascontiguousarray(T[rows]))
            if kept:      # the effective weights fl32(w * factor), with room for fl32(wmax * amp)
                e = r["factor"] if w is None else (w[rows] * r["factor"]).astype(np.float32)
                wm = float(np.float32(wmax * _amp(goss)))
                out = m.newton_leaves_prepared(ds, pred, tar, obj, leaf_l2=leaf_l2, rows=rows, weights=np.ascontiguousarray(e), weight_max=wm)
                assert out["bits"] == cpp.newton_sum_bits(len(rows), wm)
            elif w is None:
                m.newton_leaves_prepared(ds, pred, tar, obj, leaf_l2=leaf_l2, rows=rows)
            else:
                m.newton_leaves_prepared(ds, pred, tar, obj, leaf_l2=leaf_l2, rows=rows, weights=np.ascontiguousarray(w if rows is None else w[rows]), weight_max=float(wmax))
    for b0 in range(0, n, bs):
        advance(b0, min(bs, n - b0))
    if obj == "rmse" and w is None:   # the column-sum loss of the plain loop: fit_prepared's own final stage on no further iteration
        return m.fit_prepared(ds, T, 0), seen
    return m.objective_gradient(P, T, obj, weights=w)[1], seen


# ---- 1. the loop a caller could write -----------------------------------------------------------------------------------------------------------------
CASES = [("rmse", 1, {}), ("rmse", 8, {}), ("logistic", 3, {}), ("softmax", 4, {}),
         ("rmse", 8, dict(weights=True, colsample=0.5)), ("logistic", 3, dict(leaf_update="newton")),
         ("softmax", 4, dict(leaf_update="newton", weights=True)), ("softmax", 8, dict(weights=True))]


@pytest.mark.parametrize("obj,D,extra", CASES, ids=["%s-%d-%s" % (o, D, "+".join(sorted(x)) or "plain") for o, D, x in CASES])
@pytest.mark.parametrize("policy,score,gen", POLICIES)
@pytest.mark.parametrize("n,bs,T", SHAPES)
def test_a_goss_fit_is_the_loop_a_caller_could_write(n, bs, T, policy, score, gen, obj, D, extra, tmp_path):
    goss, seed = (0.2, 0.1), 1000 * D + n
    d = _data(n, D)
    X, tar = d["X"], _targets(obj, d, D)
    w = d["w"] if extra.get("weights") else None
    leaf, colsample = extra.get("leaf_update", "gradient"), extra.get("colsample", 1.0)
    kw = dict(objective=obj, leaf_update=leaf, leaf_l2=0.5, colsample=colsample, seed=seed)
    if w is not None:
        kw["weights"] = w
    a = _model(D, policy, score, gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, tar, T, goss=goss, **kw)
    assert isinstance(loss_a, float) and a.get_num_trees() == T
    b = _model(D, policy, score, gen, batch_size=bs)
    loss_b, seen = _manual_loop(b, ds, tar, w, obj, D, bs, T, a.get_bias(), goss, seed, leaf=leaf, colsample=colsample)
    for (draw, m, top), (_, bn) in zip(seen, _batches(n, bs, T)):
        assert top == (int(np.floor(np.float64(goss[0]) * bn)) if m else 0), "exactly floor(a * rows) top rows (draws: %s)" % seen
        assert m < bn if bn > 64 else True, "the premise: the large batches are sampled"
    assert any(m > 0 for _, m, _ in seen)
    assert _file(a, tmp_path) == _file(b, tmp_path), "the saved files differ (draws: %s)" % seen
    assert _same_bits(loss_a, loss_b), "loss %r != %r" % (loss_a, loss_b)
    # and it is neither the unsampled fit nor the subsampled one at the same kept fraction
    for other in ({}, dict(subsample=0.3)):
        c = _model(D, policy, score, gen, batch_size=bs)
        c.fit_prepared(ds, tar, T, **dict(kw, **other))
        assert _file(c, tmp_path) != _file(a, tmp_path)


def test_the_first_tree_of_a_softmax_fit_is_all_ties():
    n, D = 4096, 4
    d = _data(n, D)
    m = _model(D)
    ds = m.prepare_dataset(d["X"])
    m.fit_prepared(ds, d["y"], 0, objective="softmax")            # the bias alone
    P = np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (n, 1))
    G, _ = m.objective_gradient(P, d["y"], "softmax")
    r = ds.sample_goss(G, 0.2, 0.1, seed=0, draw=0)
    norms = {G[i].tobytes() for i in range(n)}
    assert len(norms) == D, "the premise: one gradient row per class"
    assert int((r["factor"] == np.float32(1.0)).sum()) == r["n_top"] == n // 5


# ---- 2. validation, warm start -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,score,gen,bs", [("oblivious", "L2", "Quantile", 5000), ("greedy", "Cosine", "Uniform", 700)])
def test_a_goss_fit_with_a_validation_set(policy, score, gen, bs, tmp_path):
    n, nv, D, T, goss, seed = 2000, 333, 3, 6, (0.2, 0.1), 4
    d = _data(n + nv, D)
    X, Xv, Y, Yv = d["X"][:n], d["X"][n:], np.ascontiguousarray(d["real"][:n]), np.ascontiguousarray(d["real"][n:])
    a = _model(D, policy, score, gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    dsv = a.prepare_dataset(Xv, reference=ds)
    r = a.fit_prepared(ds, Y, T, valid=dsv, valid_targets=Yv, goss=goss, seed=seed)
    assert isinstance(r, dict) and r["iterations"] == T and np.asarray(r["valid_loss"]).shape == (T + 1,)
    for k in range(T + 1):
        got = np.asarray(r["valid_loss"], np.float64)[k]
        want = np.asarray(a.staged_loss(Xv, None, Yv, stops=[k]), np.float64)[0]
        print("k = %d  valid_loss %.17g  staged_loss %.17g" % (k, got, want))
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_loss[%d]" % k
    assert r["best_n_trees"] == int(np.argmin(np.asarray(r["valid_loss"])))
    b = _model(D, policy, score, gen, batch_size=bs)
    loss_b = b.fit_prepared(ds, Y, T, goss=goss, seed=seed)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], loss_b)
    # a classifier watched by its metric, with Newton leaves and colsample: the model of the call without the watch
    lab, labv = np.ascontiguousarray(d["y"][:n] % D), np.ascontiguousarray(d["y"][n:] % D)
    kw = dict(objective="softmax", leaf_update="newton", colsample=0.5, goss=goss, seed=seed)
    c = _model(D, policy, score, gen, batch_size=bs)
    rc = c.fit_prepared(ds, lab, T, valid=dsv, valid_targets=labv, eval_metric="error", **kw)
    e = _model(D, policy, score, gen, batch_size=bs)
    loss_e = e.fit_prepared(ds, lab, rc["iterations"], **kw)
    assert _file(c, tmp_path) == _file(e, tmp_path) and _same_bits(rc["loss"], loss_e)


@pytest.mark.parametrize("obj,leaf", [("rmse", "gradient"), ("logistic", "newton")])
def test_a_continued_fit_continues_the_sequence_of_draws(obj, leaf, tmp_path):
    n, D, seed, goss = 1500, 3, 77, (0.1, 0.1)
    d = _data(n, D)
    tar = _targets(obj, d, D)
    kw = dict(objective=obj, leaf_update=leaf, goss=goss, seed=seed)
    a = _model(D, batch_size=700)
    ds = a.prepare_dataset(d["X"])
    a.fit_prepared(ds, tar, 3, **kw)
    loss_a = a.fit_prepared(ds, tar, 4, **kw)
    b = _model(D, batch_size=700)
    loss_b = b.fit_prepared(ds, tar, 7, **kw)
    assert a.get_num_trees() == b.get_num_trees() == 7
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)
    c = _model(D, batch_size=700)
    c.fit_prepared(ds, tar, 7, **dict(kw, seed=seed + 1))
    assert _file(c, tmp_path) != _file(a, tmp_path)


# ---- 3. draws that keep no row --------------------------------------------------------------------------------------------------------------------------
def test_a_draw_that_keeps_no_row_takes_the_whole_batch(tmp_path):
    n, nf, D, goss, seed, T = 8, 3, 2, (0.1, 0.09), 5, 12          # floor(0.1 * 8) == 0 top rows; p = 0.09 / 0.9
    p = np.float64(goss[1]) / (1.0 - np.float64(goss[0]))
    kept = [cpp.sample_rows_host(n, float(p), seed=seed ^ GOSS_STREAM, draw=k).size for k in range(T)]
    assert min(kept) == 0 and max(kept) > 0, "the premise: the draws of this run include an empty and a non-empty one (%s)" % kept
    for obj, leaf in (("rmse", "gradient"), ("logistic", "newton")):
        d = _data(n, D, nf)
        tar = _targets(obj, d, D)
        a = _model(D, depth=2, n_bins=4, n_features=nf)
        ds = a.prepare_dataset(d["X"])
        loss_a = a.fit_prepared(ds, tar, T, objective=obj, leaf_update=leaf, leaf_l2=0.5, goss=goss, seed=seed)
        b = _model(D, depth=2, n_bins=4, n_features=nf)
        loss_b, seen = _manual_loop(b, ds, tar, None, obj, D, 5000, T, a.get_bias(), goss, seed, leaf=leaf)
        assert [m for _, m, _ in seen] == kept and [k for k, _, _ in seen] == list(range(T))
        assert _file(a, tmp_path) == _file(b, tmp_path)
        assert _same_bits(loss_a, loss_b)


# ---- 4. goss=None ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs", [(3000, 1024), (1000, 5000)])
def test_goss_none_is_the_call_without_the_keyword(n, bs, tmp_path):
    D, T = 3, 5
    d = _data(n, D)
    files, losses = [], []
    for kw in ({}, dict(goss=None), dict(goss=None, seed=12345), dict(goss=(0.2, 0.1), seed=12345), dict(subsample=0.3, seed=12345)):
        m = _model(D, batch_size=bs)
        ds = m.prepare_dataset(d["X"])
        m.set_profiling(2)
        losses.append(m.fit_prepared(ds, d["real"], T, **kw))
        phases = m.last_phase_times()
        m.set_profiling(0)
        assert "continue_codes" in phases and "grad_stats" in phases, sorted(phases)
        assert ("sample_goss" in phases) == (kw.get("goss") is not None), sorted(phases)
        assert ("sample_rows" in phases) == ("subsample" in kw), sorted(phases)
        files.append(_file(m, tmp_path))
    assert files[0] == files[1] == files[2] and _same_bits(losses[0], losses[1]) and _same_bits(losses[0], losses[2])
    assert files[3] != files[0] and files[3] != files[4]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_as_it_was(tmp_path):
    n, D = 1000, 3
    d = _data(n, D)
    m = _model(D)
    ds = m.prepare_dataset(d["X"])
    m.fit_prepared(ds, d["real"], 2, goss=(0.2, 0.1))
    before = _file(m, tmp_path)
    for goss in ((float("nan"), 0.1), (0.1, float("nan")), (-0.1, 0.1), (1.0, 0.1), (0.1, 0.0), (0.1, 1.5), (0.6, 0.5), (0.0, 2.0**-25), (0.1,), (0.1, 0.1, 0.1), 0.5):
        with pytest.raises((RuntimeError, TypeError)):
            m.fit_prepared(ds, d["real"], 2, goss=goss)
    with pytest.raises(RuntimeError, match="subsample"):
        m.fit_prepared(ds, d["real"], 2, goss=(0.2, 0.1), subsample=0.5)
    assert 8.0 * 1e4 > 65536 and float(d["w"].max()) == 8.0
    with pytest.raises(RuntimeError, match="65536"):
        m.fit_prepared(ds, d["real"], 2, goss=(0.0, 1e-4), weights=d["w"])
    with pytest.raises(RuntimeError, match="65536"):
        m.fit_prepared(ds, d["real"], 2, goss=(0.0, 1e-5))                       # the amplification alone: 1e5
    assert m.get_num_trees() == 2 and _file(m, tmp_path) == before
    m.fit_prepared(ds, d["real"], 1, goss=(0.0, 1e-4), weights=np.minimum(d["w"], 6.0))   # 6e4 fits
    assert m.get_num_trees() == 3
