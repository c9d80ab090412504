"""fit_prepared growing every tree on a sample of its batch, on the GPU (GBRL.fit_prepared(ds, Y, T, subsample=, seed=); include/gbrl_hip.h, "Row
subsampling").  Every comparison is exact (file bytes, the bits of the loss):
  * against the loop a caller could write from public calls, with the sample taken from a NumPy restatement of the sampler's rule: set_bias,
    predict_continue_prepared of a held prediction, G = P - Y, rows = the kept rows of the batch at draw = the tree count (the whole batch when
    none is kept), step_prepared(ds, G[rows - start], rows=rows);
  * subsample = 1.0 is the call without the keywords, and has no sampler phase;
  * a data set so small that draws keep no row; warm starts; a validation set; seeds.
"""
import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

U64 = np.uint64


# ---- the sampler's rule, restated from its text (include/gbrl_hip.h) ---------------------------------------------------------------------------
def restate_sample(n, subsample, seed=0, draw=0, row0=0):
    rows = np.arange(row0, row0 + n, dtype=np.int64)
    with np.errstate(over="ignore"):
        x = (U64(draw) << U64(32)) | rows.astype(np.uint64)
        z = x + U64((int(seed) + 1) % 2**64) * U64(0x9E3779B97F4A7C15)
        z ^= z >> U64(30); z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27); z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        u = (z >> U64(40)).astype(np.int64)
    return rows[u < int(np.floor(np.float64(subsample) * 16777216.0))].astype(np.int32)


# ---- helpers (tests/test_gpu_fit_prepared.py's) -------------------------------------------------------------------------------------------------
def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, batch_size=5000):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _data(n, F, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    W = rng.standard_normal((F, D)).astype(np.float32)
    Y = (np.tanh(X @ W) + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    return X, Y


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 else np.ascontiguousarray(A)


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


def _manual_loop(m, ds, Y, D, bs, iterations, bias, p, seed):
    """the loop a caller could write; returns the draws it saw as (draw, rows kept)"""
    n = Y.shape[0]
    Ys = _shape(Y, D)
    if bias is not None:
        m.set_bias(np.asarray(bias, np.float32))
    P = _shape(np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (n, 1)), D)
    through, seen = {}, []
    for start, bn in _batches(n, bs, iterations):
        sl = slice(start, start + bn)
        T = m.get_num_trees()
        a = through.get(start, 0)
        whole = None if bn == n else np.arange(start, start + bn, dtype=np.int32)
        if a < T:
            P[sl] = np.asarray(m.predict_continue_prepared(ds, np.ascontiguousarray(P[sl]), a, T, rows=whole))
        through[start] = T
        G = np.ascontiguousarray((P[sl] - Ys[sl]).astype(np.float32))
        idx = restate_sample(bn, p, seed, draw=T, row0=start)
        seen.append((T, idx.size))
        if idx.size == 0:
            m.step_prepared(ds, G, rows=whole)
        else:
            m.step_prepared(ds, np.ascontiguousarray(G[idx - start]), rows=idx)
    return seen


def _loss_of(m, ds, Y, D):
    """the loss fit_prepared returns for the model as it stands: its own final stage on no further iterations; checked against NumPy loosely"""
    loss = m.fit_prepared(ds, _shape(Y, D), 0)
    n = Y.shape[0]
    P = np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (n, 1))
    P = np.asarray(m.predict_continue_prepared(ds, _shape(P, D), 0, m.get_num_trees())).reshape(n, D)
    ref = np.sqrt(0.5 * np.sum((P.astype(np.float64) - Y) ** 2) / n)
    assert abs(loss - ref) <= 1e-5 * max(1.0, ref), (loss, ref)
    return loss


# ---- 1. the loop a caller could write --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("D", [1, 8])
@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("n,bs,T", [(4096, 5000, 6), (1000, 384, 7), (4100, 4096, 5)])
def test_a_sampled_fit_is_the_loop_a_caller_could_write(n, bs, T, policy, score, gen, D, p, tmp_path):
    F, seed = 7, 1000 * D + n
    X, Y = _data(n, F, D, seed=40 + n + D)
    a = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, _shape(Y, D), T, subsample=p, seed=seed)
    assert isinstance(loss_a, float) and a.get_num_trees() == T
    b = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    seen = _manual_loop(b, ds, Y, D, bs, T, a.get_bias(), p, seed)
    # (the 4-row batch of n = 4100 may keep no row at 0.1: the loop then takes the batch, as the call must)
    assert all(k < bn for (_, k), (_, bn) in zip(seen, _batches(n, bs, T)) if bn > 64), "the premise: the large batches are sampled"
    assert any(0 < k for _, k in seen)
    assert _file(a, tmp_path) == _file(b, tmp_path), "the saved files differ (draws: %s)" % seen
    loss_b = _loss_of(b, ds, Y, D)
    assert _same_bits(loss_a, loss_b), "loss %r != %r" % (loss_a, loss_b)
    # and it is not the unsampled fit
    c = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    c.fit_prepared(ds, _shape(Y, D), T)
    assert _file(c, tmp_path) != _file(a, tmp_path)


# ---- 2. subsample = 1.0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs", [(3000, 1024), (1000, 5000)])
def test_subsample_one_is_the_call_without_the_keywords(n, bs, tmp_path):
    F, D, T = 9, 3, 5
    X, Y = _data(n, F, D, seed=81)
    files, losses = [], []
    for kw in ({}, dict(subsample=1.0), dict(subsample=1.0, seed=12345), dict(subsample=0.5, seed=12345)):
        m = _model(F, D, batch_size=bs)
        ds = m.prepare_dataset(X)
        m.set_profiling(2)
        losses.append(m.fit_prepared(ds, Y, T, **kw))
        phases = m.last_phase_times()
        m.set_profiling(0)
        assert "continue_codes" in phases and "grad_stats" in phases, sorted(phases)
        assert ("sample_rows" in phases) == (kw.get("subsample", 1.0) < 1.0), sorted(phases)
        files.append(_file(m, tmp_path))
    assert files[0] == files[1] == files[2] and _same_bits(losses[0], losses[1]) and _same_bits(losses[0], losses[2])
    assert files[3] != files[0]


# ---- 3. draws that keep no row ----------------------------------------------------------------------------------------------------------------
def test_a_draw_that_keeps_no_row_takes_the_whole_batch(tmp_path):
    n, F, D, p, seed, T = 8, 3, 2, 0.1, 5, 12
    kept = [restate_sample(n, p, seed, draw=d).size for d in range(40)]
    assert sum(1 for k in kept if k == 0) == 19, "the premise: 19 of the draws 0 to 39 keep no row of 8"
    assert min(kept[:T]) == 0 and max(kept[:T]) > 0, "the premise: the draws of this run include an empty and a non-empty one"
    X, Y = _data(n, F, D, seed=90)
    a = _model(F, D, depth=2, n_bins=4)
    ds = a.prepare_dataset(X)
    loss_a = a.fit_prepared(ds, Y, T, subsample=p, seed=seed)
    b = _model(F, D, depth=2, n_bins=4)
    seen = _manual_loop(b, ds, Y, D, 5000, T, a.get_bias(), p, seed)
    assert [k for _, k in seen] == kept[:T] and [d for d, _ in seen] == list(range(T))
    assert _file(a, tmp_path) == _file(b, tmp_path)
    assert _same_bits(loss_a, _loss_of(b, ds, Y, D))


# ---- 4. warm start -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_a_continued_fit_continues_the_sequence_of_draws(p, tmp_path):
    n, F, D, seed = 1500, 7, 3, 77
    X, Y = _data(n, F, D, seed=60)
    a = _model(F, D, batch_size=5000)
    ds = a.prepare_dataset(X)
    a.fit_prepared(ds, Y, 3, subsample=p, seed=seed)
    loss_a = a.fit_prepared(ds, Y, 4, subsample=p, seed=seed)
    b = _model(F, D, batch_size=5000)
    loss_b = b.fit_prepared(ds, Y, 7, subsample=p, seed=seed)
    assert a.get_num_trees() == b.get_num_trees() == 7
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)


# ---- 5. validation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,score,gen,bs", [("oblivious", "L2", "Quantile", 5000), ("greedy", "Cosine", "Uniform", 700)])
def test_a_sampled_fit_with_a_validation_set(policy, score, gen, bs, tmp_path):
    n, nv, F, D, T, p, seed = 2000, 333, 7, 3, 6, 0.5, 4
    X, Y = _data(n, F, D, seed=70)
    Xv, Yv = _data(nv, F, D, seed=71)
    a = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    dsv = a.prepare_dataset(Xv, reference=ds)
    r = a.fit_prepared(ds, Y, T, valid=dsv, valid_targets=Yv, subsample=p, seed=seed)
    assert isinstance(r, dict) and r["iterations"] == T and np.asarray(r["valid_loss"]).shape == (T + 1,)
    T0 = 0
    for k in range(T + 1):
        got = np.asarray(r["valid_loss"], np.float64)[k]
        want = np.asarray(a.staged_loss(Xv, None, Yv, stops=[T0 + k]), np.float64)[0]
        print("k = %d  valid_loss %.17g  staged_loss %.17g" % (k, got, want))
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_loss[%d]" % k
    assert r["best_n_trees"] == T0 + int(np.argmin(np.asarray(r["valid_loss"])))
    b = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    loss_b = b.fit_prepared(ds, Y, T, subsample=p, seed=seed)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], loss_b)
    # a stopping rule ends the sampled loop as it ends the unsampled one: the model is the one of `iterations` iterations
    c = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    rc = c.fit_prepared(ds, Y, 40, valid=dsv, valid_targets=Yv, early_stopping_rounds=1, min_delta=0.05, subsample=p, seed=seed)
    assert 1 <= rc["iterations"] < 40, "the premise: an improvement of 0.05 per iteration does not last 40 iterations"
    d = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    loss_d = d.fit_prepared(ds, Y, rc["iterations"], subsample=p, seed=seed)
    assert _file(c, tmp_path) == _file(d, tmp_path) and _same_bits(rc["loss"], loss_d)


# ---- 6. seeds ----------------------------------------------------------------------------------------------------------------------------------
def test_one_seed_one_model_two_seeds_two_models(tmp_path):
    n, nv, F, D, T = 3000, 400, 9, 2, 5
    X, Y = _data(n, F, D, seed=95)
    Xv, Yv = _data(nv, F, D, seed=96)
    out = []
    for seed in (2**64 - 1, 2**64 - 1, 6):
        m = _model(F, D, batch_size=1024)
        ds = m.prepare_dataset(X)
        dsv = m.prepare_dataset(Xv, reference=ds)
        r = m.fit_prepared(ds, Y, T, valid=dsv, valid_targets=Yv, early_stopping_rounds=4, subsample=0.25, seed=seed)
        out.append((_file(m, tmp_path), np.float32(r["loss"]).tobytes(), np.asarray(r["valid_loss"]).tobytes(), r["iterations"], r["best_n_trees"]))
    assert out[0] == out[1]
    assert out[0][0] != out[2][0]
