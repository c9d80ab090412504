"""fit_prepared growing every tree on a sample of the columns, on the GPU (GBRL.fit_prepared(ds, Y, T, colsample=, seed=); include/gbrl_hip.h,
"Column subsampling").  Every comparison is exact (file bytes, the bits of the losses):
  * against the loop a caller could write from public calls, with the columns taken from a NumPy restatement of the column rule at draw = the
    tree count: set_bias, predict_continue_prepared of a held prediction, G = P - Y, step_prepared(ds, G, rows=, cols=);
  * together with subsample; with a validation set; warm starts; seeds;
  * colsample = 1.0, and one feature at any colsample, are the call without the keyword and have no gather_cols phase.
"""
import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

U64 = np.uint64
STREAM = 0x636F6C73616D706C


# ---- the two rules, restated from their text (include/gbrl_hip.h) ---------------------------------------------------------------------------------
def restate_u(seed, draw, idx):
    with np.errstate(over="ignore"):
        x = (U64(draw) << U64(32)) | np.asarray(idx, dtype=np.uint64)
        z = x + U64((int(seed) + 1) % 2**64) * U64(0x9E3779B97F4A7C15)
        z ^= z >> U64(30); z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27); z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        return (z >> U64(40)).astype(np.int64)


def restate_rows(n, subsample, seed=0, draw=0, row0=0):
    rows = np.arange(row0, row0 + n, dtype=np.int64)
    return rows[restate_u(seed, draw, rows) < int(np.floor(np.float64(subsample) * 16777216.0))].astype(np.int32)


def restate_cols(F, colsample, seed=0, draw=0):
    k = max(1, int(np.floor(np.float64(colsample) * F + 0.5)))
    f = np.arange(F, dtype=np.int64)
    u = restate_u(int(seed) ^ STREAM, draw, f)
    return np.sort(f[np.lexsort((f, u))[:k]]).astype(np.int32)


# ---- helpers (tests/test_gpu_fit_subsample.py's) ---------------------------------------------------------------------------------------------------
def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, batch_size=5000):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.linspace(0.5, 1.5, F).astype(np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


_DATA = {}


def _data(n, F, D, seed):
    if (n, F, D, seed) not in _DATA:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, F)).astype(np.float32)
        W = rng.standard_normal((F, D)).astype(np.float32)
        Y = (np.tanh(X @ W) + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
        _DATA[(n, F, D, seed)] = (X, Y)
    return _DATA[(n, F, D, seed)]


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


def _manual_loop(m, ds, Y, D, bs, iterations, bias, q, seed, p=1.0):
    """the loop a caller could write; returns the column lists it drew"""
    n, F = Y.shape[0], ds.n_features
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
        cols = restate_cols(F, q, seed, draw=T)
        seen.append(cols)
        rows = whole
        if p < 1.0:
            idx = restate_rows(bn, p, seed, draw=T, row0=start)
            if idx.size:
                rows, G = idx, np.ascontiguousarray(G[idx - start])
        m.step_prepared(ds, G, rows=rows, cols=cols)
    return seen


def _loss_of(m, ds, Y, D):
    """the loss fit_prepared returns for the model as it stands: its own final stage on no further iterations"""
    return m.fit_prepared(ds, _shape(Y, D), 0)


# ---- 1. the loop a caller could write ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 0.5])                                      # alone, and together with row sampling
@pytest.mark.parametrize("q", [0.5, 0.25])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("n,bs,T,F", [(3000, 5000, 6, 20), (1000, 384, 7, 12), (2500, 2048, 5, 17)])   # batch_size = n and < n
def test_a_column_sampled_fit_is_the_loop_a_caller_could_write(n, bs, T, F, policy, score, gen, D, q, p, tmp_path):
    seed = 1000 * D + n
    X, Y = _data(n, F, D, seed=40 + n + D)
    a = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    kw = dict(colsample=q, seed=seed)
    if p < 1.0:
        kw["subsample"] = p
    loss_a = a.fit_prepared(ds, _shape(Y, D), T, **kw)
    assert isinstance(loss_a, float) and a.get_num_trees() == T
    b = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    seen = _manual_loop(b, ds, Y, D, bs, T, a.get_bias(), q, seed, p)
    k = max(1, int(np.floor(q * F + 0.5)))
    assert all(c.size == k and k < F for c in seen) and len({c.tobytes() for c in seen}) > 1, "the premise: proper subsets, not all the same"
    assert _file(a, tmp_path) == _file(b, tmp_path), "the saved files differ (columns: %s)" % [c.tolist() for c in seen]
    assert _same_bits(loss_a, _loss_of(b, ds, Y, D))
    # every tree's features lie in its draw
    e = a.get_ensemble_data()
    fi, depths, ti = np.asarray(e["feature_indices"]).reshape(np.asarray(e["depths"]).size, -1), np.asarray(e["depths"]), np.asarray(e["tree_indices"])
    for s in range(depths.size):
        t = s if policy == "oblivious" else int(np.searchsorted(ti, s, side="right")) - 1
        assert set(fi[s, :depths[s]].tolist()) <= set(seen[t].tolist()), (s, t)
    # and it is not the unsampled fit
    c = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    c.fit_prepared(ds, _shape(Y, D), T)
    assert _file(c, tmp_path) != _file(a, tmp_path)


# ---- 2. colsample = 1.0; one feature ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs", [(3000, 1024), (1000, 5000)])
def test_colsample_one_is_the_call_without_the_keyword(n, bs, tmp_path):
    F, D, T = 13, 3, 5
    X, Y = _data(n, F, D, seed=81)
    files, losses = [], []
    for kw in ({}, dict(colsample=1.0), dict(colsample=1.0, seed=12345), dict(colsample=0.5, seed=12345), dict(colsample=0.5, subsample=0.5, seed=12345)):
        m = _model(F, D, batch_size=bs)
        ds = m.prepare_dataset(X)
        m.set_profiling(2)
        losses.append(m.fit_prepared(ds, Y, T, **kw))
        phases = m.last_phase_times()
        m.set_profiling(0)
        assert "continue_codes" in phases and "grad_stats" in phases, sorted(phases)
        assert ("gather_cols" in phases) == (kw.get("colsample", 1.0) < 1.0), sorted(phases)
        assert ("sample_rows" in phases) == (kw.get("subsample", 1.0) < 1.0), sorted(phases)
        if kw.get("colsample", 1.0) < 1.0:
            assert "gather_codes" not in phases, "rows and columns are gathered in one pass"
        files.append(_file(m, tmp_path))
    assert files[0] == files[1] == files[2] and _same_bits(losses[0], losses[1]) and _same_bits(losses[0], losses[2])
    assert files[3] != files[0] and files[4] != files[3]


@pytest.mark.parametrize("q", [0.01, 0.5, 1.0])
def test_one_feature_is_the_unsubsampled_fit(q, tmp_path):
    n, F, D, T = 800, 1, 2, 4
    X, Y = _data(n, F, D, seed=82)
    a = _model(F, D, batch_size=300)
    ds = a.prepare_dataset(X)
    a.set_profiling(2)
    loss_a = a.fit_prepared(ds, Y, T, colsample=q, seed=5)
    assert "gather_cols" not in a.last_phase_times()
    b = _model(F, D, batch_size=300)
    loss_b = b.fit_prepared(ds, Y, T)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)


# ---- 3. warm start -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 0.5])
def test_a_continued_fit_continues_the_sequence_of_draws(p, tmp_path):
    n, F, D, seed = 1500, 14, 3, 77
    X, Y = _data(n, F, D, seed=60)
    a = _model(F, D, batch_size=5000)
    ds = a.prepare_dataset(X)
    a.fit_prepared(ds, Y, 3, subsample=p, colsample=0.4, seed=seed)
    loss_a = a.fit_prepared(ds, Y, 4, subsample=p, colsample=0.4, seed=seed)
    b = _model(F, D, batch_size=5000)
    loss_b = b.fit_prepared(ds, Y, 7, subsample=p, colsample=0.4, seed=seed)
    assert a.get_num_trees() == b.get_num_trees() == 7
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(loss_a, loss_b)


# ---- 4. validation -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,score,gen,bs", [("oblivious", "L2", "Quantile", 5000), ("greedy", "Cosine", "Uniform", 700)])
def test_a_column_sampled_fit_with_a_validation_set(policy, score, gen, bs, tmp_path):
    n, nv, F, D, T, q, seed = 2000, 333, 15, 3, 6, 0.5, 4
    X, Y = _data(n, F, D, seed=70)
    Xv, Yv = _data(nv, F, D, seed=71)
    a = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    dsv = a.prepare_dataset(Xv, reference=ds)
    r = a.fit_prepared(ds, Y, T, valid=dsv, valid_targets=Yv, colsample=q, seed=seed)
    assert isinstance(r, dict) and r["iterations"] == T and np.asarray(r["valid_loss"]).shape == (T + 1,)
    for k in range(T + 1):
        got = np.asarray(r["valid_loss"], np.float64)[k]
        want = np.asarray(a.staged_loss(Xv, None, Yv, stops=[k]), np.float64)[0]
        print("k = %d  valid_loss %.17g  staged_loss %.17g" % (k, got, want))
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_loss[%d]" % k
    assert r["best_n_trees"] == int(np.argmin(np.asarray(r["valid_loss"])))
    b = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    loss_b = b.fit_prepared(ds, Y, T, colsample=q, seed=seed)
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], loss_b)


# ---- 5. seeds ------------------------------------------------------------------------------------------------------------------------------------
def test_one_seed_one_model_two_seeds_two_models(tmp_path):
    n, F, D, T = 3000, 16, 2, 5
    X, Y = _data(n, F, D, seed=95)
    out = []
    for seed in (2**64 - 1, 2**64 - 1, 6):
        m = _model(F, D, batch_size=1024)
        ds = m.prepare_dataset(X)
        loss = m.fit_prepared(ds, Y, T, colsample=0.25, seed=seed)
        out.append((_file(m, tmp_path), np.float32(loss).tobytes()))
    assert out[0] == out[1]
    assert out[0][0] != out[2][0]
