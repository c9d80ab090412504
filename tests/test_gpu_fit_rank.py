"""fit_prepared(objective="pairwise" | "lambdarank", group=) on the GPU (include/gbrl_hip.h, "Ranking objectives").  tests/test_gpu_rank.py holds
rank_gradient and newton_leaves_prepared(group=) to the host rule; here
  1. the fit is byte for byte -- the saved model file, the loss -- the loop predict_continue_prepared -> rank_gradient -> step_prepared ->
     newton_leaves_prepared(group=) written from the public pieces: both objectives, gradient and Newton leaves, ndcg_at set and unset, oblivious and
     greedy trees, F = 5 and F = 16, the same with colsample = 0.5;
  2. with valid=, valid_group= and early_stopping_rounds, valid_loss[k] is rank_gradient's loss of the validation prediction after k trees, the stop
     and best_n_trees follow early_stop_scan on that curve, and the model is the one the call without valid= leaves at that iteration count;
  3. 5 + 5 iterations leave the bytes of 10; a fresh model's bias is 0;
  4. on a synthetic monotone rule lambdarank with Newton leaves ends with valid_loss[-1] < valid_loss[0];
  5. every refusal leaves the model's file bytes as they were;
  6. a call without the new keywords has no rank phase and the bytes of the call spelt with the keywords at None.
"""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

cpp = gbrl_amd.gbrl_cpp
f32 = np.float32


def _model(F, policy="oblivious", depth=3, n_bins=32, batch_size=5000, D=1):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func="L2", generator_type="Quantile",
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _same_bits(a, b):
    return f32(a).tobytes() == f32(b).tobytes()


def _scan(curve, rounds, min_delta=0.0):
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_early_stop_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(curve, np.float64)
    stop, best = C.c_int(-7), C.c_int(-7)
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, len(c), rounds, min_delta, C.byref(stop), C.byref(best)) == 0
    return stop.value, best.value


_DATA = {}


def _data(n_queries, F, seed):
    """queries of 1 to 40 rows; the relevance (0..4) is a noisy monotone function of the first two features"""
    key = (n_queries, F, seed)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        group = rng.integers(1, 41, n_queries).astype(np.int32)
        group[::7] = 2
        n = int(group.sum())
        X = rng.standard_normal((n, F)).astype(f32)
        z = X[:, 0] + 0.5 * X[:, 1] + 0.5 * rng.standard_normal(n)
        y = np.clip(np.floor((z + 2.0) * 1.25), 0, 4).astype(np.int32)
        _DATA[key] = (X, y, group)
    return _DATA[key]


def _manual_loop(m, ds, y, group, objective, ndcg_at, iterations, leaf, colsample=1.0, seed=0, watch=None, leaf_l2=1.0):
    """predict_continue_prepared -> rank_gradient -> step_prepared -> newton_leaves_prepared(group=); watch = (dsv, yv, groupv, rounds)"""
    n = ds.n_rows
    P = np.full(n, m.get_bias()[0], f32)
    done = m.get_num_trees()
    curve = []

    def evaluate():
        dsv, yv, gv, _ = watch
        base = np.full(dsv.n_rows, m.get_bias()[0], f32)
        Pv = base if m.get_num_trees() == 0 else np.asarray(m.predict_continue_prepared(dsv, base, 0, m.get_num_trees()))
        curve.append(m.rank_gradient(np.ascontiguousarray(Pv), yv, gv, objective, ndcg_at)["loss"])
    if done:
        P = np.asarray(m.predict_continue_prepared(ds, P, 0, done))
    if watch:
        evaluate()
    for _ in range(iterations):
        T = m.get_num_trees()
        if done < T:
            P = np.asarray(m.predict_continue_prepared(ds, np.ascontiguousarray(P), done, T))
            done = T
        r = m.rank_gradient(np.ascontiguousarray(P), y, group, objective, ndcg_at)
        kw = {}
        if colsample < 1.0:
            kw["cols"] = ds.sample_cols(colsample, seed=seed, draw=T)
        m.step_prepared(ds, r["grad"], **kw)
        if leaf == "newton":
            m.newton_leaves_prepared(ds, np.ascontiguousarray(P), y, objective, leaf_l2=leaf_l2, group=group, ndcg_at=ndcg_at)
        if watch:
            evaluate()
            best = int(np.argmin(curve))
            if watch[3] > 0 and len(curve) - 1 - best >= watch[3]:
                break
    T = m.get_num_trees()
    if done < T:
        P = np.asarray(m.predict_continue_prepared(ds, np.ascontiguousarray(P), done, T))
    return m.rank_gradient(np.ascontiguousarray(P), y, group, objective, ndcg_at)["loss"], np.asarray(curve, np.float64)


KINDS = [("pairwise", None), ("lambdarank", None), ("lambdarank", 5)]


@pytest.mark.parametrize("colsample", [1.0, 0.5])
@pytest.mark.parametrize("leaf", ["gradient", "newton"])
@pytest.mark.parametrize("objective,ndcg_at", KINDS)
@pytest.mark.parametrize("F,policy", [(5, "oblivious"), (16, "greedy")])
def test_fit_is_its_manual_loop(tmp_path, F, policy, objective, ndcg_at, leaf, colsample):
    X, y, group = _data(120, F, seed=F)
    assert 1700 <= len(y) <= 3000
    T = 4
    a, b = _model(F, policy), _model(F, policy)
    dsa, dsb = a.prepare_dataset(X), b.prepare_dataset(X)
    kw = dict(colsample=colsample, seed=77) if colsample < 1.0 else {}
    loss = a.fit_prepared(dsa, y, T, objective=objective, group=group, ndcg_at=ndcg_at, leaf_update=leaf, **kw)
    assert a.get_num_trees() == T and a.get_bias()[0] == 0.0
    b.set_bias(np.zeros(1, f32))
    want, _ = _manual_loop(b, dsb, y, group, objective, ndcg_at, T, leaf, colsample=colsample, seed=77)
    assert _file(a, tmp_path) == _file(b, tmp_path)
    assert _same_bits(loss, want), (loss, want)
    assert np.isfinite(loss) and loss > 0


@pytest.mark.parametrize("objective,ndcg_at,leaf", [("pairwise", None, "newton"), ("lambdarank", 10, "gradient"), ("lambdarank", None, "newton")])
def test_validation_and_early_stopping(tmp_path, objective, ndcg_at, leaf):
    F, T, R = 5, 12, 3
    X, y, group = _data(120, F, seed=5)
    Xv, yv, gv = _data(60, F, seed=6)
    a, b, c = _model(F), _model(F), _model(F)
    dsa, dsb, dsc = a.prepare_dataset(X), b.prepare_dataset(X), c.prepare_dataset(X)
    dva, dvb = a.prepare_dataset(Xv, reference=dsa), b.prepare_dataset(Xv, reference=dsb)
    r = a.fit_prepared(dsa, y, T, valid=dva, valid_targets=yv, valid_group=gv, early_stopping_rounds=R, objective=objective, group=group, ndcg_at=ndcg_at,
                       leaf_update=leaf)
    b.set_bias(np.zeros(1, f32))
    want, curve = _manual_loop(b, dsb, y, group, objective, ndcg_at, T, leaf, watch=(dvb, yv, gv, R))
    assert r["valid_loss"].tobytes() == curve.tobytes(), (r["valid_loss"], curve)
    stop_after, best = _scan(curve, R)       # the rule on the curve: the loop ended where it says, the best entry is the one it names
    assert r["iterations"] == len(curve) - 1 == a.get_num_trees() == stop_after and r["best_n_trees"] == best
    assert _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(r["loss"], want)
    # the watch changes nothing: the call without valid= at that iteration count
    c.fit_prepared(dsc, y, r["iterations"], objective=objective, group=group, ndcg_at=ndcg_at, leaf_update=leaf)
    assert _file(c, tmp_path) == _file(a, tmp_path)
    # rounds = 0 records only: the same curve from sums that stayed on the device
    d = _model(F)
    dsd = d.prepare_dataset(X)
    r0 = d.fit_prepared(dsd, y, r["iterations"], valid=d.prepare_dataset(Xv, reference=dsd), valid_targets=yv, valid_group=gv, objective=objective, group=group,
                        ndcg_at=ndcg_at, leaf_update=leaf)
    assert r0["valid_loss"].tobytes() == curve.tobytes()


def test_a_second_call_continues(tmp_path):
    F = 5
    X, y, group = _data(120, F, seed=5)
    kw = dict(objective="lambdarank", group=group, leaf_update="newton")
    a, b = _model(F, "greedy"), _model(F, "greedy")
    dsa, dsb = a.prepare_dataset(X), b.prepare_dataset(X)
    a.fit_prepared(dsa, y, 5, **kw)
    la = a.fit_prepared(dsa, y, 5, **kw)
    lb = b.fit_prepared(dsb, y, 10, **kw)
    assert a.get_num_trees() == 10 and _file(a, tmp_path) == _file(b, tmp_path) and _same_bits(la, lb)
    assert b.get_bias()[0] == 0.0


def test_lambdarank_learns_the_monotone_rule():
    F = 5
    X, y, group = _data(120, F, seed=5)
    Xv, yv, gv = _data(60, F, seed=6)
    m = _model(F, depth=4)
    ds = m.prepare_dataset(X)
    r = m.fit_prepared(ds, y, 30, valid=m.prepare_dataset(Xv, reference=ds), valid_targets=yv, valid_group=gv, objective="lambdarank", group=group, ndcg_at=10,
                       leaf_update="newton")
    print("validation 1 - NDCG@10:", r["valid_loss"][0], "->", r["valid_loss"][-1])
    assert r["valid_loss"][-1] < r["valid_loss"][0]


def test_refusals_leave_the_model_as_it_was(tmp_path):
    F = 5
    X, y, group = _data(120, F, seed=5)
    n = len(y)
    m = _model(F)
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, y, 2, objective="pairwise", group=group)
    before = _file(m, tmp_path)
    dsv = m.prepare_dataset(X[:group[0] + group[1]], reference=ds)
    yv, gv = y[:group[0] + group[1]], group[:2]
    rank = dict(objective="lambdarank", group=group)
    short, long_ = group.copy(), group.copy()
    short[-1] += 1
    long_[3] = 1025
    zero = group.copy(); zero[5] = 0
    bad_y = y.copy(); bad_y[11] = 31
    cases = [
        (dict(objective="lambdarank"), "needs group"),
        (dict(objective="logistic", group=group), "belong to the ranking objectives"),
        (dict(rank, group=short), "sum to %d" % (n + 1)),
        (dict(rank, group=long_), r"group\[3\] = 1025 \(query 3\)"),
        (dict(rank, group=zero), r"group\[5\] = 0 \(query 5\)"),
        (dict(rank, subsample=0.5), "subsample"),
        (dict(rank, goss=(0.2, 0.2)), "goss"),
        (dict(rank, weights=np.ones(n, f32)), "weights"),
        (dict(rank, valid=dsv, valid_targets=yv, valid_group=gv, valid_weights=np.ones(len(yv), f32)), "weights"),
        (dict(rank, alpha=0.5), "alpha"),
        (dict(rank, valid=dsv, valid_targets=yv, valid_group=gv, eval_metric="error"), "eval_metric"),
        (dict(rank, leaf_update="quantile"), "quantile leaf values"),
        (dict(rank, valid=dsv, valid_targets=yv), "valid_group"),
        (dict(rank, valid=dsv, valid_targets=yv, valid_group=[3]), "valid_group sizes sum to 3"),
        (dict(rank, ndcg_at=-1), "ndcg_at"),
        (dict(objective="pairwise", group=group, ndcg_at=5), "ndcg_at"),
    ]
    for kw, what in cases:
        t = y.astype(f32) if kw["objective"] == "logistic" else y
        with pytest.raises(RuntimeError, match=what):
            m.fit_prepared(ds, t, 2, **kw)
    with pytest.raises(RuntimeError, match=r"label 31 \(row 11\)"):
        m.fit_prepared(ds, bad_y, 2, **rank)
    bad_v = yv.copy(); bad_v[1] = -3
    with pytest.raises(RuntimeError, match=r"label -3 \(row 1\)"):
        m.fit_prepared(ds, y, 2, valid=dsv, valid_targets=bad_v, valid_group=gv, **rank)
    with pytest.raises(RuntimeError, match="no pair"):
        m.fit_prepared(ds, np.full(n, 2, np.int32), 2, objective="pairwise", group=group)
    assert _file(m, tmp_path) == before
    # a batch must hold whole queries; a model of two outputs has no score
    small = _model(F, batch_size=n - 1)
    with pytest.raises(RuntimeError, match="batch_size"):
        small.fit_prepared(small.prepare_dataset(X), y, 2, **rank)
    two = _model(F, D=2)
    with pytest.raises(RuntimeError, match="output_dim == 1"):
        two.fit_prepared(two.prepare_dataset(X), y, 2, **rank)
    assert small.get_num_trees() == 0 and two.get_num_trees() == 0
    # and the next call is served
    m.fit_prepared(ds, y, 1, **rank)
    assert m.get_num_trees() == 3


def test_a_call_without_the_keywords_is_what_it_was(tmp_path):
    F, T = 5, 3
    X, y, group = _data(120, F, seed=5)
    t = (y > 1).astype(f32)
    files, losses = [], []
    for kw in ({}, dict(group=None, ndcg_at=None, valid_group=None)):
        m = _model(F)
        ds = m.prepare_dataset(X)
        m.set_profiling(2)
        losses.append(m.fit_prepared(ds, t, T, objective="logistic", leaf_update="newton", **kw))
        phases = m.last_phase_times()
        m.set_profiling(0)
        assert "continue_codes" in phases and "grad_stats" in phases and "newton_leaves" in phases, sorted(phases)
        assert "rank_gradient" not in phases, sorted(phases)
        files.append(_file(m, tmp_path))
    assert files[0] == files[1] and _same_bits(losses[0], losses[1])
    m = _model(F)
    ds = m.prepare_dataset(X)
    m.set_profiling(2)
    m.fit_prepared(ds, y, T, objective="lambdarank", group=group, leaf_update="newton")
    phases = m.last_phase_times()
    m.set_profiling(0)
    assert "rank_gradient" in phases and "continue_codes" in phases and "newton_leaves" in phases, sorted(phases)
