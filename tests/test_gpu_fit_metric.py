"""fit_prepared(eval_metric=) on the GPU (include/gbrl_hip.h, "Classifier metrics"): the validation rows' metric per iteration, counted on the
device behind the validation launch, and the stopping rule on that curve.  Every comparison is exact:
  1. valid_metric[k] is gbrl_cpp.eval_metric_host of predict_continue_prepared(dsv, tiled bias, 0, T0 + k) for every k -- fresh and warm
     starts, one batch and three, with and without row and column samples;
  2. valid_loss, the loss and the saved model are those of the same call without eval_metric, byte for byte;
  3. iterations and best_n_trees are gbrl_hip_early_stop_scan's on the metric curve (the AUC negated), and on a run where the loss curve's
     minimum and the metric curve's best differ it is the metric that decides;
  4. what is refused leaves the model as it was; two runs give the same dicts and bytes.
n = 600 at batch_size 256 is three batches with a last one of 88 rows; the 257 validation rows are four waves and one row."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

host = gbrl_amd.gbrl_cpp.eval_metric_host
N, NV, F, DEPTH = 600, 257, 5, 3
CASES = [("logistic", 1, "error"), ("logistic", 1, "auc"), ("logistic", 3, "error"), ("logistic", 3, "auc"), ("softmax", 4, "error")]
IDS = ["%s-D%d-%s" % c for c in CASES]


def _model(D, bs, lr=0.1):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=32, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cpu", batch_size=bs)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=lr, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


def _rule(curve, rounds, min_delta=0.0):
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_early_stop_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(curve, np.float64)
    stop, best = C.c_int(-1), C.c_int(-1)
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, len(c), rounds, min_delta, C.byref(stop), C.byref(best)) == 0
    return stop.value, best.value


def _score(metric, curve):
    """what the stopping rule sees of a metric curve: the error as it is, the AUC negated"""
    return -np.asarray(curve) if metric == "auc" else np.asarray(curve)


_DATA = {}


def _data(obj, D, seed=0, noise=0.8):
    """training and validation rows of one population: noisy linear scores; logistic: D independent 0 / 1 columns, softmax: the arg-max class"""
    key = (obj, D, seed, noise)
    if key not in _DATA:
        rng = np.random.default_rng(9300 + 17 * seed + D)
        X = rng.standard_normal((N + NV, F)).astype(np.float32)
        S = X @ rng.standard_normal((F, D)).astype(np.float32) + noise * rng.standard_normal((N + NV, D)).astype(np.float32)
        T = np.argmax(S, axis=1).astype(np.int32) if obj == "softmax" else _shape((S > 0.3).astype(np.float32), D)
        _DATA[key] = (X[:N], T[:N], X[N:], T[N:])
    return _DATA[key]


def _prefix_metric(m, dsv, Tv, obj, D, metric, trees):
    base = _shape(np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (NV, 1)), D)
    P = base if trees == 0 else np.asarray(m.predict_continue_prepared(dsv, base, 0, trees))
    return host(np.ascontiguousarray(P).reshape(NV, D), Tv, obj, metric)[0]


def _check_curve(m, dsv, Tv, obj, D, metric, r, T0):
    assert r["eval_metric"] == metric and r["valid_metric"].dtype == np.float64 and r["valid_metric"].shape == (r["iterations"] + 1,)
    for k, got in enumerate(r["valid_metric"]):
        want = _prefix_metric(m, dsv, Tv, obj, D, metric, T0 + k)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_metric[%d] = %r, eval_metric_host gives %r" % (k, got, want)


@pytest.mark.parametrize("bs", [N, 256])
@pytest.mark.parametrize("obj,D,metric", CASES, ids=IDS)
def test_the_curve_is_the_host_metric_of_every_prefix_and_nothing_else_changes(obj, D, metric, bs, tmp_path):
    X, T, Xv, Tv = _data(obj, D)
    iterations = 7
    m = _model(D, bs)
    ds = m.prepare_dataset(X)
    dsv = m.prepare_dataset(Xv, reference=ds)
    r = m.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, objective=obj, eval_metric=metric)
    assert sorted(r) == ["best_n_trees", "eval_metric", "iterations", "loss", "valid_loss", "valid_metric"] and r["iterations"] == iterations
    _check_curve(m, dsv, Tv, obj, D, metric, r, 0)
    assert (r["iterations"], r["best_n_trees"]) == _rule(_score(metric, r["valid_metric"]), 0)
    plain = _model(D, bs)
    rp = plain.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, objective=obj)
    assert sorted(rp) == ["best_n_trees", "iterations", "loss", "valid_loss"]
    assert r["valid_loss"].tobytes() == rp["valid_loss"].tobytes() and np.float32(r["loss"]).tobytes() == np.float32(rp["loss"]).tobytes()
    assert _file(m, tmp_path) == _file(plain, tmp_path), "the metric changed the model"
    # two runs: the same dict, the same bytes
    again = _model(D, bs)
    ra = again.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, objective=obj, eval_metric=metric)
    assert ra["valid_metric"].tobytes() == r["valid_metric"].tobytes() and ra["valid_loss"].tobytes() == r["valid_loss"].tobytes()
    assert (ra["loss"], ra["iterations"], ra["best_n_trees"], ra["eval_metric"]) == (r["loss"], r["iterations"], r["best_n_trees"], r["eval_metric"])
    assert _file(again, tmp_path) == _file(m, tmp_path)


@pytest.mark.parametrize("bs", [N, 256])
@pytest.mark.parametrize("obj,D,metric", CASES, ids=IDS)
def test_samples_and_a_warm_start(obj, D, metric, bs, tmp_path):
    X, T, Xv, Tv = _data(obj, D)
    kw = dict(objective=obj, subsample=0.5, colsample=0.6, seed=11)
    m = _model(D, bs)
    ds = m.prepare_dataset(X)
    dsv = m.prepare_dataset(Xv, reference=ds)
    m.fit_prepared(ds, T, 4, **kw)                                   # T0 = 4 trees, no validation
    T0 = m.get_num_trees()
    assert T0 == 4
    twin = gbrl_amd.GBRL(m)
    r = m.fit_prepared(ds, T, 6, valid=dsv, valid_targets=Tv, eval_metric=metric, **kw)
    _check_curve(m, dsv, Tv, obj, D, metric, r, T0)
    stop_after, best = _rule(_score(metric, r["valid_metric"]), 0)
    assert (r["iterations"], r["best_n_trees"]) == (stop_after, T0 + best) == (6, T0 + best)
    rp = twin.fit_prepared(ds, T, 6, valid=dsv, valid_targets=Tv, **kw)
    assert r["valid_loss"].tobytes() == rp["valid_loss"].tobytes() and np.float32(r["loss"]).tobytes() == np.float32(rp["loss"]).tobytes()
    assert _file(m, tmp_path) == _file(twin, tmp_path), "the metric changed the model"


@pytest.mark.parametrize("bs", [N, 256])
@pytest.mark.parametrize("obj,D,metric", CASES, ids=IDS)
def test_early_stopping_follows_the_metric_curve(obj, D, metric, bs, tmp_path):
    X, T, Xv, Tv = _data(obj, D)
    iterations = 12
    full = _model(D, bs)
    ds = full.prepare_dataset(X)
    dsv = full.prepare_dataset(Xv, reference=ds)
    rf = full.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, objective=obj, eval_metric=metric)
    score = _score(metric, rf["valid_metric"])
    assert (rf["iterations"], rf["best_n_trees"]) == _rule(score, 0)
    stop_after, best = _rule(score, 2)
    s = _model(D, bs)
    rs = s.fit_prepared(ds, T, iterations, valid=dsv, valid_targets=Tv, early_stopping_rounds=2, objective=obj, eval_metric=metric)
    assert (rs["iterations"], rs["best_n_trees"]) == (stop_after, best) and s.get_num_trees() == stop_after
    assert rs["valid_metric"].tobytes() == rf["valid_metric"][:stop_after + 1].tobytes()
    assert rs["valid_loss"].tobytes() == rf["valid_loss"][:stop_after + 1].tobytes()
    cut = _model(D, bs)
    loss_cut = cut.fit_prepared(ds, T, stop_after, objective=obj)
    assert _file(s, tmp_path) == _file(cut, tmp_path) and np.float32(rs["loss"]).tobytes() == np.float32(loss_cut).tobytes()


def test_the_metric_curve_decides_where_the_two_curves_disagree(tmp_path):
    """A run whose loss curve has its minimum at another entry than its error curve: with eval_metric it is the error's entry that best_n_trees
    names and the error's rule that stops the loop, without it the loss's.  The first of a handful of runs that shows it is taken; the steps of
    the later ones are large (init_lr 2 and 8), where the log loss turns up within a few trees while the share of wrong rows stays flat."""
    found = None
    for seed, lr in [(0, 0.1), (1, 0.1), (2, 0.1), (0, 2.0), (1, 2.0), (0, 8.0), (1, 8.0)]:
        X, T, Xv, Tv = _data("logistic", 1, seed=seed, noise=1.5)
        m = _model(1, N, lr=lr)
        ds = m.prepare_dataset(X)
        dsv = m.prepare_dataset(Xv, reference=ds)
        r = m.fit_prepared(ds, T, 12, valid=dsv, valid_targets=Tv, objective="logistic", eval_metric="error")
        by_loss, by_metric = _rule(r["valid_loss"], 0)[1], _rule(r["valid_metric"], 0)[1]
        print("seed %d, init_lr %g: the loss is lowest after %d trees, the error after %d" % (seed, lr, by_loss, by_metric))
        if by_loss != by_metric:
            found = (seed, lr, ds, dsv, T, Tv, r, by_loss, by_metric)
            break
    assert found is not None, "no run among these has its two curves disagree: the case does not show which one decides"
    seed, lr, ds, dsv, T, Tv, r, by_loss, by_metric = found
    assert r["best_n_trees"] == by_metric
    plain = _model(1, N, lr=lr)
    rp = plain.fit_prepared(ds, T, 12, valid=dsv, valid_targets=Tv, objective="logistic")
    assert rp["best_n_trees"] == by_loss and rp["valid_loss"].tobytes() == r["valid_loss"].tobytes()
    # and the stopping rule: each run stops where ITS curve says
    for kw, curve in [(dict(eval_metric="error"), r["valid_metric"]), (dict(), r["valid_loss"])]:
        stop_after, best = _rule(curve, 2)
        s = _model(1, N, lr=lr)
        rs = s.fit_prepared(ds, T, 12, valid=dsv, valid_targets=Tv, objective="logistic", early_stopping_rounds=2, **kw)
        assert (rs["iterations"], rs["best_n_trees"]) == (stop_after, best), kw


def test_refusals_leave_the_model_as_it_was(tmp_path):
    X, T, Xv, Tv = _data("logistic", 3)
    _, Ts, _, Tvs = _data("softmax", 3)
    m = _model(3, N)
    ds = m.prepare_dataset(X)
    dsv = m.prepare_dataset(Xv, reference=ds)
    before = _file(m, tmp_path)
    one_class = Tv.copy()
    one_class[:, 1] = 1.0
    refused = [
        (dict(objective="logistic", eval_metric="error"), T, "eval_metric needs a validation set"),
        (dict(valid=dsv, valid_targets=Tvs, objective="softmax", eval_metric="auc"), Ts, "auc with the softmax objective"),
        (dict(valid=dsv, valid_targets=Tv, objective="rmse", eval_metric="error"), T, "the rmse objective has no metric"),
        (dict(valid=dsv, valid_targets=Tv, eval_metric="auc"), T, "the rmse objective has no metric"),
        (dict(valid=dsv, valid_targets=one_class, objective="logistic", eval_metric="auc"), T, "column 1 of the targets has no negative row"),
        (dict(valid=dsv, valid_targets=1 - one_class, objective="logistic", eval_metric="auc"), T, "column 1 of the targets has no positive row"),
        (dict(valid=dsv, valid_targets=Tv, objective="logistic", eval_metric="logloss"), T, "Invalid metric"),
    ]
    for kw, targets, message in refused:
        with pytest.raises(RuntimeError, match=message):
            m.fit_prepared(ds, targets, 3, **kw)
        assert m.get_num_trees() == 0 and _file(m, tmp_path) == before, "a refused call changed the model: %s" % message
    # a column of one class is no obstacle to the error rate
    r = m.fit_prepared(ds, T, 2, valid=dsv, valid_targets=one_class, objective="logistic", eval_metric="error")
    assert r["valid_metric"].shape == (3,)
