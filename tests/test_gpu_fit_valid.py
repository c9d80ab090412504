"""fit_prepared watching a validation set, on the GPU (GBRL.fit_prepared(ds, Y, T, valid=, valid_targets=, early_stopping_rounds=, min_delta=);
include/gbrl_hip.h: gbrl_hip_fit_prepared_valid).  Every comparison is exact (bytes):
  * valid_loss[k] against staged_loss(Xv, None, Yv, stops=[T0 + k])[0] for every k, on a fresh model and on a warm start, through the streaming
    kernel and with GBRL_HIP_CONTINUE_GENERIC=1 (D = 65 takes the general kernel either way);
  * the model's file bytes and 'loss' against fit_prepared(ds, Y, iterations run) on a twin model;
  * a stop that is guaranteed (targets mirrored about the bias), a loop that cannot stop, a stop in the middle predicted from the recorded curve;
  * iterations / best_n_trees against gbrl_hip_early_stop_scan and a three-line restatement of the rule, in every case;
  * determinism, and the refusal of a validation set with thresholds of its own.
"""
import ctypes as C
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

F, T = 17, 12


def _model(D, policy, batch_size, depth=3):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=32, split_score_func="L2" if policy == "oblivious" else "Cosine",
                      generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _data(n, nv, D, seed):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((F, D)).astype(np.float32)
    def draw(rows):
        X = rng.standard_normal((rows, F)).astype(np.float32)
        return X, (np.tanh(X @ W) + 0.3 * rng.standard_normal((rows, D))).astype(np.float32)
    return draw(n) + draw(nv)


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 else np.ascontiguousarray(A)


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


def _rule(curve, rounds, min_delta=0.0):
    best = 0
    for k in range(1, len(curve)):
        best = k if curve[k] < curve[best] - min_delta else best
        if rounds > 0 and k - best >= rounds:
            return k, best
    return len(curve) - 1, best


def _scan(curve, rounds, min_delta=0.0):
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_early_stop_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(curve, np.float64)
    stop, best = C.c_int(-7), C.c_int(-7)
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, len(c), rounds, min_delta, C.byref(stop), C.byref(best)) == 0
    return stop.value, best.value


def _check_result(r, T0, rounds, min_delta=0.0):
    """the shape of the dict, and the rule applied to the curve it returns"""
    assert sorted(r) == ["best_n_trees", "iterations", "loss", "valid_loss"]
    vl = r["valid_loss"]
    assert vl.dtype == np.float64 and vl.shape == (r["iterations"] + 1,) and isinstance(r["loss"], float)
    want = _rule(vl.tolist(), rounds, min_delta)
    assert _scan(vl, rounds, min_delta) == want
    assert (r["iterations"], r["best_n_trees"]) == (want[0], T0 + want[1]), (r["iterations"], r["best_n_trees"], want, vl.tolist())


def _check_curve(m, r, T0, Xv, Yv, D):
    for k, got in enumerate(r["valid_loss"]):
        want = np.asarray(m.staged_loss(Xv, None, _shape(Yv, D), stops=[T0 + k]), np.float64)[0]
        print("k = %d  valid_loss %.17g  staged_loss %.17g" % (k, got, want))
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), "valid_loss[%d] = %r, staged_loss(stops=[%d]) = %r" % (k, got, T0 + k, want)


CASES = [
    # n, n_v, D, batch_size (None: n), policy
    (257, 65, 1, None, "oblivious"),
    (257, 1000, 3, 100, "greedy"),
    (4097, 65, 8, 100, "oblivious"),
    (4097, 1000, 65, None, "greedy"),       # D = 65: the general kernel
    (257, 1000, 65, 100, "oblivious"),
    (4097, 65, 3, None, "greedy"),
    (4097, 1000, 1, 100, "greedy"),
    (257, 65, 8, None, "greedy"),
]


@pytest.mark.parametrize("n,nv,D,bs,policy", CASES)
def test_curve_model_and_loss(n, nv, D, bs, policy, tmp_path):
    bs = bs or n
    X, Y, Xv, Yv = _data(n, nv, D, seed=500 + n + nv + D)
    a = _model(D, policy, bs)
    ds = a.prepare_dataset(X)
    dsv = a.prepare_dataset(Xv, reference=ds)
    assert dsv.thresholds_id == ds.thresholds_id
    # ---- a fresh model, record only
    r = a.fit_prepared(ds, _shape(Y, D), T, valid=dsv, valid_targets=_shape(Yv, D))
    _check_result(r, 0, 0)
    assert r["iterations"] == T and a.get_num_trees() == T
    assert np.asarray(a.get_ensemble_data()["depths"]).max() >= 2
    _check_curve(a, r, 0, Xv, Yv, D)
    twin = _model(D, policy, bs)
    loss = twin.fit_prepared(ds, _shape(Y, D), T)
    assert _file(a, tmp_path) == _file(twin, tmp_path), "the validation pass changed the model"
    assert np.float32(r["loss"]).tobytes() == np.float32(loss).tobytes()
    # ---- the general kernel gives the same curve and the same model
    with _env("GBRL_HIP_CONTINUE_GENERIC", "1"):
        g = _model(D, policy, bs)
        rg = g.fit_prepared(ds, _shape(Y, D), T, valid=dsv, valid_targets=_shape(Yv, D))
    assert rg["valid_loss"].tobytes() == r["valid_loss"].tobytes() and _file(g, tmp_path) == _file(a, tmp_path)
    assert np.float32(rg["loss"]).tobytes() == np.float32(r["loss"]).tobytes()
    # ---- a stop in the middle, predicted from the recorded curve: a min_delta that only some of the gains reach
    gains = -np.diff(r["valid_loss"])
    delta = float(np.sort(gains)[len(gains) // 2]) if (gains > 0).all() else 0.0
    stop_after, best = _rule(r["valid_loss"].tolist(), 2, delta)
    s = _model(D, policy, bs)
    rs = s.fit_prepared(ds, _shape(Y, D), T, valid=dsv, valid_targets=_shape(Yv, D), early_stopping_rounds=2, min_delta=delta)
    _check_result(rs, 0, 2, delta)
    assert (rs["iterations"], rs["best_n_trees"]) == (stop_after, best) and s.get_num_trees() == stop_after
    assert rs["valid_loss"].tobytes() == r["valid_loss"][:stop_after + 1].tobytes()
    twin_s = _model(D, policy, bs)
    loss_s = twin_s.fit_prepared(ds, _shape(Y, D), stop_after)
    assert _file(s, tmp_path) == _file(twin_s, tmp_path) and np.float32(rs["loss"]).tobytes() == np.float32(loss_s).tobytes()
    # ---- a warm start: T0 = T, the bias kept
    r2 = a.fit_prepared(ds, _shape(Y, D), 3, valid=dsv, valid_targets=_shape(Yv, D), early_stopping_rounds=3)
    _check_result(r2, T, 3)
    assert a.get_num_trees() == T + r2["iterations"]
    assert np.float64(r2["valid_loss"][0]).tobytes() == np.float64(r["valid_loss"][T]).tobytes()
    _check_curve(a, r2, T, Xv, Yv, D)
    loss2 = twin.fit_prepared(ds, _shape(Y, D), r2["iterations"])
    assert _file(a, tmp_path) == _file(twin, tmp_path) and np.float32(r2["loss"]).tobytes() == np.float32(loss2).tobytes()


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("n,D", [(257, 3), (4097, 8)])
def test_a_stop_that_is_guaranteed_and_a_loop_that_cannot_stop(n, D, policy, tmp_path):
    X, Y, _, _ = _data(n, 1, D, seed=600 + n)
    m = _model(D, policy, n)                                     # batch_size >= n: every tree is grown on every row
    ds = m.prepare_dataset(X)
    # targets mirrored about the bias: a leaf value is the mean of the raw gradients, so the first tree moves every leaf with a non-zero mean
    # away from them, and a tree that changes nothing leaves the loss equal -- entry 1 does not improve
    mirrored = (2.0 * Y.mean(axis=0, dtype=np.float64) - Y).astype(np.float32)
    r = m.fit_prepared(ds, _shape(Y, D), T, valid=ds, valid_targets=_shape(mirrored, D), early_stopping_rounds=1)
    _check_result(r, 0, 1)
    assert r["iterations"] == 1 and r["best_n_trees"] == 0 and m.get_num_trees() == 1, r
    twin = _model(D, policy, n)
    loss = twin.fit_prepared(ds, _shape(Y, D), 1)
    assert _file(m, tmp_path) == _file(twin, tmp_path) and np.float32(r["loss"]).tobytes() == np.float32(loss).tobytes()
    # the training rows as their own validation set: the first tree lowers the loss, so k - best never reaches T
    c = _model(D, policy, n)
    rc = c.fit_prepared(ds, _shape(Y, D), T, valid=ds, valid_targets=_shape(Y, D), early_stopping_rounds=T)
    _check_result(rc, 0, T)
    assert rc["iterations"] == T and c.get_num_trees() == T


def test_two_runs_give_the_same_dicts_and_bytes(tmp_path):
    n, nv, D = 3000, 700, 4
    X, Y, Xv, Yv = _data(n, nv, D, seed=700)
    out = []
    for _ in range(2):
        m = _model(D, "greedy", 1024)
        ds = m.prepare_dataset(X)
        dsv = m.prepare_dataset(Xv, reference=ds)
        r = m.fit_prepared(ds, Y, 6, valid=dsv, valid_targets=Yv, early_stopping_rounds=4, min_delta=1e-4)
        _check_result(r, 0, 4, 1e-4)
        out.append((r["valid_loss"].tobytes(), np.float32(r["loss"]).tobytes(), r["iterations"], r["best_n_trees"], _file(m, tmp_path)))
    assert out[0] == out[1]


def test_a_validation_set_with_thresholds_of_its_own_is_refused(tmp_path):
    n, nv, D = 300, 90, 2
    X, Y, Xv, Yv = _data(n, nv, D, seed=800)
    m = _model(D, "oblivious", n)
    ds = m.prepare_dataset(X)
    own = m.prepare_dataset(Xv)
    assert own.thresholds_id != ds.thresholds_id
    before = _file(m, tmp_path)
    with pytest.raises(RuntimeError, match="reference="):
        m.fit_prepared(ds, Y, 3, valid=own, valid_targets=Yv)
    with pytest.raises(RuntimeError, match="valid_targets"):
        m.fit_prepared(ds, Y, 3, valid=ds)
    with pytest.raises(RuntimeError, match="Expected valid_targets of shape"):
        m.fit_prepared(ds, Y, 3, valid=ds, valid_targets=Yv)
    with pytest.raises(RuntimeError, match="early_stopping_rounds"):
        m.fit_prepared(ds, Y, 3, valid=ds, valid_targets=Y, early_stopping_rounds=-1)
    with pytest.raises(RuntimeError, match="min_delta"):
        m.fit_prepared(ds, Y, 3, valid=ds, valid_targets=Y, min_delta=float("nan"))
    assert m.get_num_trees() == 0 and _file(m, tmp_path) == before
    bound = m.prepare_dataset(Xv, reference=ds)
    r = m.fit_prepared(ds, Y, 2, valid=bound, valid_targets=Yv)
    assert r["iterations"] == 2 and m.get_num_trees() == 2
