"""GBRL.refit_leaves_prepared (include/gbrl_hip.h; gbrl_amd/csrc/refit_codes.hip), every comparison on bytes.  One NumPy oracle restates the rule per
tree: the row's leaf from predict_leaves, g and h from the host rules, int64 sums with np.add.at, newton_values_host or refit_leaves' mean, the decay
mix in float64; the prediction in front of the next tree is the refitted model's own chain, as in test_gpu_refit.py.  Every refit runs through the
streaming kernels and, with GBRL_HIP_CONTINUE_GENERIC=1, the general ones.  The models are grown with fit_prepared on 64 * 9 + 1 rows, never modified."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
N = 64 * 9 + 1


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


def _new(F, D, policy, depth, **kw):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=16, split_score_func="L2", generator_type="Quantile",
                      grow_policy=policy, device="cpu", batch_size=5000, **kw)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.3, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


@functools.lru_cache(maxsize=None)
def _grown(F, D, policy, depth, obj, T):
    rng = np.random.default_rng(100 * F + 10 * D + depth + T + (7 if policy == "greedy" else 0))
    m = _new(F, D, policy, depth)
    X = rng.standard_normal((N, F)).astype(np.float32)
    s = X[:, :1] - 0.5 * X[:, 1:2]
    if obj == "softmax":
        y = ((s[:, 0] + rng.standard_normal(N)) > 0).astype(np.int32) + rng.integers(0, D - 1, N).astype(np.int32)
    elif obj == "logistic":
        y = _shape(((s + rng.standard_normal((N, D))) > 0).astype(np.float32) * 0.75 + 0.125 * rng.random((N, D)).astype(np.float32), D)
    else:
        y = _shape((s + rng.standard_normal((N, D))).astype(np.float32), D)
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, y, T, objective=obj)
    assert m.get_num_trees() == T
    return m, ds, X, y


def _refit(m0, ds, y, generic="0", profiling=0, **kw):
    c = gbrl_amd.GBRL(m0)
    c.set_profiling(profiling)
    os.environ["GBRL_HIP_CONTINUE_GENERIC"] = generic
    try:
        r = c.refit_leaves_prepared(ds, y, **kw)
    finally:
        os.environ.pop("GBRL_HIP_CONTINUE_GENERIC", None)
    return c, r


def _values(m, D):
    return np.asarray(m.get_ensemble_data()["values"], np.float32).reshape(-1, D).copy()


def _oracle(m0, mr, ds, X, y, obj, a, stop, oblivious, leaf_update="gradient", leaf_l2=0.0, decay_rate=0.0, weights=None):
    """the values and counts of the range by the rule; mr is the refitted model, whose chain advances P"""
    ti, dep = (np.asarray(m0.get_ensemble_data()[k]) for k in ("tree_indices", "depths"))
    old = _values(m0, np.asarray(m0.get_bias()).size)
    L, D = old.shape
    n = X.shape[0]
    P = np.tile(np.asarray(m0.get_bias(), np.float32).reshape(1, D), (n, 1))
    P = np.asarray(m0.predict_continue_prepared(ds, _shape(P, D), 0, a)).reshape(n, D) if a else P
    want, counts, first_bits = old.copy(), [], None
    for t in range(a, stop):
        l0, l1 = int(ti[t]), (int(ti[t + 1]) if t + 1 < len(ti) else L)
        depths = np.full(l1 - l0, dep[t], np.int32) if oblivious else dep[l0:l1].astype(np.int32)
        leaf = np.asarray(m0.predict_leaves(X, None, t, t + 1)).reshape(n).astype(np.int64) - l0
        g = cpp.objective_gradient_host(_shape(P, D), y, obj, weights=weights).reshape(n, D)
        if newton := leaf_update == "newton":
            h = cpp.objective_hessian_host(_shape(P, D), None, obj, weights=weights).reshape(n, D)
            bits = cpp.newton_sum_bits(n, None if weights is None else float(weights.max()))
        else:
            gmax = float(np.abs(g).max())
            bits = min(60, math.frexp(4.0e18 / (float(n) * gmax))[1] - 2) if gmax > 0 else 40
        first_bits = bits if first_bits is None else first_bits
        q = lambda x: np.rint(x.astype(np.float64) * 2.0 ** bits).astype(np.int64)
        sums = np.zeros((l1 - l0, (2 if newton else 1) * D + 1), np.int64)
        np.add.at(sums[:, :D], leaf, q(g))
        if newton:
            np.add.at(sums[:, D:2 * D], leaf, q(h))
        np.add.at(sums[:, -1], leaf, 1)
        cnt = sums[:, -1]
        if newton:
            v = cpp.newton_values_host(sums, bits, old[l0:l1], depths, leaf_l2)
        else:
            v = ((sums[:, :D].astype(np.float64) / 2.0 ** bits) / np.maximum(cnt, 1)[:, None].astype(np.float64)).astype(np.float32)
        kept = np.repeat(((cnt == 0) | (depths == 0))[:, None], D, axis=1)
        if newton:
            kept |= ~(sums[:, D:2 * D].astype(np.float64) / 2.0 ** bits + leaf_l2 > 0.0)
        if decay_rate:
            mean = v.astype(np.float64) if newton else (sums[:, :D].astype(np.float64) / 2.0 ** bits) / np.maximum(cnt, 1)[:, None].astype(np.float64)
            v = (np.float64(decay_rate) * old[l0:l1].astype(np.float64) + (1.0 - decay_rate) * mean).astype(np.float32)
        want[l0:l1] = np.where(kept, old[l0:l1], v)
        counts.append(cnt)
        P = np.asarray(mr.predict_continue_prepared(ds, _shape(P, D), t, t + 1)).reshape(n, D)
    return want, np.concatenate(counts), first_bits


def _check(case, a=0, n=N, weights=None, **kw):
    """refit [a, T) on the first n rows through both kernel forms, against the oracle; returns the refitted model, its result and the data"""
    F, D, policy, depth, obj, T = case
    m0, ds, X, y = _grown(*case)
    if n != N:
        X, y = np.ascontiguousarray(X[:n]), np.ascontiguousarray(y[:n])
        ds = m0.prepare_dataset(X, reference=ds)
    w = None if weights is None else np.ascontiguousarray(weights[:n])
    mr, r = _refit(m0, ds, y, objective=obj, start_tree_idx=a, weights=w, **kw)
    mg, rg = _refit(m0, ds, y, generic="1", objective=obj, start_tree_idx=a, weights=w, **kw)
    want, counts, bits = _oracle(m0, mr, ds, X, y, obj, a, T, policy == "oblivious", weights=w, **kw)
    got = _values(mr, D)
    assert got.tobytes() == want.tobytes(), "values differ from the oracle at %s" % np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()
    ti = np.asarray(m0.get_ensemble_data()["tree_indices"])
    assert r["values"].dtype == np.float32 and r["values"].tobytes() == want[ti[a]:].tobytes()
    assert r["counts"].dtype == np.int64 and r["counts"].tobytes() == counts.tobytes() and r["bits"] == bits
    assert _values(mg, D).tobytes() == got.tobytes() and np.float64(rg["loss"]).tobytes() == np.float64(r["loss"]).tobytes(), "the general kernels differ"
    assert np.float64(r["loss"]).tobytes() == np.float64(mr.staged_loss_prepared(ds, y, [T], obj, weights=w)["loss"][0]).tobytes()
    return mr, r, (m0, ds, X, y)


def _file(m, tmp_path):
    p = tmp_path / "m.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


# (F, D, policy, depth, objective, T), first tree, rows -- one case per edge: the 16-column record, the tile, depth 1 (in-wave sums), T = 1, start > 0
NEWTON = [((5, 1, "oblivious", 1, "logistic", 1), 0, 1), ((16, 3, "oblivious", 3, "logistic", 2), 0, 63), ((17, 3, "greedy", 3, "logistic", 5), 1, 64),
          ((17, 3, "oblivious", 3, "softmax", 5), 1, 65), ((16, 4, "greedy", 1, "softmax", 2), 0, N), ((5, 4, "greedy", 3, "softmax", 5), 0, N),
          ((5, 3, "greedy", 1, "logistic", 1), 0, N), ((17, 1, "oblivious", 3, "logistic", 5), 0, N)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,a,n", NEWTON)
def test_newton_is_the_oracle_and_the_public_loop(case, a, n):
    F, D, policy, depth, obj, T = case
    mr, r, (m0, ds, X, y) = _check(case, a, n, leaf_update="newton", leaf_l2=0.5)
    loop = gbrl_amd.GBRL(m0)
    P = _shape(np.tile(np.asarray(m0.get_bias(), np.float32).reshape(1, D), (n, 1)), D)
    P = np.asarray(loop.predict_continue_prepared(ds, P, 0, a)) if a else P
    for t in range(a, T):
        assert loop.newton_leaves_prepared(ds, P, y, obj, leaf_l2=0.5, tree=t)["bits"] == r["bits"]
        P = np.asarray(loop.predict_continue_prepared(ds, P, t, t + 1))
    assert _values(loop, D).tobytes() == _values(mr, D).tobytes()
    _check(case, a, n, leaf_update="newton", leaf_l2=0.5, decay_rate=0.3)


@pytest.mark.gpu
@pytest.mark.parametrize("D,decay_rate", [(1, 0.0), (4, 0.3), (8, 1.0), (8, 0.0)])
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_rmse_gradient_is_refit_leaves(policy, D, decay_rate, tmp_path):
    case = (17, D, policy, 3, "rmse", 5)
    mr, r, (m0, ds, X, y) = _check(case, 1, decay_rate=decay_rate)
    ref = gbrl_amd.GBRL(m0)
    loss = ref.refit_leaves(X, None, y, 1, 0, decay_rate)   # (the float rows behind ds)
    assert _file(ref, tmp_path) == _file(mr, tmp_path) and np.float64(loss).tobytes() == np.float64(r["loss"]).tobytes()
    a = np.asarray(mr.predict(X, None))   # predict, the walk over the codes and a saved and loaded model see the new values
    b = np.asarray(mr.predict_continue_prepared(ds, _shape(np.tile(np.asarray(m0.get_bias(), np.float32).reshape(1, D), (N, 1)), D), 0, 5))
    assert a.tobytes() == b.tobytes() == np.asarray(gbrl_amd.GBRL.load(str(tmp_path / "m.gbrl_model")).predict(X, None)).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case,a,n", [((17, 3, "oblivious", 3, "logistic", 5), 0, N), ((16, 4, "greedy", 3, "softmax", 5), 1, 65), ((5, 1, "greedy", 1, "logistic", 2), 0, 63)])
def test_classifier_gradient_is_the_oracle(case, a, n, tmp_path):
    _check(case, a, n, decay_rate=0.3)
    mr, r, (m0, ds, X, y) = _check(case, a, n)
    if n == N and a == 0:   # on the data and targets of the fit the gradient means are the ones the steps stored
        assert _file(mr, tmp_path) == _file(m0, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_update", ["newton", "gradient"])
@pytest.mark.parametrize("case", [(17, 3, "oblivious", 3, "logistic", 5), (16, 4, "greedy", 3, "softmax", 5)])
def test_weights(case, leaf_update):
    kw = dict(leaf_update=leaf_update, leaf_l2=0.5 if leaf_update == "newton" else 0.0)
    plain, _, _ = _check(case, **kw)
    ones, _, _ = _check(case, weights=np.ones(N, np.float32), **kw)
    assert _values(ones, case[1]).tobytes() == _values(plain, case[1]).tobytes()
    w = (2.0 * np.random.default_rng(5).random(N)).astype(np.float32)
    w[3], w[70] = 0.0, 65536.0   # one exact 0, one weight at the cap
    _check(case, weights=w, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("D,generic,streamed", [(3, "0", 2.0), (3, "1", 0.0), (65, "0", 0.0)])
@pytest.mark.parametrize("obj,leaf_update", [("logistic", "newton"), ("rmse", "gradient")])
def test_the_kernel_form_is_the_one_named(obj, leaf_update, D, generic, streamed):
    case = (16, D, "oblivious", 3, obj, 2)
    _check(case, leaf_update=leaf_update)   # (D = 65: the general form on its own, against the oracle)
    m0, ds, X, y = _grown(*case)
    c, _ = _refit(m0, ds, y, generic, profiling=1, objective=obj, leaf_update=leaf_update)
    assert dict(c.last_phase_times())["refit_streamed_trees"] == streamed


def _stump_in_front():
    """a greedy model whose tree 0 is one leaf of depth 0 (min_data_in_leaf = 60 and a step of 100 rows: no candidate survives), then a real tree"""
    m0, ds, X, y = _grown(5, 3, "greedy", 3, "logistic", 2)
    m = _new(5, 3, "greedy", 3, min_data_in_leaf=60)
    ds2 = m.prepare_dataset(X)
    G = np.ascontiguousarray(np.sign(X[:, :3]).astype(np.float32))
    m.step_prepared(m.prepare_dataset(np.ascontiguousarray(X[:100]), reference=ds2), np.ascontiguousarray(G[:100]))
    m.step_prepared(ds2, G)
    assert np.asarray(m.get_ensemble_data()["tree_indices"]).tolist() == [0, 1]
    return m, ds2


REFUSALS = [("a NaN target", "logistic", dict(), "tree 0"), ("a target of 1.5", "logistic", dict(leaf_update="newton"), r"outside \[0, 1\]"),
            ("clean", "rmse", dict(leaf_update="newton"), "rmse"), ("clean", "quantile", dict(), "quantile"), ("clean", "lambdarank", dict(), "ranking"),
            ("other thresholds", "logistic", dict(), "tree 0"), ("a stump in front", "logistic", dict(start_tree_idx=1), "depth 0"),
            ("clean", "logistic", dict(decay_rate=1.5), "decay_rate")]


@pytest.mark.gpu
@pytest.mark.parametrize("what,obj,kw,match", REFUSALS)
def test_refusals_leave_the_model_bytes(what, obj, kw, match, tmp_path):
    m0, ds, X, y = _grown(5, 3, "greedy", 3, "logistic", 2)
    c, y = gbrl_amd.GBRL(m0), y.copy()
    if "target" in what:
        y[70, 1] = np.nan if "NaN" in what else 1.5
    elif what == "other thresholds":
        ds = c.prepare_dataset(np.ascontiguousarray(2.0 * X + 1.0))
    elif what == "a stump in front":
        c, ds = _stump_in_front()
    keep = _file(c, tmp_path)
    with pytest.raises(RuntimeError, match=match):
        c.refit_leaves_prepared(ds, y, objective=obj, **kw)
    assert _file(c, tmp_path) == keep


def test_refusals_that_need_no_device():
    m, y = _new(4, 2, "oblivious", 2), np.zeros((8, 2), np.float32)
    for kw, match in ((dict(), "data set"), (dict(objective="nonsense"), "objective"), (dict(leaf_update="nonsense"), "leaf_update"), (dict(objective="pairwise"), "ranking")):
        with pytest.raises(RuntimeError, match=match):
            m.refit_leaves_prepared(None, y, **kw)


def test_newton_value_split_on_the_host(tmp_path):   # tests/cxx/newton_core_check.cpp under the address and undefined-behaviour sanitizers
    root, exe = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), tmp_path / "newton_core_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "gbrl_amd", "csrc"),
                    os.path.join(root, "tests", "cxx", "newton_core_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr
