"""GBRL.newton_leaves_prepared on the GPU (include/gbrl_hip.h, "Newton leaf values"; gbrl_amd/csrc/newton.hip) against NumPy, integers compared
exactly.  tests/test_newton_host.py holds the hessian and the value rule to float64; here a tree or two are grown with step_prepared, the rows are
routed with predict_leaves on the observations, g and h come from the host rules, are quantised and summed in NumPy int64, and
  1. sums, bits and values are equal with no tolerance, through the streaming kernel and the general one, which return the same bytes;
  2. the model holds those values for that tree and every other tree is untouched; predict sees them (the mirror was sent again);
  3. rows= (duplicates, a permutation subset) indexes pred and targets by position; tree=0 of two trees takes the tiled bias;
  4. what the kernel refuses (a target outside [0, 1], a NaN target, a prediction that is not finite) leaves the model bytes as they were.
"""
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

cpp = gbrl_amd.gbrl_cpp


def _model(F, D, policy, depth, n_bins=16):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func="L2", generator_type="Quantile",
                      grow_policy=policy, device="cpu", batch_size=5000)
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


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


N_GROW = 200   # the trees are grown on this many rows; the sums are taken on the first n of them (a data set bound to the same thresholds)
_CASES = {}


def _case(F, D, policy, depth, obj, trees=1):
    """a model of `trees` trees grown on the objective's gradient, its data, and the prediction in front of every tree"""
    key = (F, D, policy, depth, obj, trees)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * F + 10 * D + depth + (7 if policy == "greedy" else 0))
        X = rng.standard_normal((N_GROW, F)).astype(np.float32)
        if obj == "softmax":
            T = rng.integers(0, D, N_GROW).astype(np.int32)
        else:
            T = (rng.random((N_GROW, D)) < 0.4).astype(np.float32)
            T[::7] = rng.random((len(T[::7]), D)).astype(np.float32)   # soft targets inside (0, 1) too
        m = _model(F, D, policy, depth)
        m.set_bias(rng.normal(0.0, 0.5, D).astype(np.float32))
        ds = m.prepare_dataset(X)
        P = np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (N_GROW, 1))
        before = []
        for t in range(trees):
            before.append(P.copy())
            G = cpp.objective_gradient_host(_shape(P, D), _shape(T, D) if obj != "softmax" else T, obj).reshape(N_GROW, D)
            # a signal the tree can split on, whatever the targets: the gradient plus a step along the first two features
            G = (G + 0.5 * np.sign(X[:, :1]) + 0.25 * np.sign(X[:, 1:2])).astype(np.float32)
            m.step_prepared(ds, _shape(G, D))
            P = np.asarray(m.predict_continue_prepared(ds, _shape(P, D), t, t + 1)).reshape(N_GROW, D)
        _CASES[key] = (m, ds, X, T, before)
    return _CASES[key]


def _is_oblivious(policy):
    return policy == "oblivious"


def _check(m, ds_n, Xn, pred, T, obj, D, tree, leaf_l2, policy, rows=None):
    """both kernel families against NumPy; returns the model's values afterwards"""
    sel = np.arange(Xn.shape[0]) if rows is None else rows
    ens0 = m.get_ensemble_data()
    ti = np.asarray(ens0["tree_indices"])
    leaf0 = int(ti[tree])
    leaf1 = int(ti[tree + 1]) if tree + 1 < len(ti) else int(np.asarray(ens0["values"]).shape[0])
    NL = leaf1 - leaf0
    dep = np.asarray(ens0["depths"])
    depths = np.full(NL, dep[tree], np.int32) if _is_oblivious(policy) else dep[leaf0:leaf1].astype(np.int32)
    n = len(sel)
    leaves = np.asarray(m.predict_leaves(np.ascontiguousarray(Xn[sel]), None, tree, tree + 1)).reshape(n) - leaf0
    g = cpp.objective_gradient_host(_shape(pred, D), T, obj).reshape(n, D)
    h = cpp.objective_hessian_host(_shape(pred, D), None, obj).reshape(n, D)
    bits = min(40, 62 - int(n).bit_length())
    q = lambda x: np.rint(x.astype(np.float64) * 2.0 ** bits).astype(np.int64)
    sums = np.zeros((NL, 2 * D + 1), np.int64)
    ok = (leaves >= 0) & (leaves < NL)
    np.add.at(sums[:, :D], leaves[ok], q(g)[ok])
    np.add.at(sums[:, D:2 * D], leaves[ok], q(h)[ok])
    np.add.at(sums[:, 2 * D], leaves[ok], 1)
    old = np.asarray(ens0["values"], np.float32).reshape(-1, D).copy()
    want = cpp.newton_values_host(sums, bits, old[leaf0:leaf1], depths, leaf_l2)
    kw = {} if rows is None else {"rows": np.asarray(rows, np.int32)}
    got = []
    for generic in ("0", "1"):   # the streaming kernel and the general one
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            r = m.newton_leaves_prepared(ds_n, _shape(pred, D), T, obj, leaf_l2=leaf_l2, tree=tree, **kw)
        assert sorted(r) == ["bits", "sums", "values"]
        assert r["sums"].dtype == np.int64 and r["sums"].shape == (NL, 2 * D + 1) and r["values"].dtype == np.float32 and r["values"].shape == (NL, D)
        assert r["bits"] == bits
        assert r["sums"].tobytes() == sums.tobytes(), "generic = %s: the sums differ from NumPy's\n%r\n%r" % (generic, r["sums"], sums)
        assert r["values"].tobytes() == want.tobytes(), "generic = %s: the values differ" % generic
        now = np.asarray(m.get_ensemble_data()["values"], np.float32).reshape(-1, D)
        assert now[leaf0:leaf1].tobytes() == want.tobytes()
        assert now[:leaf0].tobytes() == old[:leaf0].tobytes() and now[leaf1:].tobytes() == old[leaf1:].tobytes(), "another tree's values changed"
        got.append((r["sums"].tobytes(), r["values"].tobytes()))
    assert got[0] == got[1]
    assert int(sums[:, 2 * D].sum()) == int(ok.sum()) and (NL == 1 or ok.all())
    return want


SHAPES = [(n, 17, 3) for n in (1, 63, 64, 65, 200)] + [(200, 16, 3), (200, 40, 3)] + [(65, 16, 1), (65, 16, 8), (65, 16, 65)]


CASES = [(n, F, D, obj) for (n, F, D) in SHAPES for obj in ("logistic", "softmax") if obj == "logistic" or D >= 2]


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("n,F,D,obj", CASES)
def test_sums_and_values_are_numpys(n, F, D, obj, depth, policy):
    m, ds, X, T, before = _case(F, D, policy, depth, obj)
    assert m.get_num_trees() == 1
    Xn = np.ascontiguousarray(X[:n])
    ds_n = ds if n == N_GROW else m.prepare_dataset(Xn, reference=ds)
    Tn = np.ascontiguousarray(T[:n]) if obj == "softmax" else _shape(T[:n], D)
    leaf_l2 = 1.0 if depth == 1 else 0.25
    _check(m, ds_n, Xn, before[0][:n], Tn, obj, D, 0, leaf_l2, policy)


@pytest.mark.parametrize("obj,D", [("logistic", 3), ("softmax", 4)])
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_rows_index_pred_by_position(policy, obj, D):
    m, ds, X, T, before = _case(17, D, policy, 3, obj)
    rng = np.random.default_rng(3)
    for rows in (np.int32([5, 5, 7, 0, 199, 5, 64, 63]), rng.permutation(N_GROW)[:131].astype(np.int32)):
        pred = np.ascontiguousarray(before[0][rows])
        Tn = np.ascontiguousarray(T[rows]) if obj == "softmax" else _shape(T[rows], D)
        _check(m, ds, X, pred, Tn, obj, D, 0, 1.0, policy, rows=rows)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_tree_zero_of_two_and_the_last(policy, tmp_path):
    D, obj = 3, "logistic"
    m, ds, X, T, before = _case(16, D, policy, 3, obj, trees=2)
    assert m.get_num_trees() == 2
    bias = np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (N_GROW, 1))
    assert before[0].tobytes() == bias.tobytes()
    _check(m, ds, X, before[0], _shape(T, D), obj, D, 0, 1.0, policy)            # pred = the tiled bias
    # tree 1 at the prediction over the NEW tree 0; tree = -1 names it
    P1 = np.asarray(m.predict_continue_prepared(ds, bias, 0, 1)).reshape(N_GROW, D)
    want = _check(m, ds, X, P1, _shape(T, D), obj, D, 1, 0.5, policy)
    r = m.newton_leaves_prepared(ds, P1, _shape(T, D), obj, leaf_l2=0.5)
    assert r["values"].tobytes() == want.tobytes()
    # predict reads the new values: the walk over the observations, the walk over the codes and a model loaded from the file agree
    a = np.asarray(m.predict(X, None))
    b = np.asarray(m.predict_continue_prepared(ds, bias, 0, 2))
    p = tmp_path / "m.gbrl_model"
    assert m.save(str(p)) == 0
    c = np.asarray(gbrl_amd.GBRL.load(str(p)).predict(X, None))
    assert a.tobytes() == b.tobytes() == c.tobytes()


@pytest.mark.parametrize("obj,D", [("logistic", 3), ("softmax", 3)])
@pytest.mark.parametrize("generic", ["0", "1"])
def test_refusals_leave_the_model_bytes(generic, obj, D, tmp_path):
    m, ds, X, T, before = _case(16, D, "oblivious", 3, obj)
    Tn = T if obj == "softmax" else _shape(T, D)
    keep = _file(m, tmp_path)
    bad = []
    if obj == "logistic":
        for v in (1.5, -0.25, np.nan):
            t = T.copy(); t[77, 1] = v
            bad.append((before[0], t, "target"))
    for v in (np.inf, -np.inf, np.nan):
        p = before[0].copy(); p[130, 2] = v
        bad.append((p, Tn, "prediction"))
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        for p, t, what in bad:
            with pytest.raises(RuntimeError, match=what):
                m.newton_leaves_prepared(ds, p, t, obj)
            assert _file(m, tmp_path) == keep
        for kw, what in ((dict(leaf_l2=-1.0), "leaf_l2"), (dict(leaf_l2=float("nan")), "leaf_l2"), (dict(tree=1), "tree"), (dict(tree=-2), "tree")):
            with pytest.raises(RuntimeError, match=what):
                m.newton_leaves_prepared(ds, before[0], Tn, obj, **kw)
        with pytest.raises(RuntimeError, match="rmse"):
            m.newton_leaves_prepared(ds, before[0], _shape(np.zeros((N_GROW, D), np.float32), D), "rmse")
        assert _file(m, tmp_path) == keep
        # and the same call with clean inputs goes through, twice with the same bytes
        r1 = m.newton_leaves_prepared(ds, before[0], Tn, obj)
        f1 = _file(m, tmp_path)
        r2 = m.newton_leaves_prepared(ds, before[0], Tn, obj)
        assert _file(m, tmp_path) == f1 and f1 != keep
        assert r1["sums"].tobytes() == r2["sums"].tobytes() and r1["values"].tobytes() == r2["values"].tobytes()
    _CASES.pop((16, D, "oblivious", 3, obj, 1))   # the shared model now holds newton values: the next user grows its own


@pytest.mark.parametrize("D,generic,streamed", [(3, "0", 1.0), (3, "1", 0.0), (65, "0", 0.0)])
def test_the_kernel_family_is_the_one_named(D, generic, streamed):
    """the phase list of a profiled call names the step and says which family took the sums: both families are really run above"""
    m, ds, X, T, before = _case(16, D, "oblivious", 3, "logistic")
    m.set_profiling(2)
    try:
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            m.newton_leaves_prepared(ds, before[0], _shape(T, D), "logistic")
        phases = dict(m.last_phase_times())
    finally:
        m.set_profiling(0)
    assert "newton_leaves" in phases and phases["newton_leaves"] > 0.0
    assert phases["newton_streamed"] == streamed
