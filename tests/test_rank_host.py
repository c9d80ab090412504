"""CPU-side checks of the ranking objectives (include/gbrl_hip.h, "Ranking objectives"; gbrl_amd/csrc/rank_core.h): the rule on the host against an
independent NumPy walk (tests/golden/rank_cases.py), the constructed cases, the discount table and every refusal that needs no device.  The rule is
one definition for host and device; tests/test_gpu_rank.py then holds the kernels to these bytes.

The pairwise loss is computed on the device only (a float64 libm expression, as the logistic loss is), so its check is in tests/test_gpu_rank.py."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd
import rank_cases as R   # tests/golden (conftest.py puts it on the path)

cpp = gbrl_amd.gbrl_cpp
f32 = np.float32
E_INVALID = -1
C_SYMBOLS = ("gbrl_hip_rank_gradient", "gbrl_hip_rank_gradient_host", "gbrl_hip_rank_discounts", "gbrl_hip_rank_geometry", "gbrl_hip_fit_prepared_rank",
             "gbrl_hip_newton_leaves_prepared_rank")


def _same(r, want, what):
    g, h, ndcg, pos, pairs = want
    assert r["grad"].dtype == f32 and r["hess"].dtype == f32 and r["ndcg"].dtype == np.float64 and r["positions"].dtype == np.int32
    assert r["positions"].tobytes() == pos.tobytes(), what
    assert r["ndcg"].tobytes() == ndcg.tobytes(), (what, r["ndcg"], ndcg)
    assert r["grad"].tobytes() == g.tobytes(), (what, np.nonzero(r["grad"] != g)[0][:5])
    assert r["hess"].tobytes() == h.tobytes(), (what, np.nonzero(r["hess"] != h)[0][:5])
    assert r["pairs"] == pairs, what


def test_c_symbols_and_python_names():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for name in C_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("rank_gradient_host", "rank_discounts", "rank_geometry"):
        assert hasattr(cpp, name), name
    assert hasattr(gbrl_amd.GBRL, "rank_gradient")
    assert cpp.rank_geometry() == {"max_query": 1024, "max_label": 30}


def test_discounts_are_the_table():
    """two libm calls (the library's log2 and NumPy's) may differ by one unit in the last place; every other test uses the table itself"""
    d = cpp.rank_discounts()
    assert d.dtype == np.float64 and d.shape == (1024,)
    want = 1.0 / np.log2(np.arange(1024, dtype=np.float64) + 2.0)
    assert (np.abs(d - want) <= np.spacing(want)).all()
    assert d[0] == 1.0 and d[2] == 0.5 and (np.diff(d) < 0).all()
    assert cpp.rank_discounts().tobytes() == d.tobytes()


@pytest.mark.parametrize("objective,ndcg_at", [("pairwise", None), ("lambdarank", None), ("lambdarank", 10)])
def test_rule_against_the_numpy_walk(objective, ndcg_at):
    s, y = R.scores_and_labels(R.LAYOUT, seed=7)
    assert len(s) == 1672
    r = cpp.rank_gradient_host(s, y, R.LAYOUT, objective, ndcg_at)
    assert sorted(r) == (["grad", "hess", "loss", "ndcg", "pairs", "positions"] if objective == "lambdarank" else ["grad", "hess", "ndcg", "pairs", "positions"])
    _same(r, R.walk(cpp, s, y, R.LAYOUT, objective, ndcg_at), (objective, ndcg_at))
    if objective == "lambdarank":
        assert abs(r["loss"] - (1.0 - np.mean(r["ndcg"]))) <= 1e-14
        assert (np.abs(r["grad"]) < 1024).all() and (r["hess"] >= 0).all()
    assert r["pairs"] > 0 and r["grad"].any()


@pytest.mark.parametrize("case", R.constructed(), ids=lambda c: c[0])
def test_constructed_cases(case):
    name, s, y, group = case
    for objective, ks in (("pairwise", [None]), ("lambdarank", [None, 1, 3, 2000])):
        for k in ks:
            r = cpp.rank_gradient_host(s, y, group, objective, k)
            _same(r, R.walk(cpp, s, y, group, objective, k), (name, objective, k))
    r = cpp.rank_gradient_host(s, y, group, "pairwise")
    lam = cpp.rank_gradient_host(s, y, group, "lambdarank")
    if name == "bradley_terry":       # -log sigmoid(s_0 - s_1): g = (-r, +r), h = (e, e), the existing logistic bits
        d = np.array([s[0] - s[1]], f32)
        rho = cpp.objective_gradient_host(-d, np.zeros(1, f32), "logistic")[0]
        eta = cpp.objective_hessian_host(d, None, "logistic")[0]
        assert r["grad"].tobytes() == np.array([-rho, rho], f32).tobytes() and r["hess"].tobytes() == np.array([eta, eta], f32).tobytes()
        assert r["pairs"] == 1 and rho > 0
    if name == "all_scores_equal":    # positions are the row order inside each query
        assert r["positions"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4]
    if name == "zeros_tie":           # +0.0 and -0.0 tie: row order; 1.0 is first
        assert r["positions"].tolist() == [1, 2, 3, 4, 0]
    if name in ("all_labels_zero", "all_labels_equal"):
        assert not r["grad"].any() and not r["hess"].any() and not lam["grad"].any() and r["pairs"] == 0
        assert np.signbit(r["grad"]).sum() == 0
    if name == "all_labels_zero":
        assert (lam["ndcg"] == 1.0).all() and lam["loss"] == 0.0
    if name == "all_labels_equal":    # any order of equal labels is ideal
        assert (lam["ndcg"] == 1.0).all()
    if name == "labels_30_and_0":
        assert r["pairs"] == 9 and lam["grad"].any() and np.isfinite(lam["grad"]).all() and (lam["ndcg"] > 0).all() and (lam["ndcg"] < 1).all()
    if name == "one_row":
        assert r["positions"].tolist() == [0] and not r["grad"].any() and lam["ndcg"][0] == 1.0
    if name.startswith("exp_branches"):
        assert np.isfinite(r["grad"]).all() and np.isfinite(r["hess"]).all() and r["grad"].any()
    # ndcg_at above the query size is no truncation; ndcg_at = 1 leaves only pairs that involve the first position
    assert cpp.rank_gradient_host(s, y, group, "lambdarank", 2000)["grad"].tobytes() == lam["grad"].tobytes()
    assert cpp.rank_gradient_host(s, y, group, "lambdarank", 0)["grad"].tobytes() == lam["grad"].tobytes()


def test_refusals_of_the_host_rule():
    s, y = np.zeros(6, f32), np.array([0, 1, 2, 0, 1, 2], np.int32)
    cases = [
        (dict(group=[3, 2]), "sum to 5"),
        (dict(group=[3, 4]), "sum to 7"),
        (dict(group=[3, 0, 3]), r"group\[1\] = 0 \(query 1\)"),
        (dict(group=[-1, 7]), r"group\[0\] = -1 \(query 0\)"),
        (dict(group=[3, 3], ndcg_at=-1), "ndcg_at"),
        (dict(group=[3, 3], objective="pairwise", ndcg_at=3), "ndcg_at"),
        (dict(group=[3, 3], objective="rmse"), "Invalid objective"),
        (dict(group=[3, 3], objective="hinge"), "Invalid objective"),
        (dict(group=None), "needs group"),
        (dict(group=[]), "needs group"),
    ]
    for kw, what in cases:
        kw = dict(dict(objective="lambdarank"), **kw)
        with pytest.raises(RuntimeError, match=what):
            cpp.rank_gradient_host(s, y, kw["group"], kw["objective"], kw.get("ndcg_at"))
    big = np.zeros(1030, f32)
    with pytest.raises(RuntimeError, match=r"group\[1\] = 1025 \(query 1\)"):
        cpp.rank_gradient_host(big, np.zeros(1030, np.int32), [5, 1025], "lambdarank")
    for bad in (31, -1):
        yb = y.copy(); yb[4] = bad
        with pytest.raises(RuntimeError, match=r"label %d \(row 4\)" % bad):
            cpp.rank_gradient_host(s, yb, [3, 3], "pairwise")
    for v in (np.nan, np.inf, -np.inf):
        sb = s.copy(); sb[2] = v
        with pytest.raises(RuntimeError, match="not finite"):
            cpp.rank_gradient_host(sb, y, [3, 3], "lambdarank")
    with pytest.raises(RuntimeError, match="int32"):
        cpp.rank_gradient_host(s, y.astype(np.int64), [3, 3], "lambdarank")
    with pytest.raises(RuntimeError, match="labels"):
        cpp.rank_gradient_host(s, y[:5], [3, 3], "lambdarank")
    with pytest.raises(RuntimeError, match="one number"):
        cpp.rank_gradient_host(np.zeros((6, 2), f32), y, [3, 3], "lambdarank")


def _model(D=1):
    m = gbrl_amd.GBRL(input_dim=3, output_dim=D, policy_dim=D, max_depth=3, n_bins=16, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious",
                      device="cpu", batch_size=64)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    return m


def test_model_refusals_that_need_no_device():
    """rank_gradient checks the objective, the model's width, the group and ndcg_at before it looks for a device"""
    s, y = np.zeros(6, f32), np.array([0, 1, 2, 0, 1, 2], np.int32)
    m = _model()
    for kw, what in ((dict(group=[3, 2]), "sum to 5"), (dict(group=[3, 0, 3]), r"\(query 1\)"), (dict(group=[3, 3], ndcg_at=-2), "ndcg_at"),
                     (dict(group=[3, 3], objective="pairwise", ndcg_at=2), "ndcg_at"), (dict(group=[3, 3], objective="logistic"), "Invalid objective"),
                     (dict(group=None), "needs group")):
        with pytest.raises(RuntimeError, match=what):
            m.rank_gradient(s, y, **kw)
    with pytest.raises(RuntimeError, match="output_dim == 1"):
        _model(2).rank_gradient(s, y, [3, 3])
    # objective_gradient forwards the ranking names and keeps group away from the others
    with pytest.raises(RuntimeError, match="sum to 5"):
        m.objective_gradient(s, y, "lambdarank", group=[3, 2])
    with pytest.raises(RuntimeError, match="needs group"):
        m.objective_gradient(s, y, "pairwise")
    with pytest.raises(RuntimeError, match="group"):
        m.objective_gradient(s, s, "logistic", group=[3, 3])
    with pytest.raises(RuntimeError, match="ndcg_at"):
        m.objective_gradient(s, s, "rmse", ndcg_at=3)
    with pytest.raises(RuntimeError, match="weights"):
        m.objective_gradient(s, y, "pairwise", weights=np.ones(6, f32), group=[3, 3])
    # the calls that know no query structure refuse the ranking names, and say why
    for name in ("pairwise", "lambdarank"):
        with pytest.raises(RuntimeError, match="ranking"):
            cpp.objective_gradient_host(s, y, name)
        with pytest.raises(RuntimeError, match="ranking"):
            cpp.objective_hessian_host(s, None, name)
    assert m.get_num_trees() == 0


def test_fit_refusals_that_need_no_device():
    """fit_prepared checks its options before it looks at the data set: a null data set is never reached"""
    m = _model()
    y = np.array([0, 1, 2, 0, 1, 2, 1, 0], np.int32)
    w = np.ones(8, f32)
    rank = dict(objective="lambdarank", group=[4, 4])
    cases = [
        (dict(objective="lambdarank"), "needs group"),
        (dict(objective="pairwise"), "needs group"),
        (dict(objective="rmse", group=[4, 4]), "belong to the ranking objectives"),
        (dict(objective="logistic", ndcg_at=3), "belong to the ranking objectives"),
        (dict(objective="rmse", valid_group=[4, 4]), "valid_group"),
        (dict(rank, group=[4, 0, 4]), r"group\[1\] = 0 \(query 1\)"),
        (dict(rank, group=[4, 1025]), r"group\[1\] = 1025 \(query 1\)"),
        (dict(rank, subsample=0.5), "subsample"),
        (dict(rank, goss=(0.2, 0.2)), "goss"),
        (dict(rank, weights=w), "weights"),
        (dict(rank, alpha=0.5), "alpha"),
        (dict(rank, eval_metric="error"), "eval_metric"),
        (dict(rank, leaf_update="quantile"), "quantile leaf values"),
        (dict(rank, leaf_update="hessian"), "Invalid leaf_update"),
        (dict(rank, leaf_update="newton", leaf_l2=-1.0), "leaf_l2"),
        (dict(rank, ndcg_at=-1), "ndcg_at"),
        (dict(objective="pairwise", group=[4, 4], ndcg_at=3), "ndcg_at"),
        (dict(objective="hinge", group=[4, 4]), "Invalid objective"),
    ]
    for kw, what in cases:
        t = y if kw["objective"] in ("pairwise", "lambdarank") else y.astype(f32)     # relevance labels, or float targets
        with pytest.raises(RuntimeError, match=what):
            m.fit_prepared(None, t, 2, **kw)
    with pytest.raises(RuntimeError, match="output_dim == 1"):
        _model(2).fit_prepared(None, y, 2, **rank)
    with pytest.raises(RuntimeError, match="group"):
        m.newton_leaves_prepared(None, np.zeros(8, f32), np.zeros(8, f32), "logistic", group=[4, 4])
    with pytest.raises(RuntimeError, match="rows"):
        m.newton_leaves_prepared(None, np.zeros(8, f32), y, "lambdarank", group=[4, 4], rows=np.arange(4, dtype=np.int32))
    assert m.get_num_trees() == 0


def test_the_c_abi_codes():
    """codes 4 and 5 belong to the ranking calls; every other entry refuses them, and an unknown code keeps its message"""
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    s, y = np.array([0.5, -0.5, 0.0], f32), np.array([1, 0, 2], np.int32)
    group = np.array([3], np.int32)
    g, h, pos = np.full(3, 7.0, f32), np.full(3, 7.0, f32), np.zeros(3, np.int32)
    ndcg, pairs = np.zeros(1), C.c_int64(0)
    lib.gbrl_hip_rank_gradient_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
    args = (s.ctypes.data, y.ctypes.data, group.ctypes.data, 1, 3)
    outs = (g.ctypes.data, h.ctypes.data, None, ndcg.ctypes.data, pos.ctypes.data, C.addressof(pairs))
    for code in (7, 0, 3, -1):
        assert lib.gbrl_hip_rank_gradient_host(*args, code, 0, *outs) == E_INVALID and b"unknown objective" in lib.gbrl_hip_last_error()
        assert (g == 7.0).all()
    assert lib.gbrl_hip_rank_gradient_host(*args, 4, 0, *outs) == 0 and pairs.value == 3
    assert g.tobytes() == cpp.rank_gradient_host(s, y, [3], "pairwise")["grad"].tobytes()
    assert lib.gbrl_hip_rank_gradient_host(*args, 5, 0, *outs) == 0
    assert g.tobytes() == cpp.rank_gradient_host(s, y, [3], "lambdarank")["grad"].tobytes()
    loss = C.c_double(0)
    assert lib.gbrl_hip_rank_gradient_host(*args, 4, 0, g.ctypes.data, h.ctypes.data, C.addressof(loss), None, None, None) == E_INVALID   # the pairwise loss is device-only
    lib.gbrl_hip_objective_gradient_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = np.full(3, 7.0, f32)
    for code in (4, 5):
        assert lib.gbrl_hip_objective_gradient_host(s.ctypes.data, s.ctypes.data, 3, 1, code, out.ctypes.data) == E_INVALID and (out == 7.0).all()
        assert b"ranking" in lib.gbrl_hip_last_error()
    assert lib.gbrl_hip_objective_gradient_host(s.ctypes.data, s.ctypes.data, 3, 1, 7, out.ctypes.data) == E_INVALID and b"unknown objective" in lib.gbrl_hip_last_error()


def test_keywords_are_documented():
    for fn, words in ((gbrl_amd.GBRL.rank_gradient, ("objective='lambdarank'", "ndcg_at=None", "'grad'", "'hess'", "'loss'", "'ndcg'", "'positions'", "'pairs'",
                                                     "Bradley-Terry", "lambdarank_norm", "label_gain")),
                      (cpp.rank_gradient_host, ("ndcg_at=None", "rank_discounts", "objective_hessian_host")),
                      (gbrl_amd.GBRL.objective_gradient, ("group=None", "ndcg_at=None", "rank_gradient")), (cpp.rank_discounts, ("log2",)),
                      (gbrl_amd.GBRL.fit_prepared, ("group=None", "ndcg_at=None", "valid_group=None", "objective='pairwise' | 'lambdarank'", "Bradley-Terry",
                                                    "newton_leaves_prepared(group=)", "label_gain")),
                      (gbrl_amd.GBRL.newton_leaves_prepared, ("group=None", "ndcg_at=None")),
                      (cpp.rank_geometry, ("max_query",))):
        for word in words:
            assert word in fn.__doc__, (fn, word)
