"""CPU-side checks of quantile regression (include/gbrl_hip.h, "Quantile regression"; gbrl_amd/csrc/quantile_core.h): the rank a level selects, the leaf
rule and the pinball gradient on the host, and every refusal that needs no device.  The rule is one definition for host and device;
tests/test_gpu_quantile.py then holds the kernels to these bits.  Everything that can be compared as bytes is.

The mean pinball loss is computed on the device only (objective_core.h: the row losses are device functions), so its check against a float64 NumPy
expression is in tests/test_gpu_quantile.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import gbrl_amd
import quantile_cases as Q   # tests/golden (conftest.py puts it on the path)

cpp = gbrl_amd.gbrl_cpp
E_INVALID = -1
C_SYMBOLS = ("gbrl_hip_fit_prepared_quantile", "gbrl_hip_quantile_leaves_prepared", "gbrl_hip_leaf_quantile_host", "gbrl_hip_quantile_rank",
             "gbrl_hip_leaf_quantile_geometry", "gbrl_hip_objective_gradient_quantile", "gbrl_hip_objective_gradient_host_quantile")

f32 = np.float32
LEVELS = [f32(0.1), f32(1.0 / 3.0), f32(0.5), f32(0.05), f32(0.95), f32(0.9), np.nextafter(f32(0), f32(1)), np.nextafter(f32(1), f32(0)),
          f32(2.0 ** -30), f32(2.0 ** -126), f32(0.75), f32(1e-3)]


def _want_rank(m, a):
    """clamp(ceil(a * m), 1, m) over the rationals: a float32 is a fraction"""
    exact = Fraction(float(a)) * m          # float(a) is exact for a float32
    k = -((-exact.numerator) // exact.denominator)
    return min(max(k, 1), m)


def test_c_symbols_and_python_names():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for name in C_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("leaf_quantile_host", "quantile_rank", "leaf_quantile_geometry", "objective_gradient_host"):
        assert hasattr(cpp, name), name
    assert hasattr(gbrl_amd.GBRL, "quantile_leaves_prepared")
    geo = cpp.leaf_quantile_geometry()
    assert sorted(geo) == ["max_select_leaves", "rows_per_chunk"] and geo["max_select_leaves"] >= 64 and geo["rows_per_chunk"] >= 64


def test_rank_is_the_exact_ceiling():
    big = [2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 2 ** 30 + 1, 2 ** 24 + 1, 10 ** 9, 16777259, 999983]
    for a in LEVELS:
        for m in list(range(1, 301)) + big:
            assert cpp.quantile_rank(m, float(a)) == _want_rank(m, a), (m, float(a))


def test_rank_where_a_double_product_rounds_across_an_integer():
    """a = M * 2^-s and m with M * m = 2^53 + 1: the double product (double)a * m rounds to 2^(53 - s), an integer for s <= 53, and its ceiling is one
    below the exact one.  2^53 + 1 = 3 * 107 * 28059810762433 has no factor pair with M < 2^24 and m < 2^31, so the pairs are built the same way from
    M * m = 2^k + 1 just above the 53-bit window after the scaling: M = 2^23 + 1 (24 bits), m = c * 2^j + 1, whose product needs more than 53 bits."""
    found = 0
    for M in (2 ** 23 + 1, 2 ** 24 - 1, 2 ** 23 + 12345, 11184811):
        for m in (2 ** 30 + 1, 2 ** 31 - 1, 2 ** 30 + 2 ** 29 + 1, 1610612737, 2 ** 30 + 3):
            P = M * m
            if P.bit_length() <= 53:
                continue
            for s in (24, 25, 30, P.bit_length() - 53 + 1, 40, 53):
                a = np.ldexp(f32(M), -s).astype(f32)
                if not (0.0 < float(a) < 1.0) or float(a) != M * 2.0 ** -s:
                    continue
                exact = _want_rank(m, a)
                assert cpp.quantile_rank(m, float(a)) == exact, (M, m, s)
                naive = min(max(int(np.ceil(np.float64(a) * np.float64(m))), 1), m)
                found += naive != exact
    assert found > 0, "no pair of the construction separates the double product from the exact one"


def test_rank_refusals():
    for m, a in ((0, 0.5), (-3, 0.5), (2 ** 31, 0.5), (10, 0.0), (10, 1.0), (10, -0.25), (10, 1.5), (10, float("nan")), (10, float("inf"))):
        with pytest.raises(RuntimeError, match="quantile_rank"):
            cpp.quantile_rank(m, a)


def _sorted_rule(x, leaves, NL, alpha):
    """np.sort per (leaf, output) with the exposed rank function: the k-th largest of the leaf's column, -0.0 taken as +0.0"""
    m, D = x.shape
    values = np.zeros((NL, D), f32)
    counts = np.zeros(NL, np.int64)
    ranks = np.zeros((NL, D), np.int64)
    canon = np.where(x == 0, f32(0), x).astype(f32)
    for l in range(NL):
        col = canon[leaves == l]
        counts[l] = len(col)
        if len(col) == 0:
            continue
        for d in range(D):
            k = cpp.quantile_rank(len(col), float(alpha[d]))
            ranks[l, d] = k
            values[l, d] = np.sort(col[:, d])[len(col) - k]
    return values, counts, ranks


@pytest.mark.parametrize("m", [1, 2, 3, 5, 63, 64, 65, 200, 1000, 4096])
def test_leaf_rule_is_the_order_statistic(m):
    rng = np.random.default_rng(m)
    D, NL = 4, 5
    x = rng.standard_normal((m, D)).astype(f32)
    x[rng.random((m, D)) < 0.33] = f32(0.25)          # a third of the values tied
    x[::11, 1] = f32(-0.0)
    x[5::11, 1] = f32(0.0)                            # both zeros mixed into a column
    x[:, 3] = f32(-1.5)                               # a column of equal values
    leaves = rng.integers(0, NL - 1, m).astype(np.int32)   # leaf NL - 1 stays empty
    if m > 4:
        leaves[:3] = [-1, NL, 7]                      # rows outside the tree join no leaf
        leaves[leaves == 2] = 0
        leaves[4] = 2                                 # a leaf of one row
    alpha = np.array([0.05, 0.5, 0.95, 1.0 / 3.0], f32)
    r = cpp.leaf_quantile_host(x, leaves, NL, alpha)
    assert sorted(r) == ["counts", "ranks", "values"]
    assert r["values"].dtype == f32 and r["values"].shape == (NL, D) and r["counts"].dtype == np.int64 and r["ranks"].shape == (NL, D)
    values, counts, ranks = _sorted_rule(x, leaves, NL, alpha)
    assert r["counts"].tobytes() == counts.tobytes() and r["ranks"].tobytes() == ranks.tobytes()
    assert r["values"].tobytes() == values.tobytes(), (r["values"], values)
    assert counts[NL - 1] == 0 and not ranks[NL - 1].any() and not r["values"][NL - 1].any()
    if m > 4:
        assert counts[2] == 1 and r["values"][2].tobytes() == np.where(x[4] == 0, f32(0), x[4]).astype(f32).tobytes()
    # -v is NumPy's inverted_cdf quantile of the residuals y - p, taken in float64 with the level as a double
    for l in range(NL):
        u = -x[leaves == l].astype(np.float64)
        for d in range(D):
            if len(u):
                assert -np.float64(r["values"][l, d]) == np.quantile(u[:, d], float(alpha[d]), method="inverted_cdf")


@pytest.mark.parametrize("n_leaves", [1, 8])
@pytest.mark.parametrize("m", [257, 5000])
@pytest.mark.parametrize("name", Q.FAMILIES)
def test_leaf_rule_on_the_key_families(name, m, n_leaves):
    """the families tests/test_gpu_quantile.py holds the kernels to (tests/golden/quantile_cases.py): the host rule is np.sort's order statistic on
    every one of them, so it is a reference there; the residuals are finite, and the families are what their names say"""
    D = 3
    pred, targets = Q.family(name, m, D, seed=m + n_leaves)
    x = Q.residual(pred, targets)
    assert x.dtype == f32 and x.shape == (m, D) and pred.dtype == f32 and targets.dtype == f32
    bits = x.view(np.uint32)
    if name == "denormal_by_subtraction":
        assert (np.abs(pred) >= Q.SMALLEST_NORMAL).all() and (np.abs(targets) >= Q.SMALLEST_NORMAL).all() and (np.abs(x) < Q.SMALLEST_NORMAL).all()
        assert (x > 0).any() and (x < 0).any() and all(len(np.unique(x[:, d])) > 100 for d in range(D))
    else:
        assert not pred.any() and x.tobytes() == (Q.values(name, m, D, seed=m + n_leaves) + f32(0)).tobytes()   # (+ 0: the zeros are +0)
    if name == "distinct":
        assert all(len(np.unique(x[:, d])) == m for d in range(D)) and (x > 0).any() and (x < 0).any()
    if name in ("last_byte", "third_byte", "second_byte"):
        shift = {"last_byte": 0, "third_byte": 8, "second_byte": 16}[name]
        r = ((bits & np.uint32(0x7fffffff)) - np.uint32(0x3f800000)) >> np.uint32(shift)
        assert (r < 256).all() and ((r << np.uint32(shift)) + np.uint32(0x3f800000) == (bits & np.uint32(0x7fffffff))).all()
        assert all(len(np.unique(bits[:, d])) == min(m, 512) for d in range(D))
    if name == "shared_prefix_ties":
        assert ((bits >> np.uint32(16)) == 0x3f80).all() and all(len(np.unique(bits[:, d])) == Q.TIE_KEYS for d in range(D))
    if name == "zeros_and_denormals":
        assert (np.abs(x) <= Q.SMALLEST_NORMAL).all() and all(len(np.unique(bits[:, d])) == 7 for d in range(D))   # (-0 has become +0)
    if name == "huge":
        assert np.abs(x).max() == np.finfo(f32).max and (np.abs(x) >= f32(2.0 ** 127)).all() and (x > 0).any() and (x < 0).any()
    if name == "negative_only":
        assert (x < 0).all()
    if name == "all_equal":
        assert len(np.unique(bits)) == 1
    rng = np.random.default_rng(m)
    leaves = np.zeros(m, np.int32) if n_leaves == 1 else rng.integers(0, n_leaves, m).astype(np.int32)
    alpha = np.array([0.05, 0.5, 0.95], f32)
    r = cpp.leaf_quantile_host(x, leaves, n_leaves, alpha)
    values, counts, ranks = _sorted_rule(x, leaves, n_leaves, alpha)
    assert (counts > 0).all()
    assert r["counts"].tobytes() == counts.tobytes() and r["ranks"].tobytes() == ranks.tobytes()
    assert r["values"].tobytes() == values.tobytes(), (r["values"], values)


def test_leaf_rule_extreme_ranks_and_scalar_level():
    x = np.arange(10, dtype=f32).reshape(10, 1) - f32(4.5)
    leaves = np.zeros(10, np.int32)
    lo, hi = float(np.nextafter(f32(0), f32(1))), float(np.nextafter(f32(1), f32(0)))
    r = cpp.leaf_quantile_host(x, leaves, 1, lo)
    assert r["ranks"][0, 0] == 1 and r["values"][0, 0] == x.max()      # k = 1: the largest x, the smallest residual
    r = cpp.leaf_quantile_host(x, leaves, 1, hi)
    assert r["ranks"][0, 0] == 10 and r["values"][0, 0] == x.min()     # k = m
    r1 = cpp.leaf_quantile_host(x[:, 0], leaves, 1, 0.5)                # [m] is [m, 1]
    assert r1["ranks"][0, 0] == 5 and r1["values"][0, 0] == f32(0.5)
    x3 = np.tile(x, (1, 3))
    assert cpp.leaf_quantile_host(x3, leaves, 1, 0.5)["values"].tobytes() == cpp.leaf_quantile_host(x3, leaves, 1, [0.5, 0.5, 0.5])["values"].tobytes()


def test_leaf_rule_refusals():
    x = np.zeros((4, 2), f32)
    leaves = np.zeros(4, np.int32)
    for alpha in ([0.5], [0.5, 0.5, 0.5]):
        with pytest.raises(RuntimeError, match="one level per output"):
            cpp.leaf_quantile_host(x, leaves, 1, alpha)
    for alpha, name in (([0.5, 0.0], r"alpha\[1\]"), ([1.0, 0.5], r"alpha\[0\]"), ([0.5, float("nan")], r"alpha\[1\]"), (-0.5, r"alpha\[0\]"), (float("inf"), r"alpha\[0\]")):
        with pytest.raises(RuntimeError, match=name):
            cpp.leaf_quantile_host(x, leaves, 1, alpha)
    for v in (np.nan, np.inf, -np.inf):
        bad = x.copy(); bad[2, 1] = v
        with pytest.raises(RuntimeError, match="not finite"):
            cpp.leaf_quantile_host(bad, leaves, 1, 0.5)
    with pytest.raises(RuntimeError):
        cpp.leaf_quantile_host(x, leaves, 0, 0.5)
    with pytest.raises(RuntimeError):
        cpp.leaf_quantile_host(x, leaves[:3], 1, 0.5)


def test_gradient_is_the_pinball_step():
    a = np.array([0.1, 0.5, 0.9], f32)
    p = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [2.5, -0.0, 1e-30], [3.0, 3.0, 3.0]], f32)
    y = np.array([[0.5, 0.5, 0.5], [2.0, 2.0, 2.0], [2.5, 0.0, 1e-30], [np.nextafter(f32(3), f32(4)), 3.0, np.nextafter(f32(3), f32(0))]], f32)
    g = cpp.objective_gradient_host(p, y, "quantile", alpha=a)
    up, down = (f32(1) - a).astype(f32), (-a).astype(f32)
    want = np.stack([up, down, np.zeros(3, f32), np.array([down[0], 0.0, up[2]], f32)])
    assert g.dtype == f32 and g.tobytes() == want.tobytes(), (g, want)
    # a scalar level is broadcast; one output
    g1 = cpp.objective_gradient_host(p[:, 0].copy(), y[:, 0].copy(), "quantile", alpha=0.25)
    assert g1.tobytes() == np.array([0.75, -0.25, 0.0, -0.25], f32).tobytes()
    # the step is that of x = fl32(p - y): where the float32 difference is 0 the step is 0
    rng = np.random.default_rng(0)
    P = rng.standard_normal((257, 3)).astype(f32)
    Y = np.where(rng.random((257, 3)) < 0.3, P, rng.standard_normal((257, 3))).astype(f32)
    x = (P - Y).astype(f32)
    want = np.where(x > 0, up, np.where(x < 0, down, f32(0))).astype(f32)
    assert cpp.objective_gradient_host(P, Y, "quantile", alpha=a).tobytes() == want.tobytes()


def test_gradient_refusals():
    p = np.zeros((4, 2), f32)
    with pytest.raises(RuntimeError, match="needs alpha"):
        cpp.objective_gradient_host(p, p, "quantile")
    for obj in ("rmse", "logistic"):
        with pytest.raises(RuntimeError, match="alpha"):
            cpp.objective_gradient_host(p, p, obj, alpha=0.5)
    with pytest.raises(RuntimeError, match=r"alpha\[1\]"):
        cpp.objective_gradient_host(p, p, "quantile", alpha=[0.5, 1.0])
    with pytest.raises(RuntimeError, match="one level per output"):
        cpp.objective_gradient_host(p, p, "quantile", alpha=[0.5, 0.5, 0.5])
    with pytest.raises(RuntimeError, match="weights"):
        cpp.objective_gradient_host(p, p, "quantile", weights=np.ones(4, f32), alpha=0.5)
    with pytest.raises(RuntimeError, match="Invalid objective"):
        cpp.objective_gradient_host(p, p, "hinge", alpha=0.5)


def test_the_hessian_rule_refuses_the_quantile_objective():
    """the pinball hessian is zero: objective_hessian_host has nothing to return for it, and never another objective's hessian"""
    p = np.zeros((4, 2), f32)
    with pytest.raises(RuntimeError, match="quantile"):
        cpp.objective_hessian_host(p, None, "quantile")
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_objective_hessian_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = np.full((4, 2), 7.0, f32)
    assert lib.gbrl_hip_objective_hessian_host(p.ctypes.data, 4, 2, 3, out.ctypes.data) == E_INVALID and (out == 7.0).all()
    assert cpp.objective_hessian_host(p, None, "logistic").tobytes() == np.full((4, 2), 0.25, f32).tobytes()   # the others are as they were


def _model(D=2):
    m = gbrl_amd.GBRL(input_dim=3, output_dim=D, policy_dim=D, max_depth=3, n_bins=16, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious",
                      device="cpu", batch_size=64)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    return m


def test_fit_refusals_that_need_no_device(tmp_path):
    """fit_prepared checks its options before it looks at the data set: a null data set is never reached"""
    m = _model()
    y = np.zeros((8, 2), f32)
    w = np.ones(8, f32)
    cases = [
        (dict(objective="quantile"), "needs alpha"),
        (dict(objective="rmse", alpha=0.5), "alpha"),
        (dict(objective="logistic", alpha=[0.5, 0.5]), "alpha"),
        (dict(objective="quantile", alpha=[0.5, 1.0]), r"alpha\[1\]"),
        (dict(objective="quantile", alpha=[0.5, float("nan")]), r"alpha\[1\]"),
        (dict(objective="quantile", alpha=0.0), r"alpha\[0\]"),
        (dict(objective="quantile", alpha=[0.5]), "one level per output"),
        (dict(objective="quantile", alpha=[0.5, 0.5, 0.5]), "one level per output"),
        (dict(objective="rmse", leaf_update="quantile"), "quantile leaf values"),
        (dict(objective="logistic", leaf_update="quantile"), "quantile leaf values"),
        (dict(objective="quantile", alpha=0.5, leaf_update="newton"), "hessian is zero"),
        (dict(objective="quantile", alpha=0.5, weights=w), "weights"),
        (dict(objective="quantile", alpha=0.5, leaf_update="quantile", goss=(0.2, 0.2)), "goss"),
        (dict(objective="quantile", alpha=0.5, leaf_update="hessian"), "Invalid leaf_update"),
        (dict(objective="hinge", alpha=0.5), "Invalid objective"),
    ]
    for kw, what in cases:
        with pytest.raises(RuntimeError, match=what):
            m.fit_prepared(None, y, 2, **kw)
    assert m.get_num_trees() == 0


def test_keywords_are_documented():
    doc = gbrl_amd.GBRL.fit_prepared.__doc__
    for word in ("alpha=None", "objective='quantile'", "leaf_update='quantile'", "quantile_leaves_prepared", "inverted_cdf"):
        assert word in doc, word
    assert "alpha=None" in gbrl_amd.GBRL.objective_gradient.__doc__ and "alpha=None" in cpp.objective_gradient_host.__doc__
    for fn, words in ((gbrl_amd.GBRL.quantile_leaves_prepared, ("alpha", "rows=None", "tree=-1", "'values'", "'counts'", "'ranks'")),
                      (cpp.leaf_quantile_host, ("n_leaves", "alpha", "quantile_rank")), (cpp.quantile_rank, ("ceil", "exactly"))):
        for word in words:
            assert word in fn.__doc__, (fn, word)
