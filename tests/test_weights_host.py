"""CPU-side checks of row weights (include/gbrl_hip.h, "Row weights"; gbrl_amd/csrc/objective_core.h and newton_core.h): the weighted gradient and
hessian are one float32 multiply behind the unweighted rules, all-ones weights change no byte, the Newton quantum makes room for the largest weight,
and the host entries refuse what the rule refuses.  tests/test_gpu_fit_weights.py holds the device to these bits."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
E_INVALID = -1
C_SYMBOLS = ("gbrl_hip_fit_prepared_weighted", "gbrl_hip_objective_gradient_weighted", "gbrl_hip_newton_leaves_prepared_weighted",
             "gbrl_hip_objective_gradient_host_weighted", "gbrl_hip_objective_hessian_host_weighted", "gbrl_hip_newton_sum_bits_weighted")
WEIGHT_MAX = 65536.0


def _inputs(n, D, seed):
    rng = np.random.default_rng(seed)
    p = (3.0 * rng.standard_normal((n, D))).astype(np.float32)
    y = rng.uniform(0.0, 1.0, (n, D)).astype(np.float32)
    labels = rng.integers(0, max(D, 1), n).astype(np.int32)
    w = rng.uniform(0.0, 8.0, n).astype(np.float32)
    w[::7] = 0.0
    w[3] = np.float32(WEIGHT_MAX)
    w[5] = np.float32(1.0)
    return p, y, labels, w


def _targets(obj, y, labels):
    return labels if obj == "softmax" else y


def test_c_symbols_and_python_names():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for name in C_SYMBOLS:
        assert hasattr(lib, name), name
    for fn in (cpp.GBRL.fit_prepared, cpp.GBRL.objective_gradient, cpp.GBRL.newton_leaves_prepared, cpp.objective_gradient_host, cpp.objective_hessian_host):
        assert "weights" in fn.__doc__
    assert "valid_weights" in cpp.GBRL.fit_prepared.__doc__ and "weight_max" in cpp.GBRL.newton_leaves_prepared.__doc__
    assert "weight_max" in cpp.newton_sum_bits.__doc__


@pytest.mark.parametrize("obj,D", [("rmse", 1), ("rmse", 5), ("logistic", 1), ("logistic", 8), ("softmax", 5), ("softmax", 68)])
def test_weighted_gradient_and_hessian_are_one_multiply_behind_the_rule(obj, D):
    n = 777
    p, y, labels, w = _inputs(n, D, seed=n + D)
    t = _targets(obj, y, labels)
    g = cpp.objective_gradient_host(p, t, obj)
    gw = cpp.objective_gradient_host(p, t, obj, weights=w)
    assert gw.dtype == np.float32 and gw.shape == g.shape
    assert gw.tobytes() == (w[:, None] * g).astype(np.float32).tobytes()
    h = cpp.objective_hessian_host(p, None, obj)
    hw = cpp.objective_hessian_host(p, None, obj, weights=w)
    assert hw.dtype == np.float32 and hw.tobytes() == (w[:, None] * h).astype(np.float32).tobytes()
    # all-ones weights: the unweighted bytes
    ones = np.ones(n, np.float32)
    assert cpp.objective_gradient_host(p, t, obj, weights=ones).tobytes() == g.tobytes()
    assert cpp.objective_hessian_host(p, None, obj, weights=ones).tobytes() == h.tobytes()
    # None is the call without the keyword
    assert cpp.objective_gradient_host(p, t, obj, weights=None).tobytes() == g.tobytes()
    if D == 1:   # the one-dimensional form
        assert cpp.objective_gradient_host(p[:, 0].copy(), t[:, 0].copy(), obj, weights=w).tobytes() == gw.tobytes()


def _bits(m, weight_max):
    e = 0
    while 2.0 ** e < weight_max:
        e += 1
    return min(40, 62 - int(m).bit_length() - e)


def test_newton_sum_bits_with_a_weight_max():
    above_one = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    above_two = float(np.nextafter(np.float32(2.0), np.float32(3.0)))
    cases = ((0.0, 0), (0.5, 0), (1.0, 0), (above_one, 1), (2.0, 1), (above_two, 2), (3.0, 2), (4.0, 2), (8.0, 3), (32768.0, 15),
             (float(np.nextafter(np.float32(32768.0), np.float32(65536.0))), 16), (WEIGHT_MAX, 16))
    for m in (1, 2, 3, 2**5, 2**20, 2**21 - 1, 2**21, 2**22 - 1, 2**22, 2**22 + 1, 2**30, 2**31 - 1):
        assert cpp.newton_sum_bits(m, None) == cpp.newton_sum_bits(m) == cpp.newton_sum_bits(m, 1.0)
        for wmax, e in cases:
            got = cpp.newton_sum_bits(m, wmax)
            assert got == min(40, 62 - int(m).bit_length() - e) == _bits(m, wmax), (m, wmax, got)
            assert got >= 0 and m * 2 ** e * 2 ** got < 2 ** 62   # |sum| <= m * weight_max * 2^bits stays below 2^62
    for bad in (float("nan"), -1.0, float("inf"), 65537.0, -0.5):
        with pytest.raises(RuntimeError, match="weight_max"):
            cpp.newton_sum_bits(100, bad)


def test_host_entries_refuse_bad_weights():
    n, D = 40, 3
    p, y, labels, w = _inputs(n, D, seed=9)
    for bad, row in ((np.nan, 17), (-1.0, 0), (np.inf, 39), (65537.0, 5), (-np.inf, 2)):
        wb = w.copy()
        wb[row] = bad
        for call in (lambda: cpp.objective_gradient_host(p, y, "logistic", weights=wb), lambda: cpp.objective_gradient_host(p, labels, "softmax", weights=wb),
                     lambda: cpp.objective_hessian_host(p, None, "logistic", weights=wb), lambda: cpp.objective_gradient_host(p, y, "rmse", weights=wb)):
            with pytest.raises(RuntimeError, match=r"row %d\)" % row):
                call()
    # the first refused row is the one named
    wb = w.copy(); wb[11] = -2.0; wb[30] = np.nan
    with pytest.raises(RuntimeError, match=r"row 11\)"):
        cpp.objective_gradient_host(p, y, "rmse", weights=wb)
    # length and dtype
    with pytest.raises(RuntimeError, match="weights"):
        cpp.objective_gradient_host(p, y, "rmse", weights=w[:-1].copy())
    with pytest.raises(RuntimeError, match="weights"):
        cpp.objective_hessian_host(p, None, "logistic", weights=np.ones((n, 1), np.float32))
    with pytest.raises(RuntimeError, match="format"):
        cpp.objective_gradient_host(p, y, "rmse", weights=w.astype(np.float64))
    # the edges of the range are weights like any other
    edge = w.copy(); edge[0] = 0.0; edge[1] = WEIGHT_MAX; edge[2] = np.float32(-0.0)
    cpp.objective_gradient_host(p, y, "rmse", weights=edge)


def test_c_abi_host_entries():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_objective_gradient_host_weighted.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    lib.gbrl_hip_objective_hessian_host_weighted.argtypes = [vp, vp, ci, ci, ci, vp]
    lib.gbrl_hip_objective_gradient_host.argtypes = [vp, vp, ci, ci, ci, vp]
    lib.gbrl_hip_newton_sum_bits_weighted.argtypes = [C.c_int64, C.c_float]
    n, D = 33, 4
    p, y, labels, w = _inputs(n, D, seed=4)
    out = np.zeros((n, D), np.float32)
    assert lib.gbrl_hip_objective_gradient_host_weighted(p.ctypes.data, y.ctypes.data, w.ctypes.data, n, D, 1, out.ctypes.data) == 0
    assert out.tobytes() == cpp.objective_gradient_host(p, y, "logistic", weights=w).tobytes()
    # a NULL weight vector is the older spelling, which keeps its bytes
    old = np.zeros((n, D), np.float32)
    assert lib.gbrl_hip_objective_gradient_host_weighted(p.ctypes.data, y.ctypes.data, None, n, D, 1, out.ctypes.data) == 0
    assert lib.gbrl_hip_objective_gradient_host(p.ctypes.data, y.ctypes.data, n, D, 1, old.ctypes.data) == 0
    assert out.tobytes() == old.tobytes() == cpp.objective_gradient_host(p, y, "logistic").tobytes()
    assert lib.gbrl_hip_objective_hessian_host_weighted(p.ctypes.data, w.ctypes.data, n, D, 2, out.ctypes.data) == 0
    assert out.tobytes() == cpp.objective_hessian_host(p, None, "softmax", weights=w).tobytes()
    wb = w.copy(); wb[8] = np.nan
    assert lib.gbrl_hip_objective_gradient_host_weighted(p.ctypes.data, y.ctypes.data, wb.ctypes.data, n, D, 1, out.ctypes.data) == E_INVALID
    assert b"row 8)" in lib.gbrl_hip_last_error()
    assert lib.gbrl_hip_objective_hessian_host_weighted(p.ctypes.data, wb.ctypes.data, n, D, 1, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_newton_sum_bits_weighted(2**22, 1.0) == 39 and lib.gbrl_hip_newton_sum_bits_weighted(2**22, 65536.0) == 23
    assert lib.gbrl_hip_newton_sum_bits_weighted(100, float("nan")) == E_INVALID and lib.gbrl_hip_newton_sum_bits_weighted(100, 65537.0) == E_INVALID


def _model(D=2):
    m = gbrl_amd.GBRL(input_dim=4, output_dim=D, policy_dim=D, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    return m


def test_binding_refusals_need_no_device():
    """every refusal here comes before a data set handle is resolved, so no GPU is touched"""
    m = _model()
    y = np.zeros((8, 2), np.float32)
    w = np.ones(8, np.float32)
    with pytest.raises(RuntimeError, match="valid_weights need a validation set"):
        m.fit_prepared(None, y, 2, valid_weights=w)
    with pytest.raises(RuntimeError, match="format"):
        m.fit_prepared(None, y, 2, weights=w.astype(np.float64))
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, y, 2, weights=w)   # past the new checks
    with pytest.raises(RuntimeError, match="weight_max needs weights"):
        m.newton_leaves_prepared(None, y, y, "logistic", weight_max=2.0)
    with pytest.raises(RuntimeError, match="weight_max"):
        m.newton_leaves_prepared(None, y, y, "logistic", weights=w, weight_max=float("nan"))
    with pytest.raises(RuntimeError, match="weights"):
        m.newton_leaves_prepared(None, y, y, "logistic", weights=np.ones(7, np.float32))
    with pytest.raises(RuntimeError, match="weights"):
        m.objective_gradient(y, y, "logistic", weights=np.ones(9, np.float32))
