"""CPU-side checks of the Newton leaf rule behind fit_prepared(leaf_update="newton") and GBRL.newton_leaves_prepared (include/gbrl_hip.h, "Newton
leaf values"; gbrl_amd/csrc/newton_core.h).  The hessian, the quantum of the sums and the leaf value are one definition for host and device, so
they are held here, on the host, to float64 NumPy; tests/test_gpu_newton.py then holds the device to these bits.

The error bounds below were MEASURED on the grids of this file (DESIGN.md section 5 has the figures) and carry one float32 ulp (2^-23) of margin:
  logistic, h >= 2^-126:  largest relative error 4.794 * 2^-24 against (1 / (1 + e)) * (e / (1 + e)), e = exp(-|p|), in float64
  logistic, h <  2^-126:  largest absolute error 0.75 * 2^-149 (the result is a float32 subnormal: a relative error means nothing there)
  softmax:                largest absolute error 2.308 * 2^-24 against q (1 - q); relative 16.942 * 2^-24 where q <= 0.5.  For q above 0.5 the rule's own
                          fl32(1 - q) cancels (q rounds to 1 and h to 0 for a class that has won): the definition scikit-learn, XGBoost and LightGBM
                          share, and the reason no relative bound is stated there."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
E_INVALID = -1
ULP = 2.0 ** -23
LOGISTIC_REL = 4.794 * 2.0 ** -24     # measured, h >= 2^-126
LOGISTIC_SUB_ABS = 0.75 * 2.0 ** -149  # measured, below
SOFTMAX_ABS = 2.308 * 2.0 ** -24       # measured
SOFTMAX_REL_SMALL_Q = 16.942 * 2.0 ** -24 # measured, q <= 0.5 and h >= 2^-126
C_SYMBOLS = ("gbrl_hip_newton_leaves_prepared", "gbrl_hip_objective_hessian_host", "gbrl_hip_newton_values_host", "gbrl_hip_fit_prepared_leaf",
             "gbrl_hip_newton_sum_bits", "gbrl_hip_fit_prepared_metric")


def logistic_grid():
    g = np.linspace(-100.0, 100.0, 2**20 + 1).astype(np.float32)
    return np.unique(np.concatenate([g, np.arange(-100, 101).astype(np.float32), np.float32([0.0, -0.0, 100.0, -100.0, 1e-30, -1e-30])]))


def logistic64(p):
    p = p.astype(np.float64)
    e = np.exp(-np.abs(p))
    return (1.0 / (1.0 + e)) * (e / (1.0 + e))


def softmax_rows():
    g = np.linspace(-100.0, 100.0, 2**16 + 1).astype(np.float32)
    rng = np.random.default_rng(11)
    rows = [np.stack([g, -0.5 * g, np.ones_like(g)], axis=1), np.stack([g, g + np.float32(0.5), 0.25 * g], axis=1),
            rng.normal(0.0, 3.0, (4096, 3)).astype(np.float32),
            np.float32([[0, 0, 0], [-0.0, 0.0, -0.0], [100, -100, 0], [-100, -100, -100], [-np.inf, 0, 1], [5, 5, -np.inf]])]
    return np.concatenate(rows).astype(np.float32)


def softmax64(p):
    p = p.astype(np.float64)
    e = np.exp(p - p.max(axis=1, keepdims=True))
    q = e / e.sum(axis=1, keepdims=True)
    return q, q * (1.0 - q)


def test_c_symbols_and_python_names():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for name in C_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("objective_hessian_host", "newton_values_host", "newton_sum_bits"):
        assert hasattr(cpp, name), name
    assert hasattr(cpp.GBRL, "newton_leaves_prepared")
    assert "leaf_update" in cpp.GBRL.fit_prepared.__doc__


def test_logistic_hessian_against_float64():
    p = logistic_grid()
    h = cpp.objective_hessian_host(p, None, "logistic")
    assert h.dtype == np.float32 and h.shape == p.shape
    want = logistic64(p)
    h64 = h.astype(np.float64)
    normal = want >= 2.0 ** -126
    rel = (np.abs(h64 - want)[normal] / want[normal]).max()
    sub = np.abs(h64 - want)[~normal].max()
    print(f"logistic hessian: largest relative error {rel / 2.0**-24:.3f} * 2^-24 (h >= 2^-126), largest absolute error {sub / 2.0**-149:.3f} * 2^-149 below")
    assert rel <= LOGISTIC_REL + ULP
    assert sub <= LOGISTIC_SUB_ABS + 2.0 ** -149
    assert h.min() >= 0.0 and h.max() <= 0.25


def test_logistic_hessian_exact_cases():
    h = cpp.objective_hessian_host(np.float32([0.0, -0.0, 100.0, -100.0, np.inf, -np.inf]), None, "logistic")
    assert h[0].tobytes() == np.float32(0.25).tobytes() and h[1].tobytes() == np.float32(0.25).tobytes()
    assert h[2].tobytes() == h[3].tobytes() and h[2] > 0.0            # symmetry, bit for bit
    assert h[4].tobytes() == np.float32(0.0).tobytes() and h[5].tobytes() == np.float32(0.0).tobytes()
    p = logistic_grid()
    assert cpp.objective_hessian_host(p, None, "logistic").tobytes() == cpp.objective_hessian_host(-p, None, "logistic").tobytes()
    assert np.isnan(cpp.objective_hessian_host(np.float32([np.nan]), None, "logistic")[0])
    # the 2-D form and the targets argument change nothing
    p2 = p[: 6 * 1000].reshape(1000, 6)
    assert cpp.objective_hessian_host(p2, np.zeros_like(p2), "logistic").tobytes() == cpp.objective_hessian_host(p2.ravel(), None, "logistic").tobytes()


def test_softmax_hessian_against_float64():
    p = softmax_rows()
    h = cpp.objective_hessian_host(p, None, "softmax")
    assert h.dtype == np.float32 and h.shape == p.shape
    q, want = softmax64(p)
    h64 = h.astype(np.float64)
    err = np.abs(h64 - want).max()
    small = (q <= 0.5) & (want >= 2.0 ** -126)
    rel = (np.abs(h64 - want)[small] / want[small]).max()
    print(f"softmax hessian: largest absolute error {err / 2.0**-24:.3f} * 2^-24, largest relative error {rel / 2.0**-24:.3f} * 2^-24 where q <= 0.5")
    assert err <= SOFTMAX_ABS + ULP * 0.25          # one ulp of the largest value, 0.25
    assert rel <= SOFTMAX_REL_SMALL_Q + ULP
    assert h.min() >= 0.0 and h.max() <= 0.25
    # q is the gradient's: g + onehot == q, and h == fl32(q * fl32(1 - q)) bit for bit
    labels = np.zeros(p.shape[0], np.int32)
    g = cpp.objective_gradient_host(p, labels, "softmax")
    q32 = g.copy()
    q32[:, 0] = g[:, 0] + np.float32(1.0)
    ok = g[:, 0] >= np.float32(-0.5)   # q >= 0.5: q - 1 and (q - 1) + 1 are exact there (Sterbenz); elsewhere column 0 is skipped
    want32 = (q32 * (np.float32(1.0) - q32)).astype(np.float32)
    assert h[:, 1:].tobytes() == want32[:, 1:].tobytes()
    assert h[ok, 0].tobytes() == want32[ok, 0].tobytes()


def test_softmax_hessian_row_with_inf():
    h = cpp.objective_hessian_host(np.float32([[1.0, np.inf, 2.0]]), None, "softmax")
    assert h.tobytes() == np.zeros((1, 3), np.float32).tobytes()      # q = (0, 1, 0): the +inf score is the maximum, not inf - inf
    h = cpp.objective_hessian_host(np.float32([[0.0, 0.0]]), None, "softmax")
    assert h.tobytes() == np.float32([[0.25, 0.25]]).tobytes()


def test_rmse_hessian_is_one_and_refusals():
    assert cpp.objective_hessian_host(np.float32([[1.0, -2.0]]), None, "rmse").tobytes() == np.ones((1, 2), np.float32).tobytes()
    with pytest.raises(Exception):
        cpp.objective_hessian_host(np.float32([1.0, 2.0]), None, "softmax")   # D == 1
    with pytest.raises(Exception):
        cpp.objective_hessian_host(np.float32([1.0]), None, "hinge")


def test_newton_sum_bits():
    for m, want in ((1, 40), (2**20, 40), (2**22 - 1, 40), (2**22, 39), (2**31 - 1, 31)):
        assert cpp.newton_sum_bits(m) == want == min(40, 62 - int(m).bit_length())
    # no sum reaches 2^62: m rows of |q(g)| <= 2^bits
    for m in (1, 3, 2**22 - 1, 2**22, 2**31 - 1):
        assert m * 2 ** cpp.newton_sum_bits(m) < 2**62


def values64(sums, bits, old, depths, l2):
    D = old.shape[1]
    out = old.copy()
    scale = 2.0 ** bits
    for l in range(old.shape[0]):
        for d in range(D):
            G = np.float64(sums[l, d]) / scale
            H = np.float64(sums[l, D + d]) / scale
            den = H + np.float64(l2)
            if sums[l, 2 * D] > 0 and depths[l] > 0 and den > 0:
                out[l, d] = np.float32(G / den)
    return out


def test_newton_values_host():
    rng = np.random.default_rng(3)
    L, D, bits = 12, 3, 40
    g = rng.uniform(-1.0, 1.0, (L, 50, D)).astype(np.float32)
    h = rng.uniform(0.0, 0.25, (L, 50, D)).astype(np.float32)
    q = lambda x: np.rint(x.astype(np.float64) * 2.0 ** bits).astype(np.int64)
    sums = np.concatenate([q(g).sum(1), q(h).sum(1), np.full((L, 1), 50, np.int64)], axis=1)
    old = rng.normal(size=(L, D)).astype(np.float32)
    depths = np.full(L, 3, np.int32)
    sums[0, 2 * D] = 0           # no row: kept
    depths[1] = 0                # depth 0: kept
    sums[2, D:2 * D] = 0         # H = 0: kept with leaf_l2 = 0, G / leaf_l2 otherwise
    sums[3, :D] = 2**61 + 12345  # beyond 2^53: the int64 -> double conversion rounds, in NumPy as in C++
    for l2 in (0.0, 1.0, 0.37, 1e-3, 1e300):
        got = cpp.newton_values_host(sums, bits, old, depths, l2)
        assert got.dtype == np.float32 and got.shape == (L, D)
        assert got.tobytes() == values64(sums, bits, old, depths, l2).tobytes(), l2
        assert got[0].tobytes() == old[0].tobytes() and got[1].tobytes() == old[1].tobytes()
    assert cpp.newton_values_host(sums, bits, old, depths, 0.0)[2].tobytes() == old[2].tobytes()
    assert cpp.newton_values_host(sums, bits, old, depths, 1.0)[2].tobytes() != old[2].tobytes()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception):
            cpp.newton_values_host(sums, bits, old, depths, bad)
    with pytest.raises(Exception):
        cpp.newton_values_host(sums[:, :-1], bits, old, depths, 1.0)


def model(D=2, **kw):
    args = dict(input_dim=4, output_dim=D, policy_dim=D, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    args.update(kw)
    m = gbrl_amd.GBRL(**args)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    return m


def test_binding_refusals_need_no_device():
    """every refusal here comes before a data set handle is resolved (ds=None would be 'null data set'), so no GPU is touched"""
    m = model()
    y = np.zeros((8, 2), np.float32)
    with pytest.raises(Exception, match="rmse"):
        m.fit_prepared(None, y, 2, leaf_update="newton")                                   # newton with rmse
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="leaf_l2"):
            m.fit_prepared(None, y, 2, objective="logistic", leaf_update="newton", leaf_l2=bad)
    with pytest.raises(Exception, match="leaf_update"):
        m.fit_prepared(None, y, 2, objective="logistic", leaf_update="hessian")            # an unknown rule
    with pytest.raises(Exception, match="null data set"):
        m.fit_prepared(None, y, 2, objective="logistic", leaf_update="newton", leaf_l2=0.0)   # past the new checks
    with pytest.raises(Exception, match="null data set"):
        m.fit_prepared(None, y, 2, objective="logistic", leaf_update="gradient")


def test_c_abi_refusals():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.gbrl_hip_objective_hessian_host.argtypes = [vp, ci, ci, ci, vp]
    lib.gbrl_hip_newton_values_host.argtypes = [vp, ci, ci, ci, vp, vp, cd, vp]
    lib.gbrl_hip_newton_sum_bits.argtypes = [C.c_int64]
    p = np.float32([0.0, 1.0])
    out = np.zeros(2, np.float32)
    assert lib.gbrl_hip_objective_hessian_host(p.ctypes.data, 2, 1, 1, out.ctypes.data) == 0
    assert out.tobytes() == cpp.objective_hessian_host(p, None, "logistic").tobytes()
    assert lib.gbrl_hip_objective_hessian_host(None, 2, 1, 1, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_objective_hessian_host(p.ctypes.data, 0, 1, 1, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_objective_hessian_host(p.ctypes.data, 2, 1, 7, out.ctypes.data) == E_INVALID
    sums = np.zeros((1, 3), np.int64)
    old = np.zeros((1, 1), np.float32)
    dep = np.ones(1, np.int32)
    assert lib.gbrl_hip_newton_values_host(sums.ctypes.data, 1, 1, 40, old.ctypes.data, dep.ctypes.data, 1.0, out.ctypes.data) == 0
    assert lib.gbrl_hip_newton_values_host(sums.ctypes.data, 1, 1, 63, old.ctypes.data, dep.ctypes.data, 1.0, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_newton_values_host(sums.ctypes.data, 1, 1, 40, old.ctypes.data, dep.ctypes.data, -1.0, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_newton_values_host(None, 1, 1, 40, old.ctypes.data, dep.ctypes.data, 1.0, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_newton_sum_bits(2**22) == 39
