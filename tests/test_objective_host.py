"""CPU-side checks of the classification objectives behind fit_prepared(objective=), GBRL.objective_gradient and gbrl_cpp.objective_gradient_host
(include/gbrl_hip.h, "Classification objectives"; gbrl_amd/csrc/objective_core.h).  The gradient rule is one definition for host and device, so
it is held here, on the host, to a float64 NumPy evaluation of the formulas; tests/test_gpu_objective.py then holds the device to these bits."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

E_INVALID = -1
C_SYMBOLS = ("gbrl_hip_fit_prepared_objective", "gbrl_hip_objective_gradient", "gbrl_hip_objective_gradient_host", "gbrl_hip_objective_exp_host")
OBJ = {"rmse": 0, "logistic": 1, "softmax": 2}
host = gbrl_amd.gbrl_cpp.objective_gradient_host
obj_exp = gbrl_amd.gbrl_cpp.objective_exp_host


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_objective_gradient_host.argtypes = [vp, vp, ci, ci, ci, vp]
    lib.gbrl_hip_objective_gradient.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp]
    lib.gbrl_hip_objective_exp_host.argtypes = [vp, ci, vp, vp]
    return lib


def sweep():
    """at least 2^20 float32 arguments in [-104, 0]: a dense grid, every power of two with its two neighbours, both zeros, the ends"""
    grid = np.linspace(-104.0, 0.0, 2**20 + 1).astype(np.float32)
    pw = -np.ldexp(np.float32(1.0), np.arange(-149, 7)).astype(np.float32)   # -2^-149 .. -2^6
    near = np.concatenate([pw, np.nextafter(pw, np.float32(0)), np.nextafter(pw, np.float32(-200))])
    t = np.concatenate([grid, near, np.float32([-0.0, 0.0, -104.0, -87.0, -88.0, -103.5])])
    return np.unique(t[(t >= -104.0) & (t <= 0.0)])


def rel_err(t):
    want = np.exp(t.astype(np.float64))
    got = obj_exp(t)
    assert got.dtype == np.float64
    return np.abs(got - want) / want


def softmax64(p, y):
    p = p.astype(np.float64)
    e = np.exp(p - p.max(axis=1, keepdims=True))
    q = e / e.sum(axis=1, keepdims=True)
    q[np.arange(p.shape[0]), y] -= 1.0
    return q


def logistic64(p, y):
    p = p.astype(np.float64)
    e = np.exp(-np.abs(p))
    return np.where(p >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) - y.astype(np.float64)


def test_c_symbols_and_python_names():
    lib = _lib()
    for name in C_SYMBOLS:
        assert hasattr(lib, name), name
    assert hasattr(gbrl_amd.GBRL, "objective_gradient") and "objective='rmse'" in gbrl_amd.GBRL.fit_prepared.__doc__
    for rounded in (False, True):
        assert obj_exp(np.float32([0.0, -0.0]), rounded=rounded).tolist() == [1.0, 1.0]
        z = obj_exp(np.float32([-104.5, -1e30, -np.inf]), rounded=rounded)
        assert z.tolist() == [0.0, 0.0, 0.0] and not np.signbit(z).any()   # +0 below -104


def test_obj_exp_relative_error_on_the_whole_range():
    """obj_exp is the value p * 2^k itself (a float32 significand, the exponent applied exactly, handed out as a double): relative error
    against numpy.exp in float64 at most 2^-22 on all of [-104, 0].  Measured maximum: 2^-23.59 (7.91e-8)."""
    t = sweep()
    assert t.size >= 2**20 and t.min() == -104.0 and t.max() == 0.0
    err = rel_err(t)
    print("obj_exp: %d points, max relative error %.4g = 2^%.3f at t = %r" % (t.size, err.max(), np.log2(err.max()), t[err.argmax()]))
    assert err.max() <= 2.0**-22


def test_the_gradients_use_obj_exp_rounded_once_to_float32():
    """obj_exp_f32, computed without float64 on host and device, is float32(obj_exp) bit for bit on the whole sweep -- nearest-even into the
    subnormals below t = -87.34, +0 where the value is at most 2^-150 -- so the bound above is the bound on the significand the gradients see;
    a subnormal result is within 2^-149 absolute of exp(t) (measured: 1.05e-45)."""
    t = sweep()
    f = obj_exp(t, rounded=True)
    assert f.dtype == np.float32 and f.tobytes() == obj_exp(t).astype(np.float32).tobytes()
    sub = np.exp(t.astype(np.float64)) < 2.0**-126
    assert sub.sum() > 2**17
    err = np.abs(f[sub].astype(np.float64) - np.exp(t[sub].astype(np.float64)))
    print("obj_exp_f32, subnormal results: %d points, max absolute error %.4g (2^-149 = %.4g)" % (sub.sum(), err.max(), 2.0**-149))
    assert err.max() <= 2.0**-149
    # the logistic gradient at y = 0 and p <= 0 is e / (1 + e): e itself wherever 1 + e rounds to 1
    p = t[t <= -20]
    assert host(p, np.zeros_like(p), "logistic").tobytes() == obj_exp(p, rounded=True).tobytes()


@pytest.mark.parametrize("D", [1, 2, 3, 8, 33, 128])
def test_gradient_against_float64(D):
    """|p| <= 16, n = 257.  Bounds: softmax (D + 16) * 2^-24, logistic 16 * 2^-24 -- obj_exp within 2^-22 (4 units), the rounding of p - m
    0.37, the sequential sum D - 1, the division and the subtraction one each.  Measured maxima (units of 2^-24): logistic 1.48;
    softmax 1.49 (D = 2), 2.01 (3), 2.24 (8), 4.33 (33), 2.25 (128)."""
    rng = np.random.default_rng(100 + D)
    n = 257
    p = rng.uniform(-16, 16, (n, D)).astype(np.float32)
    p[0] = 16.0; p[1, ::2] = -16.0
    yl = (rng.random((n, D)) < 0.5).astype(np.float32)
    g = host(p, yl, "logistic")
    assert g.dtype == np.float32 and g.shape == p.shape
    err = np.abs(g.astype(np.float64) - logistic64(p, yl)).max()
    print("logistic D=%d: max |error| %.3f * 2^-24 (bound 16)" % (D, err * 2.0**24))
    assert err <= 16 * 2.0**-24
    if D >= 2:
        y = rng.integers(0, D, n).astype(np.int32)
        g = host(p, y, "softmax")
        err = np.abs(g.astype(np.float64) - softmax64(p, y)).max()
        print("softmax  D=%d: max |error| %.3f * 2^-24 (bound %d)" % (D, err * 2.0**24, D + 16))
        assert err <= (D + 16) * 2.0**-24
    # rmse: one float32 subtraction
    assert np.array_equal(host(p, yl, "rmse"), p - yl)


def test_one_output_takes_vectors_and_c_equals_python():
    lib = _lib()
    p = np.float32([-3.0, 0.5, 2.0]); y = np.float32([0, 1, 1])
    g = host(p, y, "logistic")
    assert g.shape == (3,) and np.array_equal(g, host(p[:, None], y[:, None], "logistic")[:, 0])
    out = np.zeros(3, np.float32)
    assert lib.gbrl_hip_objective_gradient_host(p.ctypes.data, y.ctypes.data, 3, 1, OBJ["logistic"], out.ctypes.data) == 0
    assert np.array_equal(out, g)


def test_logistic_edge_inputs():
    p = np.float32([0.0, -0.0, 88, -88, 104, -104, 1e30, -1e30, np.inf, -np.inf])
    for yv in (0.0, 1.0, 0.25):
        g = host(p, np.full(p.shape, yv, np.float32), "logistic")
        assert np.isfinite(g).all() and (np.abs(g) <= 1).all(), (yv, g)
    g = host(p, np.zeros_like(p), "logistic")
    assert g[0] == 0.5 and g[1] == 0.5 and g[2] == 1.0 and g[4] == 1.0 and g[6] == 1.0 and g[5] == 0.0 and g[7] == 0.0 and 0 < g[3] < 1e-37


@pytest.mark.parametrize("D", [2, 3, 8, 33, 128])
def test_softmax_edge_inputs(D):
    rng = np.random.default_rng(D)
    n = 64
    p = rng.uniform(-16, 16, (n, D)).astype(np.float32)
    y = rng.integers(0, D, n).astype(np.int32)
    p[0] = 3.25                      # equal scores
    p[1] = -0.0; p[1, 0] = 0.0       # both zeros are equal scores
    p[2, (int(y[2]) + 1) % D] = -np.inf   # a score of -inf: probability 0
    p[3, 0] = np.inf                 # a score of +inf is the maximum: probability 1
    g = host(p, y, "softmax")
    assert np.isfinite(g).all()
    assert (np.abs(g.astype(np.float64).sum(axis=1)) <= D * 2.0**-23).all()
    onehot = np.zeros((n, D), np.float32); onehot[np.arange(n), y] = 1
    q = np.float32(1.0) / np.float32(D)
    assert np.array_equal(g[0], q - onehot[0]) and np.array_equal(g[1], q - onehot[1])
    assert g[2, (int(y[2]) + 1) % D] == 0.0
    assert np.array_equal(g[3], (np.arange(D) == 0).astype(np.float32) - onehot[3])


def test_refusals_that_need_no_device():
    lib = _lib()
    err = lib.gbrl_hip_last_error
    p = np.zeros((4, 3), np.float32); y = np.zeros((4, 3), np.float32); lab = np.zeros(4, np.int32); out = np.zeros((4, 3), np.float32)
    P, Y, L, O = p.ctypes.data, y.ctypes.data, lab.ctypes.data, out.ctypes.data
    with pytest.raises(RuntimeError, match="Invalid objective"):
        host(p, y, "hinge")
    assert lib.gbrl_hip_objective_gradient_host(P, Y, 4, 3, 7, O) == E_INVALID and b"unknown objective" in err()
    with pytest.raises(RuntimeError, match="output_dim >= 2"):
        host(p[:, :1].copy(), lab, "softmax")
    assert lib.gbrl_hip_objective_gradient_host(P, L, 4, 1, OBJ["softmax"], O) == E_INVALID and b"output_dim >= 2" in err()
    for a, b, c in ((None, Y, O), (P, None, O), (P, Y, None)):
        assert lib.gbrl_hip_objective_gradient_host(a, b, 4, 3, OBJ["logistic"], c) == E_INVALID and b"null argument" in err()
    assert lib.gbrl_hip_objective_gradient_host(P, Y, 0, 3, OBJ["logistic"], O) == E_INVALID and b"no rows" in err()
    assert lib.gbrl_hip_objective_exp_host(None, 4, None, O) == E_INVALID and b"null argument" in err()
    assert lib.gbrl_hip_objective_exp_host(P, 4, None, None) == E_INVALID and b"null argument" in err()
    # labels: out of range (the first one found is named), the wrong type, the wrong shape
    for bad in (3, -1):
        lab2 = lab.copy(); lab2[2] = bad
        with pytest.raises(RuntimeError, match=r"label %d \(row 2\) is outside \[0, 3\)" % bad):
            host(p, lab2, "softmax")
    with pytest.raises(RuntimeError, match="Expected array of format"):
        host(p, y, "softmax")                      # float targets where labels are wanted
    with pytest.raises(RuntimeError, match="Expected array of format"):
        host(p, lab, "logistic")                   # ... and the reverse
    with pytest.raises(RuntimeError, match="int32 class labels of shape"):
        host(p, np.zeros((4, 3), np.int32), "softmax")
    assert np.array_equal(out, np.zeros((4, 3), np.float32))
    # a model is needed for the device call, and refuses the same before it touches a device
    m = gbrl_amd.GBRL(input_dim=4, output_dim=1, policy_dim=1, max_depth=2, n_bins=16, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cpu", batch_size=8)
    with pytest.raises(RuntimeError, match="output_dim >= 2"):
        m.objective_gradient(np.zeros(4, np.float32), lab, "softmax")
    with pytest.raises(RuntimeError, match="Invalid objective"):
        m.objective_gradient(np.zeros(4, np.float32), np.zeros(4, np.float32), "hinge")
    with pytest.raises(RuntimeError, match="Invalid objective"):
        m.fit_prepared(None, np.zeros(4, np.float32), 3, objective="hinge")
    with pytest.raises(RuntimeError, match="output_dim >= 2"):
        m.fit_prepared(None, lab, 3, objective="softmax")
