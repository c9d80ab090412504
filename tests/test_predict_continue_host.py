"""CPU-side checks of `predict_continue` / `predict_continue_encoded` (include/gbrl_hip.h): the C symbols and the binding's methods exist,
the argument errors that need no device are reported before the device is touched, and without a GPU a valid call fails loudly."""
import ctypes

import numpy as np
import pytest

import gbrl_amd


def _model(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile",
                grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def test_symbols_and_methods_exist():
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    assert hasattr(lib, "gbrl_hip_predict_continue") and hasattr(lib, "gbrl_hip_predict_continue_encoded")
    m = _model()
    assert callable(m.predict_continue) and callable(m.predict_continue_encoded)


def test_binding_argument_errors():
    m = _model()
    X = np.zeros((300, 4), np.float32)
    base = np.zeros((300, 2), np.float32)
    with pytest.raises(RuntimeError, match="without observations"):
        m.predict_continue(None, None, base, 0, 0)
    with pytest.raises(RuntimeError, match="without base"):
        m.predict_continue(X, None, None, 0, 0)
    with pytest.raises(RuntimeError, match="Total number of features"):
        m.predict_continue(np.zeros((300, 3), np.float32), None, base, 0, 0)
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.predict_continue(X, None, base.astype(np.float64), 0, 0)
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.predict_continue(X, np.zeros((300, 1)), base, 0, 0)            # categorical cells must be S128
    with pytest.raises(RuntimeError, match="Expected base of shape"):
        m.predict_continue(X, None, np.zeros((299, 2), np.float32), 0, 0)
    with pytest.raises(RuntimeError, match="Expected base of shape"):
        m.predict_continue(X, None, np.zeros((300,), np.float32), 0, 0)  # [n] only when output_dim == 1
    with pytest.raises(RuntimeError, match="Expected dtype torch.float32"):
        m.predict_continue(X, None, (1234, (300, 2), "torch.float16", "cuda"), 0, 0)
    with pytest.raises(RuntimeError, match="Expected dtype torch.int32"):
        m.predict_continue_encoded(X[:, :3], (1234, (300, 1), "torch.int64", "cuda"), 0, base, 0, 0)
    # tree ranges the (empty) ensemble does not hold: an error, never a silent no-op -- and reported before the device is touched
    for a, b in ((0, 1), (1, 0), (-1, 0), (0, -1)):
        with pytest.raises(RuntimeError, match="invalid tree range"):
            m.predict_continue(X, None, base, a, b)


def test_c_abi_errors_before_the_device_is_touched():
    m = _model()
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gbrl_hip_predict_continue.argtypes = [vp, vp, ci, vp, ci] + [ci] * 5 + [vp, ci, vp, ci]
    lib.gbrl_hip_predict_continue_encoded.argtypes = [vp, vp, ci, vp, ci, ctypes.c_uint64] + [ci] * 5 + [vp, ci, vp, ci]
    h = m._handle()
    X = np.zeros((8, 4), np.float32)
    base = np.zeros((8, 2), np.float32)
    out = np.zeros((8, 2), np.float32)
    call = lambda n, n_num, n_cat, a, b, bp, op: lib.gbrl_hip_predict_continue(h, X.ctypes.data, 0, None, 0, n, n_num, n_cat, a, b, bp, 0, op, 0)
    assert call(8, 3, 0, 0, 0, base.ctypes.data, out.ctypes.data) == -1 and b"Incompatible dataset" in lib.gbrl_hip_last_error()
    assert call(0, 4, 0, 0, 0, base.ctypes.data, out.ctypes.data) == -1 and b"without observations" in lib.gbrl_hip_last_error()
    assert call(8, 4, 0, 0, 0, base.ctypes.data, None) == -1 and b"without observations" in lib.gbrl_hip_last_error()
    assert call(8, 4, 0, 0, 0, None, out.ctypes.data) == -1 and b"no base prediction" in lib.gbrl_hip_last_error()
    assert call(8, 4, 0, 0, 1, base.ctypes.data, out.ctypes.data) == -1 and b"invalid tree range" in lib.gbrl_hip_last_error()
    assert call(8, 4, 0, 2, 0, base.ctypes.data, out.ctypes.data) == -1 and b"invalid tree range" in lib.gbrl_hip_last_error()
    assert lib.gbrl_hip_predict_continue(None, X.ctypes.data, 0, None, 0, 8, 4, 0, 0, 0, base.ctypes.data, 0, out.ctypes.data, 0) == -1
    # categorical features announced without ids
    mc = _model()
    rc = lib.gbrl_hip_predict_continue_encoded(mc._handle(), X.ctypes.data, 0, None, 0, 0, 8, 3, 1, 0, 0, base.ctypes.data, 0, out.ctypes.data, 0)
    assert rc == -1 and b"without observations" in lib.gbrl_hip_last_error()
    wide = _model(output_dim=129, policy_dim=129)
    rc = lib.gbrl_hip_predict_continue(wide._handle(), X.ctypes.data, 0, None, 0, 8, 4, 0, 0, 0, base.ctypes.data, 0, out.ctypes.data, 0)
    assert rc != 0 and b"output_dim > 128" in lib.gbrl_hip_last_error()


def test_a_valid_call_needs_a_device():
    """No CPU path: without a HIP device the call raises; with one, an empty range hands the base back."""
    m = _model()
    X = np.zeros((300, 4), np.float32)
    base = np.arange(600, dtype=np.float32).reshape(300, 2)
    if gbrl_amd.cuda_available():
        assert np.asarray(m.predict_continue(X, None, base, 0, 0)).tobytes() == base.tobytes()
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_continue(X, None, base, 0, 0)
