"""CPU-side checks of `predict_staged` / `staged_loss` (include/gbrl_hip.h): the C symbols and the binding's methods exist, every argument
error is reported before a device is needed -- through the binding and through the C ABI -- and without a GPU a valid call fails loudly."""
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
    assert hasattr(lib, "gbrl_hip_predict_staged") and hasattr(lib, "gbrl_hip_staged_loss")
    m = _model()
    assert callable(m.predict_staged) and callable(m.staged_loss)
    # keyword names as documented
    assert "obs: object, categorical_obs: object, stops: object = None" in m.predict_staged.__doc__
    assert "obs: object, categorical_obs: object, targets: object, stops: object = None" in m.staged_loss.__doc__


def test_binding_argument_errors():
    m = _model()                      # no trees: the only legal stop is 0
    X = np.zeros((300, 4), np.float32)
    Y = np.zeros((300, 2), np.float32)
    # stops
    with pytest.raises(RuntimeError, match="stops is empty"):
        m.predict_staged(X, None, [])
    with pytest.raises(RuntimeError, match="stops is empty"):
        m.predict_staged(X, None)                      # stops=None on a model with no trees
    with pytest.raises(RuntimeError, match="stops is empty"):
        m.staged_loss(X, None, Y, stops=None)
    with pytest.raises(RuntimeError, match="strictly ascending"):
        m.predict_staged(X, None, [0, 0])
    with pytest.raises(RuntimeError, match="out of bounds"):
        m.predict_staged(X, None, [1])                 # above n_trees
    with pytest.raises(RuntimeError, match="out of bounds"):
        m.staged_loss(X, None, Y, [-1, 0])
    with pytest.raises(RuntimeError, match="out of bounds"):
        m.staged_loss(X, None, Y, stops=[0, 1])
    # targets
    with pytest.raises(RuntimeError, match="without targets"):
        m.staged_loss(X, None, None, [0])
    with pytest.raises(RuntimeError, match="Expected targets of shape"):
        m.staged_loss(X, None, np.zeros((299, 2), np.float32), [0])
    with pytest.raises(RuntimeError, match="Expected targets of shape"):
        m.staged_loss(X, None, np.zeros((300, 3), np.float32), [0])
    with pytest.raises(RuntimeError, match="Expected targets of shape"):
        m.staged_loss(X, None, np.zeros((300,), np.float32), [0])        # [n] only when output_dim == 1
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.staged_loss(X, None, Y.astype(np.float64), [0])
    with pytest.raises(RuntimeError, match="Expected dtype torch.float32"):
        m.staged_loss(X, None, (1234, (300, 2), "torch.float64", "cuda"), [0])
    # the data set errors predict gives
    for call in (lambda o, c: m.predict_staged(o, c, [0]), lambda o, c: m.staged_loss(o, c, Y, [0])):
        with pytest.raises(RuntimeError, match="without observations"):
            call(None, None)
        with pytest.raises(RuntimeError, match="Total number of features"):
            call(np.zeros((300, 3), np.float32), None)
        with pytest.raises(RuntimeError, match="Expected array of format"):
            call(X, np.zeros((300, 1)))                                  # categorical cells must be S128
    # output_dim > 128, with predict's own message
    wide = _model(output_dim=129, policy_dim=129)
    with pytest.raises(RuntimeError, match="output_dim > 128"):
        wide.predict_staged(X, None, [0])
    with pytest.raises(RuntimeError, match="output_dim > 128"):
        wide.staged_loss(X, None, np.zeros((300, 129), np.float32), [0])


def test_c_abi_errors_before_the_device_is_touched():
    m = _model()
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gbrl_hip_predict_staged.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, ci, vp, ci]
    lib.gbrl_hip_staged_loss.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, vp, ci, vp]
    h = m._handle()
    X = np.zeros((8, 4), np.float32)
    Y = np.zeros((8, 2), np.float32)
    out = np.zeros((2, 8, 2), np.float32)
    loss = np.zeros(2, np.float64)
    ok = np.array([0], np.int32)

    def staged(n, n_num, n_cat, stops, op, handle=h):
        sp = stops.ctypes.data if stops is not None and stops.size else None
        return lib.gbrl_hip_predict_staged(handle, X.ctypes.data, 0, None, 0, n, n_num, n_cat, sp, 0 if stops is None else stops.size, op, 0)

    def lossf(n, n_num, n_cat, yp, stops, lp, handle=h):
        sp = stops.ctypes.data if stops is not None and stops.size else None
        return lib.gbrl_hip_staged_loss(handle, X.ctypes.data, 0, None, 0, yp, 0, n, n_num, n_cat, sp, 0 if stops is None else stops.size, lp)

    err = lib.gbrl_hip_last_error
    assert staged(8, 3, 0, ok, out.ctypes.data) == -1 and b"Incompatible dataset" in err()
    assert staged(0, 4, 0, ok, out.ctypes.data) == -1 and b"without observations" in err()
    assert staged(8, 4, 0, ok, None) == -1 and b"without observations" in err()
    assert staged(8, 3, 1, ok, out.ctypes.data) == -1 and b"without observations" in err()      # categorical columns announced, no cells
    assert staged(8, 4, 0, None, out.ctypes.data) == -1 and b"stops is empty" in err()
    assert staged(8, 4, 0, np.array([], np.int32), out.ctypes.data) == -1 and b"stops is empty" in err()
    assert staged(8, 4, 0, np.array([1], np.int32), out.ctypes.data) == -1 and b"out of bounds" in err()
    assert staged(8, 4, 0, np.array([-1, 0], np.int32), out.ctypes.data) == -1 and b"out of bounds" in err()
    assert staged(8, 4, 0, np.array([0, 0], np.int32), out.ctypes.data) == -1 and b"strictly ascending" in err()
    assert staged(8, 4, 0, ok, out.ctypes.data, handle=None) == -1
    assert lossf(8, 3, 0, Y.ctypes.data, ok, loss.ctypes.data) == -1 and b"Incompatible dataset" in err()
    assert lossf(0, 4, 0, Y.ctypes.data, ok, loss.ctypes.data) == -1 and b"without observations" in err()
    assert lossf(8, 4, 0, None, ok, loss.ctypes.data) == -1 and b"without targets" in err()
    assert lossf(8, 4, 0, Y.ctypes.data, ok, None) == -1 and b"no output array" in err()
    assert lossf(8, 4, 0, Y.ctypes.data, None, loss.ctypes.data) == -1 and b"stops is empty" in err()
    assert lossf(8, 4, 0, Y.ctypes.data, np.array([0, 1], np.int32), loss.ctypes.data) == -1 and b"out of bounds" in err()
    assert lossf(8, 4, 0, Y.ctypes.data, np.array([0, 0], np.int32), loss.ctypes.data) == -1 and b"strictly ascending" in err()
    assert lossf(8, 4, 0, Y.ctypes.data, ok, loss.ctypes.data, handle=None) == -1
    wide = _model(output_dim=129, policy_dim=129)
    big = np.zeros((8, 129), np.float32)
    assert staged(8, 4, 0, ok, big.ctypes.data, handle=wide._handle()) != 0 and b"output_dim > 128" in err()
    assert lossf(8, 4, 0, big.ctypes.data, ok, loss.ctypes.data, handle=wide._handle()) != 0 and b"output_dim > 128" in err()


def test_a_valid_call_needs_a_device():
    """No CPU path: without a HIP device the call raises; with one, stops=[0] is the tiled bias, bit for bit, and its loss is MultiRMSE of it."""
    m = _model()
    bias = np.array([-0.0, 1.5], np.float32)
    m.set_bias(bias)
    X = np.zeros((300, 4), np.float32)
    Y = np.arange(600, dtype=np.float32).reshape(300, 2)
    if gbrl_amd.cuda_available():
        got = np.asarray(m.predict_staged(X, None, [0]))
        assert got.dtype == np.float32 and got.shape == (1, 300, 2)
        assert got[0].tobytes() == np.tile(bias, (300, 1)).tobytes()
        loss = m.staged_loss(X, None, Y, [0])
        assert loss.dtype == np.float64 and loss.shape == (1,)
        g = (np.tile(bias, (300, 1)) - Y).astype(np.float32).astype(np.float64)
        want = np.sqrt(0.5 * np.sum(g * g) / 300)
        assert abs(loss[0] - want) <= 600 * 2.0 ** -52 * want
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_staged(X, None, [0])
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.staged_loss(X, None, Y, [0])
