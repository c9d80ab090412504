"""CPU-side checks of `refit_leaves` (include/gbrl_hip.h): the C symbol and the binding's method exist, the ABI version is unchanged, and every
argument error of the contract is reported before a device is needed -- through the binding and through the C ABI with the documented status --
and leaves the model's file bytes as they were.  No GPU here, so the models with trees come from the reference's files in tests/golden."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd
from helpers import load_golden

E_INVALID, E_UNSUPPORTED = -1, -5


def _empty(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile",
                grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def _loaded(name, tmp_path):
    case, g, (X, Xc, _, _) = load_golden(name)
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p)), X, Xc


def _file_bytes(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_refit_leaves.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, C.c_double, vp]
    lib.gbrl_hip_refit_leaves.restype = ci
    lib.gbrl_hip_set_collective.argtypes = [vp, vp]
    return lib


def test_symbol_method_and_abi_version():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    assert hasattr(lib, "gbrl_hip_refit_leaves")
    lib.gbrl_hip_abi_version.restype = C.c_int
    assert lib.gbrl_hip_abi_version() == 1
    m = _empty()
    assert callable(m.refit_leaves)
    doc = m.refit_leaves.__doc__
    # keyword names as documented (how the float type of decay_rate is spelt depends on the pybind11 version)
    sig = doc.splitlines()[0]
    assert "obs: object, categorical_obs: object, targets: object, start_tree_idx: object = 0, stop_tree_idx: object = 0, decay_rate: " in sig
    assert sig.endswith("= 0.0) -> float")


def test_a_model_without_trees_is_refused(tmp_path):
    m = _empty()
    before = _file_bytes(m, tmp_path)
    X, Y = np.zeros((8, 4), np.float32), np.zeros((8, 2), np.float32)
    with pytest.raises(RuntimeError, match="has no trees"):
        m.refit_leaves(X, None, Y)
    with pytest.raises(RuntimeError, match="has no trees"):
        m.refit_leaves(X, None, Y, 0, 1, 0.5)
    assert _file_bytes(m, tmp_path) == before


@pytest.mark.parametrize("name", ["obl_l2_q", "grd_cos_q_ac"])
def test_binding_argument_errors(name, tmp_path):
    m, X, _ = _loaded(name, tmp_path)
    T, D = m.get_num_trees(), np.asarray(m.get_bias()).size
    assert T >= 3
    X = np.ascontiguousarray(X[:16])
    Y = np.zeros((16, D), np.float32)
    before = _file_bytes(m, tmp_path)
    # the range: stop == 0 means T; after that 0 <= start < stop <= T
    for a, b in ((0, T + 1), (2, 2), (2, 1), (T, 0), (T + 1, 0), (-1, 2), (0, -1)):
        with pytest.raises(RuntimeError, match="invalid tree range"):
            m.refit_leaves(X, None, Y, a, b)
    # targets: missing, another shape, another type
    with pytest.raises(RuntimeError, match="without targets"):
        m.refit_leaves(X, None, None)
    for bad in (np.zeros((15, D), np.float32), np.zeros((16, D + 1), np.float32), np.zeros((16, D, 1), np.float32)):
        with pytest.raises(RuntimeError, match="Expected targets of shape"):
            m.refit_leaves(X, None, bad)
    if D > 1:
        with pytest.raises(RuntimeError, match="Expected targets of shape"):
            m.refit_leaves(X, None, np.zeros(16, np.float32))
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.refit_leaves(X, None, Y.astype(np.float64))
    # decay_rate outside [0, 1], or NaN
    for decay in (-0.25, 1.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="decay_rate"):
            m.refit_leaves(X, None, Y, 0, 0, decay)
    # the data set errors of predict
    with pytest.raises(RuntimeError, match="without observations"):
        m.refit_leaves(None, None, Y)
    with pytest.raises(RuntimeError, match="Total number of features"):
        m.refit_leaves(np.zeros((16, X.shape[1] - 1), np.float32), None, Y)
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.refit_leaves(X.astype(np.float64), None, Y)
    assert _file_bytes(m, tmp_path) == before
    # a legal call gets as far as the device: with no GPU that is the error, and no other -- and it changes nothing either
    if not gbrl_amd.cuda_available():
        for args in ((), (1, T), (0, 0, 0.5), (0, 0, 1.0)):
            with pytest.raises(RuntimeError, match="no HIP device"):
                m.refit_leaves(X, None, Y, *args)
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.refit_leaves(X, None, Y, start_tree_idx=1, stop_tree_idx=2, decay_rate=0.3)
        assert _file_bytes(m, tmp_path) == before


def test_c_abi_errors_before_the_device_is_touched(tmp_path):
    m, X, _ = _loaded("obl_l2_q", tmp_path)
    T, F, D = m.get_num_trees(), X.shape[1], np.asarray(m.get_bias()).size
    lib = _lib()
    err = lib.gbrl_hip_last_error
    h = m._handle()
    X = np.ascontiguousarray(X[:8])
    Y = np.zeros((8, D), np.float32)
    loss = C.c_double(-7.0)
    before = _file_bytes(m, tmp_path)

    def refit(n=8, n_num=F, n_cat=0, a=0, b=0, decay=0.0, y=Y.ctypes.data, out=C.addressof(loss), handle=h):
        return lib.gbrl_hip_refit_leaves(handle, X.ctypes.data, 0, None, 0, y, 0, n, n_num, n_cat, a, b, decay, out)

    for a, b in ((0, T + 1), (2, 2), (2, 1), (T, 0), (-1, 2), (0, -1)):
        assert refit(a=a, b=b) == E_INVALID and b"invalid tree range" in err(), (a, b)
    assert refit(y=None) == E_INVALID and b"without targets" in err()
    assert refit(out=None) == E_INVALID and b"loss" in err()
    for decay in (-1e-9, 1.0000001, float("nan")):
        assert refit(decay=decay) == E_INVALID and b"decay_rate" in err(), decay
    assert refit(n_num=F - 1) == E_INVALID and b"Incompatible dataset" in err()
    assert refit(n_num=F - 1, n_cat=1) == E_INVALID and b"Incompatible dataset" in err()
    assert refit(n=0) == E_INVALID and b"without observations" in err()
    assert refit(handle=None) == E_INVALID
    empty = _empty(input_dim=F, output_dim=D, policy_dim=D)
    assert refit(handle=empty._handle()) == E_INVALID and b"has no trees" in err()
    assert loss.value == -7.0                                              # no refused call wrote the loss
    assert _file_bytes(m, tmp_path) == before
    if not gbrl_amd.cuda_available():
        assert refit() == -2 and b"no HIP device" in err()                 # GBRL_HIP_E_NO_DEVICE: the arguments were fine
        assert _file_bytes(m, tmp_path) == before


def test_a_row_sharded_model_is_unsupported(tmp_path):
    """Collective hooks make the model row-sharded: the leaf sums would need an exchange per tree, which is out of scope."""
    reduce_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)

    class Collective(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    m, X, _ = _loaded("obl_l2_q", tmp_path)
    D = np.asarray(m.get_bias()).size
    X = np.ascontiguousarray(X[:8])
    Y = np.zeros((8, D), np.float32)
    lib = _lib()
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    before = _file_bytes(m, tmp_path)
    assert lib.gbrl_hip_set_collective(m._handle(), C.byref(coll)) == 0, lib.gbrl_hip_last_error()
    try:
        loss = C.c_double(-7.0)
        rc = lib.gbrl_hip_refit_leaves(m._handle(), X.ctypes.data, 0, None, 0, Y.ctypes.data, 0, 8, X.shape[1], 0, 0, 0, 0.0, C.addressof(loss))
        assert rc == E_UNSUPPORTED and b"row-sharded" in lib.gbrl_hip_last_error()
        with pytest.raises(RuntimeError, match="row-sharded"):
            m.refit_leaves(X, None, Y)
        assert loss.value == -7.0
    finally:
        assert lib.gbrl_hip_set_collective(m._handle(), None) == 0
    assert _file_bytes(m, tmp_path) == before


def test_more_than_128_outputs_are_unsupported(tmp_path):
    """As in predict_continue: a model with trees and 257 outputs is refused with the unsupported status, before the device."""
    from shap_edges import fixture, load_model
    name = "host_d4_D257_obl"
    m = load_model(name, tmp_path)
    X = fixture(name)[2]
    D = np.asarray(m.get_bias()).size
    assert D > 128 and m.get_num_trees() >= 1
    X = np.ascontiguousarray(X[:8])
    Y = np.zeros((8, D), np.float32)
    before = _file_bytes(m, tmp_path)
    with pytest.raises(RuntimeError, match="output_dim > 128"):
        m.refit_leaves(X, None, Y)
    lib = _lib()
    loss = C.c_double(0.0)
    rc = lib.gbrl_hip_refit_leaves(m._handle(), X.ctypes.data, 0, None, 0, Y.ctypes.data, 0, 8, X.shape[1], 0, 0, 0, 0.0, C.addressof(loss))
    assert rc == E_UNSUPPORTED and b"output_dim > 128" in lib.gbrl_hip_last_error()
    assert _file_bytes(m, tmp_path) == before


def test_a_greedy_tree_of_depth_0_in_or_right_before_the_range_is_unsupported(tmp_path):
    """A greedy leaf of depth 0 never passes: predict_continue's walk applies a leaf of the NEXT tree at the stump's rate, a value the refit
    does not know yet, so the documented chain cannot be followed.  The fixture's trees are [full, stump, full]."""
    from shap_edges import fixture, load_model
    name = "t64_d12_D3_grd_stump"
    m = load_model(name, tmp_path)
    e = m.get_ensemble_data()
    ti, dep = np.asarray(e["tree_indices"]), np.asarray(e["depths"])
    assert m.get_num_trees() == 3 and len(dep) > 3 and dep[ti[1]] == 0 and ti[2] - ti[1] == 1, "the fixture is not [full, stump, full] greedy"
    X = np.ascontiguousarray(fixture(name)[2][:8])
    D = np.asarray(m.get_bias()).size
    Y = np.zeros((8, D), np.float32)
    before = _file_bytes(m, tmp_path)
    lib = _lib()
    loss = C.c_double(-7.0)
    for a, b in ((0, 0), (0, 2), (1, 2), (1, 0), (2, 3)):                  # (2, 3): the stump is tree start - 1
        with pytest.raises(RuntimeError, match="depth 0"):
            m.refit_leaves(X, None, Y, a, b)
        rc = lib.gbrl_hip_refit_leaves(m._handle(), X.ctypes.data, 0, None, 0, Y.ctypes.data, 0, 8, X.shape[1], 0, a, b, 0.0, C.addressof(loss))
        assert rc == E_UNSUPPORTED and b"depth 0" in lib.gbrl_hip_last_error(), (a, b)
    assert loss.value == -7.0 and _file_bytes(m, tmp_path) == before
    if not gbrl_amd.cuda_available():                                       # the tree in front of the stump may be refitted
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.refit_leaves(X, None, Y, 0, 1)
