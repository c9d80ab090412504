"""CPU-side checks of prepared data sets (include/gbrl_hip.h: gbrl_hip_dataset_*, gbrl_hip_step_prepared; Python: GBRL.prepare_dataset,
GBRL.step_prepared, class PreparedDataset): the symbols exist, the ABI version is unchanged, the keyword names are the documented ones, and
every refusal that can be met without a data set in hand is reported before a device is needed -- through the binding and through the C ABI
with the documented status -- and leaves the model's file bytes as they were.  No GPU here, so the models with trees come from the reference's
files in tests/golden; the refusals that need a live data set (another n_bins, generator or width, misshapen grads, m == 0, out-of-range rows)
are in tests/test_gpu_prepared.py."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd
from helpers import load_golden

E_INVALID, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -5
C_SYMBOLS = ("gbrl_hip_dataset_create", "gbrl_hip_dataset_destroy", "gbrl_hip_dataset_info", "gbrl_hip_dataset_thresholds", "gbrl_hip_dataset_codes",
             "gbrl_hip_step_prepared")


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
    lib.gbrl_hip_dataset_create.argtypes = [vp, vp, ci, ci, ci]
    lib.gbrl_hip_dataset_create.restype = vp
    lib.gbrl_hip_dataset_last_status.restype = ci
    lib.gbrl_hip_dataset_destroy.argtypes = [vp]
    lib.gbrl_hip_dataset_destroy.restype = None
    lib.gbrl_hip_dataset_info.argtypes = [vp, vp]
    lib.gbrl_hip_dataset_thresholds.argtypes = [vp, vp]
    lib.gbrl_hip_dataset_codes.argtypes = [vp, vp, ci, ci, vp]
    lib.gbrl_hip_step_prepared.argtypes = [vp, vp, vp, ci, vp, ci, ci]
    lib.gbrl_hip_set_collective.argtypes = [vp, vp]
    return lib


def test_symbols_names_and_abi_version():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for sym in C_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.gbrl_hip_abi_version.restype = C.c_int
    assert lib.gbrl_hip_abi_version() == 1
    assert gbrl_amd.PreparedDataset is gbrl_amd.gbrl_cpp.PreparedDataset
    for prop in ("n_rows", "n_features", "n_bins", "generator_type", "nbytes"):
        assert isinstance(getattr(gbrl_amd.PreparedDataset, prop), property), prop
    assert callable(gbrl_amd.PreparedDataset.thresholds)
    assert "rows: object = None" in gbrl_amd.PreparedDataset.codes.__doc__.splitlines()[0]
    m = _empty()
    assert m.prepare_dataset.__doc__.splitlines()[0].startswith("prepare_dataset(self: gbrl_cpp.GBRL, obs: object) -> gbrl_cpp.PreparedDataset")
    assert "ds: object, grads: object, rows: object = None) -> None" in m.step_prepared.__doc__.splitlines()[0]


def test_a_legal_prepare_dataset_needs_the_device_and_nothing_else(tmp_path):
    """(With a GPU present the legal calls run in tests/test_gpu_prepared.py.)"""
    if not gbrl_amd.cuda_available():
        m = _empty()
        before = _file_bytes(m, tmp_path)
        X = np.zeros((8, 4), np.float32)
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.prepare_dataset(X)
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.prepare_dataset(obs=X)
        lib = _lib()
        assert lib.gbrl_hip_dataset_create(m._handle(), X.ctypes.data, 0, 8, 4) is None
        assert lib.gbrl_hip_dataset_last_status() == E_NO_DEVICE and b"no HIP device" in lib.gbrl_hip_last_error()
        loaded, Xg, _ = _loaded("grd_cos_q_ac", tmp_path)
        with pytest.raises(RuntimeError, match="no HIP device"):
            loaded.prepare_dataset(np.ascontiguousarray(Xg[:16]))
        assert _file_bytes(m, tmp_path) == before


def test_prepare_dataset_argument_errors(tmp_path):
    m, X, _ = _loaded("obl_l2_q", tmp_path)
    F = X.shape[1]
    X = np.ascontiguousarray(X[:16])
    before = _file_bytes(m, tmp_path)
    lib = _lib()
    err = lib.gbrl_hip_last_error
    h = m._handle()

    def create(obs=X.ctypes.data, n=16, n_num=F, handle=h):
        ds = lib.gbrl_hip_dataset_create(handle, obs, 0, n, n_num)
        assert ds is None
        return lib.gbrl_hip_dataset_last_status()

    assert create(n_num=F - 1) == E_INVALID and b"Incompatible dataset" in err()
    assert create(obs=None) == E_INVALID and b"without obs" in err()
    assert create(n=0) == E_INVALID and b"without obs" in err()
    assert create(handle=None) == E_INVALID and b"null model" in err()
    fresh = _empty(input_dim=F)
    assert create(n_num=F + 1, handle=fresh._handle()) == E_INVALID and b"Total number of features" in err()
    with pytest.raises(RuntimeError, match="Incompatible dataset|Total number of features"):
        m.prepare_dataset(np.zeros((16, F - 1), np.float32))
    with pytest.raises(RuntimeError, match="without obs"):
        m.prepare_dataset(None)
    with pytest.raises(RuntimeError, match="Expected array of format"):
        m.prepare_dataset(X.astype(np.float64))
    assert _file_bytes(m, tmp_path) == before


def test_categorical_models_and_cells_are_unsupported(tmp_path):
    """Categorical split candidates depend on the step's gradients: nothing about them can be prepared ahead of a step."""
    m, X, Xc = _loaded("obl_l2_q_cat", tmp_path)
    md = m.get_metadata()
    assert Xc is not None and Xc.shape[1] > 0 and m.get_num_trees() > 0      # the file's metadata has latched its categorical columns
    X = np.ascontiguousarray(X[:16])
    before = _file_bytes(m, tmp_path)
    lib = _lib()
    with pytest.raises(RuntimeError, match="categorical columns"):
        m.prepare_dataset(X)
    assert lib.gbrl_hip_dataset_create(m._handle(), X.ctypes.data, 0, 16, X.shape[1]) is None
    assert lib.gbrl_hip_dataset_last_status() == E_UNSUPPORTED and b"categorical columns" in lib.gbrl_hip_last_error()
    # an S128 argument, on any model
    with pytest.raises(RuntimeError, match="categorical columns"):
        m.prepare_dataset(np.ascontiguousarray(Xc[:16]))
    with pytest.raises(RuntimeError, match="categorical columns"):
        _empty().prepare_dataset((12345, (16, 4), "S128", "cuda"))
    # a step on such a model is refused with the same status, whatever the data set argument is checked for first
    G = np.zeros((16, md["output_dim"]), np.float32)
    rc = lib.gbrl_hip_step_prepared(m._handle(), None, G.ctypes.data, 0, None, 0, 16)
    assert rc == E_INVALID and b"null data set" in lib.gbrl_hip_last_error()
    assert _file_bytes(m, tmp_path) == before


def test_a_row_sharded_model_is_unsupported(tmp_path):
    """Collective hooks make the model row-sharded: the thresholds of the batch would need the exchange."""
    reduce_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)

    class Collective(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    m, X, _ = _loaded("obl_l2_q", tmp_path)
    X = np.ascontiguousarray(X[:8])
    lib = _lib()
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    before = _file_bytes(m, tmp_path)
    assert lib.gbrl_hip_set_collective(m._handle(), C.byref(coll)) == 0, lib.gbrl_hip_last_error()
    try:
        assert lib.gbrl_hip_dataset_create(m._handle(), X.ctypes.data, 0, 8, X.shape[1]) is None
        assert lib.gbrl_hip_dataset_last_status() == E_UNSUPPORTED and b"collective hooks" in lib.gbrl_hip_last_error()
        with pytest.raises(RuntimeError, match="collective hooks"):
            m.prepare_dataset(X)
    finally:
        assert lib.gbrl_hip_set_collective(m._handle(), None) == 0
    assert _file_bytes(m, tmp_path) == before


def test_step_limits_keep_their_messages(tmp_path):
    """n_bins beyond the u16 codes: the message step() gives, with the unsupported status, before the device."""
    m = _empty(n_bins=70000)
    X = np.zeros((8, 4), np.float32)
    before = _file_bytes(m, tmp_path)
    with pytest.raises(RuntimeError, match=r"n_bins must be in \[1, 65534\]"):
        m.prepare_dataset(X)
    lib = _lib()
    assert lib.gbrl_hip_dataset_create(m._handle(), X.ctypes.data, 0, 8, 4) is None
    assert lib.gbrl_hip_dataset_last_status() == E_UNSUPPORTED
    assert _file_bytes(m, tmp_path) == before
    with pytest.raises(RuntimeError, match=r"n_bins must be in \[1, 65534\]"):   # step's own message (it latches the column counts first)
        m.step(X, None, np.zeros((8, 2), np.float32))


@pytest.mark.parametrize("name", ["obl_l2_q", "grd_cos_q_ac"])
def test_a_null_or_destroyed_data_set_is_an_argument_error(name, tmp_path):
    m, X, _ = _loaded(name, tmp_path)
    D = np.asarray(m.get_bias()).size
    G = np.zeros((16, D), np.float32)
    rows = np.arange(16, dtype=np.int32)
    before = _file_bytes(m, tmp_path)
    lib = _lib()
    err = lib.gbrl_hip_last_error
    # the binding: None is the null data set; anything that is not a PreparedDataset is a type error of the call
    with pytest.raises(RuntimeError, match="null data set"):
        m.step_prepared(None, G)
    with pytest.raises(RuntimeError, match="null data set"):
        m.step_prepared(ds=None, grads=G, rows=rows)
    with pytest.raises((RuntimeError, TypeError)):
        m.step_prepared(object(), G)
    # the C ABI: NULL, and a handle the library does not (or no longer) know -- never dereferenced
    stale = C.create_string_buffer(64)
    info = C.create_string_buffer(64)
    out = np.zeros(16 * 16, np.uint16)
    for ds, what in ((None, b"null data set"), (C.addressof(stale), b"destroyed")):
        assert lib.gbrl_hip_step_prepared(m._handle(), ds, G.ctypes.data, 0, None, 0, 16) == E_INVALID and what in err()
        assert lib.gbrl_hip_step_prepared(m._handle(), ds, G.ctypes.data, 0, rows.ctypes.data, 0, 16) == E_INVALID and what in err()
        assert lib.gbrl_hip_dataset_info(ds, info) == E_INVALID and what in err()
        assert lib.gbrl_hip_dataset_thresholds(ds, out.ctypes.data) == E_INVALID and what in err()
        assert lib.gbrl_hip_dataset_codes(ds, None, 0, 0, out.ctypes.data) == E_INVALID and what in err()
        lib.gbrl_hip_dataset_destroy(ds)                                    # ignored: not a data set of this library
    assert lib.gbrl_hip_step_prepared(None, None, G.ctypes.data, 0, None, 0, 16) == E_INVALID and b"null model" in err()
    assert not out.any() and info.raw == bytes(64)
    assert _file_bytes(m, tmp_path) == before
