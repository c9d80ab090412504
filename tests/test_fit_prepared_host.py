"""CPU-side checks of the walk over a prepared data set's bin codes (include/gbrl_hip.h: gbrl_hip_condition_bins,
gbrl_hip_predict_continue_prepared, gbrl_hip_fit_prepared; Python: GBRL.condition_bins, GBRL.predict_continue_prepared, GBRL.fit_prepared).
condition_bins is host code and is checked in full here against its NumPy definition; of the two device calls, everything that is refused without
a data set in hand -- through the binding and through the C ABI with the documented status, the model's file bytes unchanged afterwards.  The
models with trees come from the reference's files in tests/golden.  The calls themselves run in tests/test_gpu_fit_prepared.py."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd
from helpers import load_golden

E_INVALID, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -5
C_SYMBOLS = ("gbrl_hip_condition_bins", "gbrl_hip_predict_continue_prepared", "gbrl_hip_fit_prepared")
GOLDEN_MODELS = ("obl_l2_q", "grd_cos_q_ac")   # oblivious and greedy, numeric columns only


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
    lib.gbrl_hip_condition_bins.argtypes = [vp, vp, ci, ci, vp]
    lib.gbrl_hip_predict_continue_prepared.argtypes = [vp, vp, vp, ci, ci, vp, ci, ci, ci, vp]
    lib.gbrl_hip_fit_prepared.argtypes = [vp, vp, vp, ci, ci, vp]
    lib.gbrl_hip_set_collective.argtypes = [vp, vp]
    return lib


def _table(m, rng, drop=None):
    """A threshold table [F, n_bins] that holds every value the model's numeric conditions use for a feature (but `drop` = (f, v)), padded with
    other values and with duplicates, in shuffled order; and the used slots (split row, level, feature, value)."""
    e, md = m.get_ensemble_data(), m.get_metadata()
    F, B = md["input_dim"], md["n_bins"]   # (numeric columns only)
    depths, fi, fv, isn = (np.asarray(e[k]) for k in ("depths", "feature_indices", "feature_values", "is_numerics"))
    used = [(s, d, int(fi[s, d]), fv[s, d]) for s in range(fi.shape[0]) for d in range(int(depths[s])) if isn[s, d]]
    thr = np.empty((F, B), np.float32)
    for f in range(F):
        vals = sorted({np.float32(v) for (_, _, ff, v) in used if ff == f and (drop is None or (ff, v) != drop)})
        assert len(vals) < B, "the fixture uses more distinct thresholds than n_bins holds"
        pad = rng.uniform(-3, 3, B - len(vals)).astype(np.float32)
        pad = np.array([p for p in pad if drop is None or drop[0] != f or p != drop[1]] + [np.float32(7.5)] * B, np.float32)[:B - len(vals)]
        if vals and len(pad) > 1:
            pad[0] = vals[0]                       # a duplicate of a used value
            pad[-1] = pad[len(pad) // 2]           # and of a padding value
        row = np.concatenate([np.array(vals, np.float32), pad])
        thr[f] = rng.permutation(row)
    return thr, used


def test_symbols_names_and_abi_version():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for sym in C_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.gbrl_hip_abi_version.restype = C.c_int
    assert lib.gbrl_hip_abi_version() == 1
    m = _empty()
    assert m.condition_bins.__doc__.splitlines()[0].startswith("condition_bins(self: gbrl_cpp.GBRL, thresholds: object)")
    assert "ds: object, base: object, start_tree_idx: object = 0, stop_tree_idx: object = 0, rows: object = None)" in \
        m.predict_continue_prepared.__doc__.splitlines()[0]
    sig = m.fit_prepared.__doc__.splitlines()[0]   # (how pybind11 spells the int depends on its version)
    assert sig.startswith("fit_prepared(self: gbrl_cpp.GBRL, ds: object, targets: object, iterations: ") and sig.endswith("-> float")


@pytest.mark.parametrize("name", GOLDEN_MODELS)
def test_condition_bins_is_the_count_of_thresholds_below_the_value(name, tmp_path):
    m, _, _ = _loaded(name, tmp_path)
    before = _file_bytes(m, tmp_path)
    rng = np.random.default_rng(5)
    thr, used = _table(m, rng)
    assert used, "the fixture has no numeric condition"
    bins = m.condition_bins(thr)
    fv = np.asarray(m.get_ensemble_data()["feature_values"])
    assert bins.dtype == np.int32 and bins.shape == fv.shape
    want = np.full(fv.shape, -1, np.int32)
    for s, d, f, v in used:
        want[s, d] = int((thr[f] < v).sum())
    assert np.array_equal(bins, want)
    assert (want >= 0).sum() == len(used) and (want == -1).sum() == want.size - len(used)
    # the C ABI writes the same table
    lib = _lib()
    out = np.full(fv.size, 99, np.int32)
    assert lib.gbrl_hip_condition_bins(m._handle(), thr.ctypes.data, thr.shape[0], thr.shape[1], out.ctypes.data) == 0, lib.gbrl_hip_last_error()
    assert np.array_equal(out.reshape(fv.shape), want)
    assert _file_bytes(m, tmp_path) == before


@pytest.mark.parametrize("name", GOLDEN_MODELS)
def test_a_value_outside_the_thresholds_is_unsupported_and_names_the_tree(name, tmp_path):
    m, _, _ = _loaded(name, tmp_path)
    e = m.get_ensemble_data()
    rng = np.random.default_rng(6)
    _, used = _table(m, rng)
    s, d, f, v = used[len(used) // 2]
    oblivious = m.get_metadata()["grow_policy"] == "Oblivious"
    # the first split row (in storage order) that uses (f, v) is the one reported
    s0, d0 = min((ss, dd) for (ss, dd, ff, vv) in used if ff == f and vv == v)
    tree = s0 if oblivious else int(np.searchsorted(np.asarray(e["tree_indices"]), s0, side="right")) - 1
    thr, _ = _table(m, rng, drop=(f, v))
    assert not (thr[f] == v).any()
    lib = _lib()
    out = np.zeros(np.asarray(e["feature_values"]).size, np.int32)
    with pytest.raises(RuntimeError, match=r"tree %d, condition %d \(feature %d" % (tree, d0, f)):
        m.condition_bins(thr)
    assert lib.gbrl_hip_condition_bins(m._handle(), thr.ctypes.data, thr.shape[0], thr.shape[1], out.ctypes.data) == E_UNSUPPORTED
    assert b"tree %d," % tree in lib.gbrl_hip_last_error()
    # a NaN where the value was: NaN equals nothing
    full, _ = _table(m, rng)
    full[f][full[f] == v] = np.nan
    with pytest.raises(RuntimeError, match="tree %d," % tree):
        m.condition_bins(full)
    assert lib.gbrl_hip_condition_bins(m._handle(), full.ctypes.data, full.shape[0], full.shape[1], out.ctypes.data) == E_UNSUPPORTED


def test_condition_bins_shape_errors(tmp_path):
    m, _, _ = _loaded("obl_l2_q", tmp_path)
    thr, _ = _table(m, np.random.default_rng(7))
    F, B = thr.shape
    lib = _lib()
    out = np.zeros(np.asarray(m.get_ensemble_data()["feature_values"]).size, np.int32)
    for bad in (np.zeros((F + 1, B), np.float32), np.zeros((F, B - 1), np.float32)):
        with pytest.raises(RuntimeError, match="condition_bins"):
            m.condition_bins(bad)
        assert lib.gbrl_hip_condition_bins(m._handle(), bad.ctypes.data, bad.shape[0], bad.shape[1], out.ctypes.data) == E_INVALID
    with pytest.raises(RuntimeError, match="shape"):
        m.condition_bins(np.zeros(F * B, np.float32))
    assert lib.gbrl_hip_condition_bins(m._handle(), None, F, B, out.ctypes.data) == E_INVALID
    assert lib.gbrl_hip_condition_bins(None, thr.ctypes.data, F, B, out.ctypes.data) == E_INVALID and b"null model" in lib.gbrl_hip_last_error()
    # a model without trees has nothing to convert
    assert _empty().condition_bins(np.zeros((4, 256), np.float32)).shape == (0, 3)


@pytest.mark.parametrize("name", GOLDEN_MODELS)
def test_argument_errors_without_a_data_set(name, tmp_path):
    m, _, _ = _loaded(name, tmp_path)
    D = np.asarray(m.get_bias()).size
    y = np.zeros((16, D), np.float32)
    base = np.zeros((16, D), np.float32)
    before = _file_bytes(m, tmp_path)
    lib = _lib()
    err = lib.gbrl_hip_last_error
    h = m._handle()
    # null data set
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, y, 3)
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(ds=None, targets=y, iterations=3)
    with pytest.raises(RuntimeError, match="null data set"):
        m.predict_continue_prepared(None, base, 0, 0)
    with pytest.raises(RuntimeError, match="null data set"):
        m.predict_continue_prepared(ds=None, base=base, start_tree_idx=0, stop_tree_idx=0, rows=np.arange(16, dtype=np.int32))
    with pytest.raises((RuntimeError, TypeError)):
        m.fit_prepared(object(), y, 3)
    loss = C.c_float(-1.0)
    stale = C.create_string_buffer(64)
    for ds, what in ((None, b"null data set"), (C.addressof(stale), b"destroyed")):
        assert lib.gbrl_hip_fit_prepared(h, ds, y.ctypes.data, 0, 3, C.byref(loss)) == E_INVALID and what in err()
        assert lib.gbrl_hip_predict_continue_prepared(h, ds, None, 0, 16, base.ctypes.data, 0, 0, 0, base.ctypes.data) == E_INVALID and what in err()
    # iterations < 0, missing targets: refused whatever the data set is
    with pytest.raises(RuntimeError, match="iterations must be >= 0"):
        m.fit_prepared(None, y, -1)
    assert lib.gbrl_hip_fit_prepared(h, None, y.ctypes.data, 0, -1, C.byref(loss)) == E_INVALID and b"iterations must be >= 0" in err()
    with pytest.raises(RuntimeError, match="without targets"):
        m.fit_prepared(None, None, 3)
    assert lib.gbrl_hip_fit_prepared(h, None, None, 0, 3, C.byref(loss)) == E_INVALID and b"without targets" in err()
    assert lib.gbrl_hip_fit_prepared(None, None, y.ctypes.data, 0, 3, C.byref(loss)) == E_INVALID and b"null model" in err()
    assert lib.gbrl_hip_predict_continue_prepared(None, None, None, 0, 16, base.ctypes.data, 0, 0, 0, base.ctypes.data) == E_INVALID and b"null model" in err()
    assert loss.value == -1.0 and not base.any()
    assert _file_bytes(m, tmp_path) == before


def test_a_categorical_model_is_unsupported(tmp_path):
    m, X, Xc = _loaded("obl_l2_q_cat", tmp_path)
    D = np.asarray(m.get_bias()).size
    y = np.zeros((16, D), np.float32)
    before = _file_bytes(m, tmp_path)
    lib = _lib()
    with pytest.raises(RuntimeError, match="categorical columns"):
        m.fit_prepared(None, y, 2)
    with pytest.raises(RuntimeError, match="categorical columns"):
        m.predict_continue_prepared(None, y, 0, 0)
    loss = C.c_float(0.0)
    assert lib.gbrl_hip_fit_prepared(m._handle(), None, y.ctypes.data, 0, 2, C.byref(loss)) == E_UNSUPPORTED and b"categorical columns" in lib.gbrl_hip_last_error()
    assert lib.gbrl_hip_predict_continue_prepared(m._handle(), None, None, 0, 16, y.ctypes.data, 0, 0, 0, y.ctypes.data) == E_UNSUPPORTED
    assert b"categorical columns" in lib.gbrl_hip_last_error()
    assert _file_bytes(m, tmp_path) == before


def test_a_row_sharded_model_is_unsupported(tmp_path):
    reduce_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)

    class Collective(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    m, _, _ = _loaded("obl_l2_q", tmp_path)
    D = np.asarray(m.get_bias()).size
    y = np.zeros((8, D), np.float32)
    lib = _lib()
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    before = _file_bytes(m, tmp_path)
    assert lib.gbrl_hip_set_collective(m._handle(), C.byref(coll)) == 0, lib.gbrl_hip_last_error()
    try:
        loss = C.c_float(0.0)
        assert lib.gbrl_hip_fit_prepared(m._handle(), None, y.ctypes.data, 0, 2, C.byref(loss)) == E_UNSUPPORTED and b"collective hooks" in lib.gbrl_hip_last_error()
        assert lib.gbrl_hip_predict_continue_prepared(m._handle(), None, None, 0, 8, y.ctypes.data, 0, 0, 0, y.ctypes.data) == E_UNSUPPORTED
        with pytest.raises(RuntimeError, match="collective hooks"):
            m.fit_prepared(None, y, 2)
        with pytest.raises(RuntimeError, match="collective hooks"):
            m.predict_continue_prepared(None, y, 0, 0)
    finally:
        assert lib.gbrl_hip_set_collective(m._handle(), None) == 0
    assert _file_bytes(m, tmp_path) == before


def test_without_a_device_the_first_legal_call_reports_it(tmp_path):
    """A data set is made on the device, so without one the legal sequence ends at prepare_dataset; condition_bins needs none.
    (With a GPU present the legal calls run in tests/test_gpu_fit_prepared.py.)"""
    if not gbrl_amd.cuda_available():
        m = _empty()
        before = _file_bytes(m, tmp_path)
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.fit_prepared(m.prepare_dataset(np.zeros((8, 4), np.float32)), np.zeros((8, 2), np.float32), 2)
        assert _file_bytes(m, tmp_path) == before
