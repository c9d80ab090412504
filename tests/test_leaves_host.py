"""CPU-side checks of `predict_leaves` / `leaf_counts` and their `_encoded` variants (include/gbrl_hip.h): the C symbols and the binding's
methods exist, the ABI version is unchanged, and every argument error of the contract is reported before a device is needed -- through the
binding and through the C ABI.  No GPU here, so the models with trees come from the reference's files in tests/golden."""
import ctypes

import numpy as np
import pytest

import gbrl_amd
from helpers import load_golden

NAMES = ("gbrl_hip_predict_leaves", "gbrl_hip_predict_leaves_encoded", "gbrl_hip_leaf_counts", "gbrl_hip_leaf_counts_encoded")


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
    return gbrl_amd.GBRL.load(str(p)), case, X, Xc


def _lib():
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    vp, ci, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    lib.gbrl_hip_predict_leaves.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, ci]
    lib.gbrl_hip_predict_leaves_encoded.argtypes = [vp, vp, ci, vp, ci, u64, ci, ci, ci, ci, ci, vp, ci]
    lib.gbrl_hip_leaf_counts.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.gbrl_hip_leaf_counts_encoded.argtypes = [vp, vp, ci, vp, ci, u64, ci, ci, ci, ci, ci, vp]
    return lib


def test_symbols_methods_and_abi_version():
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
    lib.gbrl_hip_abi_version.restype = ctypes.c_int
    assert lib.gbrl_hip_abi_version() == 1
    m = _empty()
    for meth in ("predict_leaves", "predict_leaves_encoded", "leaf_counts", "leaf_counts_encoded"):
        assert callable(getattr(m, meth)), meth
    # keyword names as documented
    plain = "obs: object, categorical_obs: object, start_tree_idx: object = 0, stop_tree_idx: object = 0"
    assert plain in m.predict_leaves.__doc__ and plain in m.leaf_counts.__doc__
    for doc in (m.predict_leaves_encoded.__doc__, m.leaf_counts_encoded.__doc__):
        assert "obs: object, categorical_ids: object, dictionary_token: " in doc
        assert "start_tree_idx: object = 0, stop_tree_idx: object = 0" in doc
    # the chunk of leaf counters one launch keeps on chip is readable without a device, and the binding and the library agree
    lib.gbrl_hip_leaf_counts_chunk.restype = ctypes.c_int
    assert gbrl_amd.GBRL.leaf_counts_chunk() == lib.gbrl_hip_leaf_counts_chunk() > 0


def test_a_model_without_trees_is_refused():
    m = _empty()
    X = np.zeros((8, 4), np.float32)
    for call in (m.predict_leaves, m.leaf_counts):
        with pytest.raises(RuntimeError, match="has no trees"):
            call(X, None)
        with pytest.raises(RuntimeError, match="has no trees"):
            call(X, None, 0, 1)


@pytest.mark.parametrize("name", ["obl_l2_q", "grd_cos_q_ac"])
def test_binding_argument_errors(name, tmp_path):
    m, case, X, _ = _loaded(name, tmp_path)
    T = m.get_num_trees()
    assert T >= 3
    X = np.ascontiguousarray(X[:16])
    for call in (m.predict_leaves, m.leaf_counts):
        # the range: stop == 0 means T; after that 0 <= start < stop <= T
        for a, b in ((0, T + 1), (2, 2), (2, 1), (T, 0), (T + 1, 0), (-1, 2), (0, -1)):
            with pytest.raises(RuntimeError, match="invalid tree range"):
                call(X, None, a, b)
        # the data set errors of predict
        with pytest.raises(RuntimeError, match="without observations"):
            call(None, None)
        with pytest.raises(RuntimeError, match="Total number of features"):
            call(np.zeros((16, X.shape[1] - 1), np.float32), None)
        with pytest.raises(RuntimeError, match="Expected array of format"):
            call(X.astype(np.float64), None)
        with pytest.raises(RuntimeError, match="Expected array of format"):
            call(X[:, :-1].copy(), np.zeros((16, 1)))                    # categorical cells must be S128
    # a legal call gets as far as the device: with no GPU that is the error, and no other
    if not gbrl_amd.cuda_available():
        for call in (m.predict_leaves, m.leaf_counts):
            with pytest.raises(RuntimeError, match="no HIP device"):
                call(X, None, 1, T)
            with pytest.raises(RuntimeError, match="no HIP device"):
                call(X, None)


def test_the_element_count_guard_is_for_predict_leaves_only(tmp_path):
    """n x T >= 2^31 indices: refused with the unsupported status before the device is touched.  Shapes only -- a (data_ptr, shape, dtype,
    device) tuple announces 2^30 rows (2 trees) or 715 827 883 rows (3 trees: 2^31 + 1 indices) without an array behind it; the call fails before anything reads it."""
    m, case, X, _ = _loaded("obl_l2_q", tmp_path)
    T, F = m.get_num_trees(), X.shape[1]
    assert T >= 3
    lib = _lib()
    for n, trees in ((715827883, 3), (1 << 30, 2), ((1 << 31) - 1, 2), ((1 << 31) - 1, 0)):
        assert n * (trees or T) >= 1 << 31
        fake = (4096, (n, F), "torch.float32", "cuda")
        with pytest.raises(RuntimeError, match="2\\^31"):
            m.predict_leaves(fake, None, 0, trees)
        out = ctypes.c_int32()
        rc = lib.gbrl_hip_predict_leaves(m._handle(), 4096, 1, None, 0, n, F, 0, 0, trees, ctypes.addressof(out), 1)
        assert rc == -5 and b"2^31" in lib.gbrl_hip_last_error()          # GBRL_HIP_E_UNSUPPORTED
    # one index below the limit passes the guard (and, without a GPU, stops at the device)
    if not gbrl_amd.cuda_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_leaves((4096, ((1 << 30) - 1, F), "torch.float32", "cuda"), None, 0, 2)
        # leaf_counts reduces on the device and has no such limit
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.leaf_counts((4096, (1 << 30, F), "torch.float32", "cuda"), None, 0, 2)


def test_a_stale_dictionary_token_is_refused_before_the_device(tmp_path):
    m, case, X, Xc = _loaded("obl_l2_q_cat", tmp_path)
    e = m.get_ensemble_data()
    assert (np.asarray(e["is_numerics"]) == 0).any(), "the fixture has no categorical condition"
    n = 16
    X = np.ascontiguousarray(X[:n]) if X is not None and X.shape[1] else None
    ids = np.zeros((n, Xc.shape[1]), np.int32)
    for call in (m.predict_leaves_encoded, m.leaf_counts_encoded):
        with pytest.raises(RuntimeError, match="another category dictionary"):
            call(X, ids, 12345)
        with pytest.raises(RuntimeError, match="another category dictionary"):
            call(X, ids, 0, 0, 1)
        with pytest.raises(RuntimeError, match="Expected array of format"):
            call(X, ids.astype(np.int64), 12345)
        with pytest.raises(RuntimeError, match="invalid tree range"):
            call(X, ids, 12345, 2, 1)                                     # the range is checked first


def test_c_abi_errors_before_the_device_is_touched(tmp_path):
    m, case, X, _ = _loaded("obl_l2_q", tmp_path)
    T, F = m.get_num_trees(), X.shape[1]
    lib = _lib()
    err = lib.gbrl_hip_last_error
    h = m._handle()
    X = np.ascontiguousarray(X[:8])
    out = np.zeros((8, T), np.int32)
    cnt = np.zeros(int(np.asarray(m.get_ensemble_data()["values"]).shape[0]), np.int64)

    def leaves(n, n_num, n_cat, a, b, op, handle=h):
        return lib.gbrl_hip_predict_leaves(handle, X.ctypes.data, 0, None, 0, n, n_num, n_cat, a, b, op, 0)

    def counts(n, n_num, n_cat, a, b, op, handle=h):
        return lib.gbrl_hip_leaf_counts(handle, X.ctypes.data, 0, None, 0, n, n_num, n_cat, a, b, op)

    for f, op in ((leaves, out.ctypes.data), (counts, cnt.ctypes.data)):
        assert f(8, F - 1, 0, 0, 0, op) == -1 and b"Incompatible dataset" in err()
        assert f(0, F, 0, 0, 0, op) == -1 and b"without observations" in err()
        assert f(8, F, 0, 0, 0, None) == -1 and b"without observations" in err()
        assert f(8, F - 1, 1, 0, 0, op) == -1 and b"Incompatible dataset" in err()
        for a, b in ((0, T + 1), (2, 2), (2, 1), (T, 0), (-1, 2), (0, -1)):
            assert f(8, F, 0, a, b, op) == -1 and b"invalid tree range" in err(), (a, b)
        assert f(8, F, 0, 0, 0, op, handle=None) == -1
        empty = _empty(input_dim=F)
        assert f(8, F, 0, 0, 0, op, handle=empty._handle()) == -1 and b"has no trees" in err()
    # the encoded entry points: no ids, a stale token
    mc, _, Xn, Xc = _loaded("obl_l2_q_cat", tmp_path)
    Fn, Fc = (Xn.shape[1] if Xn is not None else 0), Xc.shape[1]
    ids = np.zeros((8, Fc), np.int32)
    xp = np.ascontiguousarray(Xn[:8]).ctypes.data if Fn else None
    big = np.zeros((8, mc.get_num_trees()), np.int64)
    assert lib.gbrl_hip_predict_leaves_encoded(mc._handle(), xp, 0, None, 0, 7, 8, Fn, Fc, 0, 0, big.ctypes.data, 0) == -1 and b"without observations" in err()
    assert lib.gbrl_hip_predict_leaves_encoded(mc._handle(), xp, 0, ids.ctypes.data, 0, 7, 8, Fn, Fc, 0, 0, big.ctypes.data, 0) == -1 and b"another category dictionary" in err()
    assert lib.gbrl_hip_leaf_counts_encoded(mc._handle(), xp, 0, ids.ctypes.data, 0, 7, 8, Fn, Fc, 0, 0, big.ctypes.data) == -1 and b"another category dictionary" in err()


def test_no_output_width_limit(tmp_path):
    """predict refuses output_dim > 128 before the device; the leaf calls do not look at the width (a model without trees is their error here)."""
    wide = _empty(output_dim=300, policy_dim=300)
    X = np.zeros((8, 4), np.float32)
    with pytest.raises(RuntimeError, match="output_dim > 128"):
        wide.predict(X, None)
    with pytest.raises(RuntimeError, match="has no trees"):
        wide.predict_leaves(X, None)
    with pytest.raises(RuntimeError, match="has no trees"):
        wide.leaf_counts(X, None)
