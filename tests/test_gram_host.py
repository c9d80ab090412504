"""The tree Gram matrix without a device (gbrl_amd/csrc/gram_core.h): gbrl_cpp.tree_gram_host against a NumPy float64 evaluation over the leaves
the NumPy walk of tests/test_gpu_leaves.py reports, scale_trees, the launch plan against its rule, the symbols and the refusals that need no device.
tests/test_gpu_tree_gram.py imports np_gram and within_bound from here.

Bound (derived, include/gbrl_hip.h): products of float32 values are exact in float64, so only the additions round:
|got - want| <= (terms + 8) * 2^-53 * sum |v_t v_u| per entry, terms = rows * D, the right-hand sum computed in NumPy."""
import ctypes
import os

import numpy as np
import pytest

import gbrl_amd
from test_gpu_leaves import _np_leaves

cpp = gbrl_amd.gbrl_cpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def np_gram(e, policy, X, Y, a, b):
    """(gram, moment, |gram| sums, |moment| sums) in float64 from get_ensemble_data(); a leaf of -1 contributes zeros"""
    L = _np_leaves(e, policy, X, None, a, b)
    vals = np.asarray(e["values"], np.float64).reshape(np.asarray(e["values"]).shape[0], -1)
    V = vals[np.maximum(L, 0)] * (L >= 0)[:, :, None]
    gram, cap = np.einsum("ntd,nud->tu", V, V), np.einsum("ntd,nud->tu", np.abs(V), np.abs(V))
    if Y is None:
        return gram, None, cap, None
    Y = np.asarray(Y, np.float64).reshape(len(X), -1)
    return gram, np.einsum("ntd,nd->t", V, Y), cap, np.einsum("ntd,nd->t", np.abs(V), np.abs(Y))


def within_bound(got, want, cap, terms):
    return (np.abs(got - want) <= (terms + 8) * 2.0 ** -53 * cap).all()


def _loaded(name, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


@pytest.mark.parametrize("name,policy", [("obl_l2_q", "oblivious"), ("explain_obl_l2_q_d6", "oblivious"), ("grd_cos_q_ac", "greedy")])
@pytest.mark.parametrize("n", [1, 97])
def test_host_rule_against_numpy(name, policy, n, tmp_path):
    m = _loaded(name, tmp_path)
    md, T, e = m.get_metadata(), m.get_num_trees(), m.get_ensemble_data()
    D = md["output_dim"]
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, md["input_dim"])).astype(f32)
    Y = rng.standard_normal((n, D)).astype(f32)
    for a, b, y in ((0, 0, Y), (T // 2, T, None)):
        r = cpp.tree_gram_host(m, X, y if y is None or D > 1 else y[:, 0].copy(), a, b)
        want, wm, cap, capm = np_gram(e, policy, X, y, a, b if b else T)
        assert r["gram"].dtype == np.float64 and r["gram"].shape == want.shape and r["rows"] == n and r["route"] == "host"
        assert within_bound(r["gram"], want, cap, n * D) and np.array_equal(r["gram"], r["gram"].T)
        assert (r["moment"] is None) if y is None else within_bound(r["moment"], wm, capm, n * D)


def test_scale_trees_values_and_predict(tmp_path):
    m = _loaded("obl_l2_q", tmp_path)
    T, md = m.get_num_trees(), m.get_metadata()
    X = np.random.default_rng(3).standard_normal((33, md["input_dim"])).astype(f32)
    before, ti = np.asarray(m.get_ensemble_data()["values"]).copy(), np.asarray(m.get_ensemble_data()["tree_indices"])
    p_before = np.asarray(cpp.tree_gram_host(m, X)["gram"])
    w = np.array([0.5, 0.0, -2.0], f32)
    s0 = T - 3
    m.scale_trees(w, start_tree_idx=s0)
    after = np.asarray(m.get_ensemble_data()["values"])
    want = before.copy()
    for k in range(3):
        lo, hi = ti[s0 + k], ti[s0 + k + 1] if s0 + k + 1 < T else len(before)
        want[lo:hi] = (before[lo:hi] * w[k]).astype(f32)
    assert after.tobytes() == want.tobytes() and m.get_num_trees() == T
    wt = np.ones(T)
    wt[s0:] = w.astype(np.float64)   # (0.5, 0 and -2 scale a float32 exactly: the Gram scales entry by entry)
    assert np.allclose(cpp.tree_gram_host(m, X)["gram"], p_before * np.outer(wt, wt), rtol=1e-12, atol=0)
    for bad, text in ((np.array([np.nan], f32), "not finite"), (np.array([np.inf], f32), "not finite"), (np.ones(T + 1, f32), "outside the model"),
                      (np.ones((2, 2), f32), "one-dimensional")):
        with pytest.raises(RuntimeError, match=text):
            m.scale_trees(bad)
    with pytest.raises(RuntimeError, match="outside the model"):
        m.scale_trees(np.ones(2, f32), start_tree_idx=T - 1)
    assert np.asarray(m.get_ensemble_data()["values"]).tobytes() == want.tobytes()


# (rows, trees, groups): one chunk; two chunks (three pairs, two operands); the tree cap, where the budget cuts the row blocks; a width beyond the LDS
@pytest.mark.parametrize("n,T,G", [(1, 1, 1), (65, 64, 8), (1 << 20, 65, 8), (1 << 20, 2048, 8), (4096, 15, 69), (4096, 15, 70), (4096, 130, 61)])
def test_launch_plan(n, T, G):
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_tree_gram_geometry.restype = None
    lib.gbrl_hip_tree_gram_geometry.argtypes = [ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
    ci = [ctypes.c_int(-1) for _ in range(4)]
    cu = [ctypes.c_uint64(0) for _ in range(2)]
    lib.gbrl_hip_tree_gram_geometry(n, T, 3, G, ctypes.byref(ci[0]), ctypes.byref(ci[1]), ctypes.byref(ci[2]), ctypes.byref(cu[0]), ctypes.byref(cu[1]), ctypes.byref(ci[3]))
    g = cpp.tree_gram_geometry(n, T, 3, G)
    assert g == {"chunk": ci[0].value, "pairs": ci[1].value, "row_blocks": ci[2].value, "scratch_bytes": cu[0].value, "lds_bytes": cu[1].value, "streaming": bool(ci[3].value)}
    chunks = -(-T // 64)
    per_block = 8 * (chunks * (chunks + 1) // 2 * 4096 + chunks * 64)
    assert g["chunk"] == 64 and g["pairs"] == chunks * (chunks + 1) // 2
    assert g["row_blocks"] == max(1, min(-(-n // 64), 512, (64 << 20) // per_block)) and g["scratch_bytes"] == g["row_blocks"] * per_block <= 64 << 20
    assert g["lds_bytes"] == 64 * ((8 * G) | 1) * 4 + (2 if chunks > 1 else 1) * 64 * 65 * 8 + 64 * 8 and g["streaming"] == (g["lds_bytes"] <= 156 * 1024)
    assert g == cpp.tree_gram_geometry(n, T, 128, G)   # (D changes the time, not the geometry)


def test_symbols_and_refusals_without_a_device(tmp_path):
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    for sym in ("gbrl_hip_tree_gram_prepared", "gbrl_hip_tree_gram_host", "gbrl_hip_tree_gram_geometry", "gbrl_hip_scale_trees"):
        assert hasattr(lib, sym)
    for name in ("tree_gram_prepared", "scale_trees"):
        assert callable(getattr(gbrl_amd.GBRL, name))
    m = _loaded("obl_l2_q", tmp_path)
    md, T = m.get_metadata(), m.get_num_trees()
    F, D = md["input_dim"], md["output_dim"]
    X = np.random.default_rng(5).standard_normal((9, F)).astype(f32)
    nan_y = np.full((9, D), np.nan, f32)
    for args, text in (((X, None, 3, 3), "invalid tree range"), ((X, None, 0, T + 1), "invalid tree range"), ((X, np.zeros((8, D), f32)), "targets"),
                       ((X[:, :-1].copy(),), "Total number of features"), ((X, nan_y if D > 1 else nan_y[:, 0].copy()), "targets hold a NaN")):
        with pytest.raises(RuntimeError, match=text):
            cpp.tree_gram_host(m, *args)
    with pytest.raises(RuntimeError, match="null data set"):
        m.tree_gram_prepared(None)
    cat = _loaded("obl_l2_q_cat", tmp_path)
    with pytest.raises(RuntimeError, match="categorical columns"):
        cat.tree_gram_prepared(None)
    empty = gbrl_amd.GBRL(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    with pytest.raises(RuntimeError, match="no trees"):
        cpp.tree_gram_host(empty, np.zeros((5, 4), f32))
    for _ in range(2):   # twice: every non-zero leaf value of tree 0 overflows
        m.scale_trees(np.array([3e38], f32))
    with pytest.raises(RuntimeError, match="leaf value of the range is not finite"):
        cpp.tree_gram_host(m, X)


def test_more_than_128_outputs_and_a_row_sharded_model_are_unsupported(tmp_path):
    """check_gram_size on a model with trees and 257 outputs, and the communicator refusal every call on a data set shares; both GBRL_HIP_E_UNSUPPORTED, no device."""
    from shap_edges import fixture, load_model
    wide = load_model("host_d4_D257_obl", tmp_path)
    X = np.ascontiguousarray(fixture("host_d4_D257_obl")[2][:8])
    assert wide.get_metadata()["output_dim"] > 128 and wide.get_num_trees() >= 1
    with pytest.raises(RuntimeError, match="tree_gram_host: output_dim > 128"):
        cpp.tree_gram_host(wide, X)
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gbrl_hip_tree_gram_host.argtypes = [vp, vp, ci, ci, vp, ci, ci, vp, vp]
    T = wide.get_num_trees()
    gram = np.full((T, T), -7.0)
    assert lib.gbrl_hip_tree_gram_host(wide._handle(), X.ctypes.data, 8, X.shape[1], None, 0, 0, gram.ctypes.data, None) == -5
    assert b"output_dim > 128" in lib.gbrl_hip_last_error() and (gram == -7.0).all()

    reduce_t = ctypes.CFUNCTYPE(ci, vp, vp, ctypes.c_size_t)

    class Collective(ctypes.Structure):
        _fields_ = [("ctx", vp), ("world_size", ci), ("rank", ci)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    m = _loaded("obl_l2_q", tmp_path)
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    lib.gbrl_hip_set_collective.argtypes = [vp, vp]
    assert lib.gbrl_hip_set_collective(m._handle(), ctypes.byref(coll)) == 0, lib.gbrl_hip_last_error()
    try:
        with pytest.raises(RuntimeError, match="tree_gram_prepared: not available on a model with a communicator.*row-sharded"):
            m.tree_gram_prepared(None)
        lib.gbrl_hip_tree_gram_prepared.argtypes = [vp, vp, vp, ci, ci, vp, ci, ci, ci, vp, vp, vp]
        assert lib.gbrl_hip_tree_gram_prepared(m._handle(), None, None, 0, 8, None, 0, 0, 0, gram.ctypes.data, None, None) == -5
        assert b"row-sharded" in lib.gbrl_hip_last_error() and (gram == -7.0).all()
    finally:
        assert lib.gbrl_hip_set_collective(m._handle(), None) == 0
