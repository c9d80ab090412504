"""SHAP values on a prepared data set, the parts that need no GPU (include/gbrl_hip.h, "SHAP values on a data set"; gbrl_amd/csrc/shap_core.h):
  * gbrl_cpp.shap_sums_host against a NumPy loop that adds sequentially -- np.cumsum(...)[-1] per tile of 64 rows and over the tiles, never np.sum
    (which adds pairwise) -- on row counts around the tile, with signed zeros, and with a NaN row: a NaN propagates into the two totals of the columns
    it sits in and into no other column;
  * gbrl_hip_shap_geometry against the budget rule, restated by hand;
  * tests/cxx/shap_core_check.cpp, the same rules and the chunk plans, built with the address and undefined-behaviour sanitizers;
  * the C symbols, the Python signatures, and the refusals that need no data set.
The calls on a data set run in tests/test_gpu_shap_prepared.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
TILE, BUDGET = 64, 64 << 20


def _seq(x):
    """the sequential float64 sum of a vector from 0.0 (cumsum adds one element after the other)"""
    return np.cumsum(np.concatenate([[0.0], x.astype(np.float64)]))[-1]


def _numpy_rule(phi):
    m = phi.shape[0]
    flat = phi.reshape(m, -1)
    out = np.empty((2, flat.shape[1]), np.float64)
    for c in range(flat.shape[1]):
        col = flat[:, c]
        for k, v in enumerate((col, np.abs(col))):
            out[k, c] = _seq(np.array([_seq(v[p:p + TILE]) for p in range(0, m, TILE)]))
    return out[0].reshape(phi.shape[1:]), out[1].reshape(phi.shape[1:])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 257, 4097])
def test_sums_host_is_the_sequential_tile_rule(m):
    rng = np.random.default_rng(m)
    F, D = (5, 3) if m < 4097 else (2, 2)
    # magnitudes far apart, so that another order of the additions gives other bytes; zeros of both signs among them
    phi = (rng.uniform(-1, 1, (m, F, D)) * 2.0 ** rng.integers(-20, 21, (m, F, D))).astype(np.float32)
    phi[rng.random((m, F, D)) < 0.1] = 0.0
    phi[rng.random((m, F, D)) < 0.1] = -0.0
    s, a = cpp.shap_sums_host(phi)
    ws, wa = _numpy_rule(phi)
    assert s.dtype == np.float64 and s.shape == (F, D) and _same(s, ws) and _same(a, wa)
    s2, a2 = cpp.shap_sums_host(phi.reshape(m, F * D))          # [m, C] is the same rule
    assert s2.shape == (F * D,) and _same(s2, ws.reshape(-1)) and _same(a2, wa.reshape(-1))
    if m >= 129:                                                # the order matters at these magnitudes: a pairwise sum is another number somewhere
        assert not _same(s, phi.astype(np.float64).sum(axis=0)) or not _same(a, np.abs(phi).astype(np.float64).sum(axis=0))


def test_signed_zeros_and_a_nan_row():
    m, F, D = 70, 3, 2
    phi = np.full((m, F, D), -0.0, np.float32)
    phi[:, 2, :] = 1.0
    s, a = cpp.shap_sums_host(phi)
    assert _same(s[:2], np.zeros((2, D))) and _same(a[:2], np.zeros((2, D)))        # +0.0: the sums start from +0.0, and fabs(-0.0) = +0.0
    assert (s[2] == 70.0).all() and (a[2] == 70.0).all()
    # a NaN row: documented propagation -- the columns it sits in become NaN in both totals, every other column keeps its bytes
    phi[5, 1, 0] = np.nan
    phi[65, 2, 1] = -np.inf
    s2, a2 = cpp.shap_sums_host(phi)
    assert np.isnan(s2[1, 0]) and np.isnan(a2[1, 0])
    assert s2[2, 1] == -np.inf and a2[2, 1] == np.inf
    keep = np.ones((F, D), bool)
    keep[1, 0] = keep[2, 1] = False
    assert _same(s2[keep], s[keep]) and _same(a2[keep], a[keep])
    ws, wa = _numpy_rule(phi)
    assert _same(s2, ws) and _same(a2, wa)


def test_sums_host_refusals():
    with pytest.raises(RuntimeError, match=r"\[m, F, D\] or \[m, C\]"):
        cpp.shap_sums_host(np.zeros(4, np.float32))
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_shap_sums_host.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    phi, s, a = np.ones((3, 2), np.float32), np.zeros(2), np.zeros(2)
    assert lib.gbrl_hip_shap_sums_host(phi.ctypes.data, 3, 2, s.ctypes.data, a.ctypes.data) == 0 and s.tolist() == [3.0, 3.0] and a.tolist() == [3.0, 3.0]
    for args in ((None, 3, 2, s.ctypes.data, a.ctypes.data), (phi.ctypes.data, 3, 2, None, a.ctypes.data), (phi.ctypes.data, 3, 2, s.ctypes.data, None),
                 (phi.ctypes.data, -1, 2, s.ctypes.data, a.ctypes.data)):
        assert lib.gbrl_hip_shap_sums_host(*args) == E_INVALID, args


def test_geometry_is_the_budget_rule():
    assert cpp.shap_geometry() == {"tile_rows": TILE, "default_chunk_rows": BUDGET // 4, "scratch_budget": BUDGET}
    assert BUDGET == cpp.partial_dependence_geometry()["scratch_budget"]          # partial dependence's budget
    for F in (1, 3, 16, 17, 40, 128, 1000, 4096, 100000):
        for D in (1, 3, 8, 64, 65, 128):
            rows = cpp.shap_geometry(F, D)["default_chunk_rows"]
            want = max(TILE, BUDGET // (4 * F * D) // TILE * TILE)                # the largest multiple of 64 inside the budget, and at least 64
            assert rows == want, (F, D, rows, want)
            assert rows % TILE == 0 and (rows == TILE or rows * 4 * F * D <= BUDGET) and (rows + TILE) * 4 * F * D > BUDGET
    assert cpp.shap_geometry(128, 8)["default_chunk_rows"] == 16384
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_shap_geometry.restype = None
    lib.gbrl_hip_shap_geometry.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    tile, rows, budget = C.c_int(), C.c_int(), C.c_uint64()
    lib.gbrl_hip_shap_geometry(17, 3, C.byref(tile), C.byref(rows), C.byref(budget))
    assert (tile.value, rows.value, budget.value) == (TILE, BUDGET // (4 * 17 * 3) // TILE * TILE, BUDGET)
    lib.gbrl_hip_shap_geometry(17, 3, None, None, None)


def test_shap_core_check_runs_clean_under_the_sanitizers(tmp_path):
    """shap_core.h without a device (tests/cxx/shap_core_check.cpp, built with the address and undefined-behaviour sanitizers): the reduction rule
    against a plain loop on random matrices up to F * D = 128 * 128, its independence of the chunking, the chunk plans at m in {1, 63, 64, 65, 4097},
    and the argument checks."""
    exe = tmp_path / "shap_core_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gbrl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "shap_core_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "all sections passed" in out.stdout, out.stdout + out.stderr
    assert len(out.stdout.strip().split("\n")) == 5, out.stdout


def _empty(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def test_symbols_and_signatures():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for sym in ("gbrl_hip_shap_prepared", "gbrl_hip_shap_importance_prepared", "gbrl_hip_shap_sums_host", "gbrl_hip_shap_geometry"):
        assert hasattr(lib, sym), sym
    m = _empty()
    sig = m.shap_prepared.__doc__.splitlines()[0]
    assert sig.startswith("shap_prepared(self: gbrl_cpp.GBRL, ds: object, norm_values: object, base_poly: object, offset: object, rows: object = None, tree_idx: object = None)")
    sig = m.shap_importance_prepared.__doc__.splitlines()[0]
    assert sig.startswith("shap_importance_prepared(self: gbrl_cpp.GBRL, ds: object, norm_values: object, base_poly: object, offset: object, rows: object = None, "
                          "chunk_rows: object = None) -> dict")
    header = open(os.path.join(ROOT, "include", "gbrl_hip.h")).read()
    for sym in ("gbrl_hip_shap_prepared(", "gbrl_hip_shap_importance_prepared(", "gbrl_hip_shap_sums_host(", "gbrl_hip_shap_geometry("):
        assert header.count("int " + sym) + header.count("void " + sym) == 1, sym


def _loaded(name, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


def test_what_is_refused_about_the_model_comes_first(tmp_path):
    """A model with categorical columns and a row-sharded model are refused before the data set is looked at (the data-set calls' shared refusal),
    with GBRL_HIP_E_UNSUPPORTED; the model's file bytes stay as they were."""
    poly = [np.zeros((2, 1), np.float32), np.zeros(1, np.float32), np.zeros((1, 1), np.float32)]
    m = _loaded("obl_l2_q_cat", tmp_path)
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    before = p.read_bytes()
    for call in (m.shap_prepared, m.shap_importance_prepared):
        with pytest.raises(RuntimeError, match="not available on a model with categorical columns"):
            call(None, *poly)
    reduce_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)

    class Collective(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    s = _loaded("obl_l2_q", tmp_path)
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    lib.gbrl_hip_set_collective.argtypes = [C.c_void_p, C.c_void_p]
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_shap_prepared.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci]
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    assert lib.gbrl_hip_set_collective(s._handle(), C.byref(coll)) == 0, lib.gbrl_hip_last_error()
    try:
        for call in (s.shap_prepared, s.shap_importance_prepared):
            with pytest.raises(RuntimeError, match="collective hooks"):
                call(None, *poly)
        assert lib.gbrl_hip_shap_prepared(s._handle(), None, None, 0, 8, -1, None, None, None, None, 0) == -5 and b"collective hooks" in lib.gbrl_hip_last_error()
    finally:
        assert lib.gbrl_hip_set_collective(s._handle(), None) == 0
    assert m.save(str(p)) == 0 and p.read_bytes() == before


def test_refusals_that_need_no_data_set():
    m = _empty()
    poly = [np.zeros((4, 3), np.float32), np.zeros(3, np.float32), np.zeros((3, 3), np.float32)]
    for call in (m.shap_prepared, m.shap_importance_prepared):
        with pytest.raises(RuntimeError, match="null data set"):
            call(None, *poly)
        with pytest.raises((RuntimeError, TypeError)):
            call(object(), *poly)
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_shap_prepared.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci]
    lib.gbrl_hip_shap_importance_prepared.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp]
    nv, bp, of = (p.ctypes.data for p in poly)
    out, s, a, stale = np.zeros((16, 4, 2), np.float32), np.zeros((4, 2)), np.zeros((4, 2)), C.c_int(0)
    h, err = m._handle(), lib.gbrl_hip_last_error
    for ds, what in ((None, b"null data set"), (C.addressof(stale), b"destroyed")):
        assert lib.gbrl_hip_shap_prepared(h, ds, None, 0, 16, -1, nv, bp, of, out.ctypes.data, 0) == E_INVALID and what in err()
        assert lib.gbrl_hip_shap_importance_prepared(h, ds, None, 0, 16, nv, bp, of, 0, s.ctypes.data, a.ctypes.data, None) == E_INVALID and what in err()
    assert lib.gbrl_hip_shap_prepared(None, None, None, 0, 16, -1, nv, bp, of, out.ctypes.data, 0) == E_INVALID and b"null model" in err()
    assert lib.gbrl_hip_shap_importance_prepared(None, None, None, 0, 16, nv, bp, of, 0, s.ctypes.data, a.ctypes.data, None) == E_INVALID and b"null model" in err()
