"""Partial dependence, the parts that need no GPU (include/gbrl_hip.h, "Partial dependence"; gbrl_amd/csrc/pd_core.h):
  * GBRL.partial_dependence_codes on models LOADED from the reference's own files (tests/golden: oblivious and greedy, numeric columns only) against
    brute force -- for every code g in 0..B the vector (g > bin) over the walked conditions on the column, taken from get_ensemble_data() and
    condition_bins(); the breaks are exactly where that vector changes; an untested column gives [0]; a prefix of the trees never has more breaks;
  * tests/cxx/pd_core_check.cpp, the same rules on random tables, built with the address and undefined-behaviour sanitizers;
  * the launch plan of gbrl_cpp.partial_dependence_geometry: inside the budget, never below 1;
  * the hook table kept in step with INTEGRATION.md section 5, the C symbols, and the refusals that need no data set.
The calls on a data set run in tests/test_gpu_partial_dependence.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -5
# oblivious and greedy, numeric columns only: (file, later trees add breaks).  The first two repeat one tree; the sched_ models grow 14 and 16
# different ones; the stump model holds a one-leaf greedy tree, whose walk runs on into the next tree
GOLDEN_MODELS = (("obl_l2_q", False), ("grd_cos_q_ac", False), ("sched_obl_l2_q", True), ("sched_grd_cos_q_ac", True), ("shap_edge_t64_d12_D3_grd_stump", False))


def _loaded(name, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


def _empty(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def _table(m, rng):
    """A threshold table [F, n_bins] that holds every value the model's numeric conditions use for a feature, padded with other values and with
    duplicates, in shuffled order (test_fit_prepared_host.py's recipe)."""
    e, md = m.get_ensemble_data(), m.get_metadata()
    F, B = md["input_dim"], md["n_bins"]
    depths, fi, fv, isn = (np.asarray(e[k]) for k in ("depths", "feature_indices", "feature_values", "is_numerics"))
    thr = np.empty((F, B), np.float32)
    for f in range(F):
        vals = sorted({np.float32(fv[s, d]) for s in range(fi.shape[0]) for d in range(int(depths[s])) if isn[s, d] and int(fi[s, d]) == f})
        assert len(vals) < B
        pad = rng.uniform(-3, 3, B - len(vals)).astype(np.float32)
        if vals and len(pad) > 1:
            pad[0] = vals[0]
            pad[-1] = pad[len(pad) // 2]
        thr[f] = rng.permutation(np.concatenate([np.array(vals, np.float32), pad]))
    return thr


def _walked_bins(m, bins, col, n_trees):
    """the bins of the numeric conditions on `col` that the walk of the trees [0, n_trees) reads (greedy: through the trees a trailing run of one-leaf
    trees runs on into)"""
    e, md = m.get_ensemble_data(), m.get_metadata()
    depths, fi, isn, ti = (np.asarray(e[k]) for k in ("depths", "feature_indices", "is_numerics", "tree_indices"))
    T, L = len(ti), np.asarray(e["values"]).shape[0]
    if md["grow_policy"] == "Oblivious":
        rows = n_trees
    else:
        first = lambda t: int(ti[t]) if t < T else L
        end = n_trees
        while end < T and first(end) - first(end - 1) == 1:
            end += 1
        rows = first(end)
    return [int(bins[s, d]) for s in range(rows) for d in range(int(depths[s])) if isn[s, d] and int(fi[s, d]) == col]


def _brute_force(walked, B):
    answers = lambda g: [g > b for b in walked]
    return [0] + [g for g in range(1, B + 1) if answers(g) != answers(g - 1)]


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_partial_dependence_codes.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    lib.gbrl_hip_partial_dependence_prepared.argtypes = [vp, vp, vp, ci, vp, ci, ci, ci, vp, vp, ci]
    lib.gbrl_hip_partial_dependence_geometry.argtypes = [ci, ci, vp, vp, vp, vp]
    lib.gbrl_hip_partial_dependence_cells.argtypes = [ci, vp, ci, ci, vp, ci, vp]
    lib.gbrl_hip_partial_dependence_geometry.restype = None
    return lib


@pytest.mark.parametrize("name,grows", GOLDEN_MODELS)
def test_codes_are_the_brute_force_breaks(name, grows, tmp_path):
    m = _loaded(name, tmp_path)
    md, T = m.get_metadata(), m.get_num_trees()
    F, B = md["input_dim"], md["n_bins"]
    assert T >= 2
    thr = _table(m, np.random.default_rng(5))
    bins = np.asarray(m.condition_bins(thr))
    lib = _lib()
    untested, fewer = 0, 0
    for col in range(F):
        full = m.partial_dependence_codes(thr, col)
        assert full.dtype == np.int32 and full.ndim == 1
        assert np.array_equal(full, m.partial_dependence_codes(thr, col, n_trees=T)) and np.array_equal(full, m.partial_dependence_codes(thr, col, -1))
        for k in (None, 1, T - 1):
            got = m.partial_dependence_codes(thr, col, n_trees=k)
            walked = _walked_bins(m, bins, col, T if k is None else k)
            assert got.tolist() == _brute_force(walked, B), (col, k)
            assert got[0] == 0 and (np.diff(got) > 0).all() and got[-1] <= B
            if not walked:
                assert got.tolist() == [0]
                untested += 1
            assert len(got) <= len(full) and set(got.tolist()) <= set(full.tolist())        # a prefix never has more breaks
            fewer += len(got) < len(full)
            # the C ABI writes the same list
            out, count = np.full(B + 1, -7, np.int32), C.c_int(-1)
            assert lib.gbrl_hip_partial_dependence_codes(m._handle(), thr.ctypes.data, F, B, col, -1 if k is None else k, out.ctypes.data, C.byref(count)) == 0
            assert out[:count.value].tolist() == got.tolist() and (out[count.value:] == -7).all()
    assert untested >= 1, "every prefix of the fixture tests every column"
    assert fewer >= 1 or not grows, "no column of the fixture gains a break behind the first tree"


def test_codes_refusals(tmp_path):
    m = _loaded("obl_l2_q", tmp_path)
    md, T = m.get_metadata(), m.get_num_trees()
    F, B = md["input_dim"], md["n_bins"]
    thr = _table(m, np.random.default_rng(6))
    for col in (-1, F):
        with pytest.raises(RuntimeError, match=r"column %d is outside \[0, %d\)" % (col, F)):
            m.partial_dependence_codes(thr, col)
    for k in (0, T + 1, -2):
        with pytest.raises(RuntimeError, match=r"n_trees %d is outside \[1, %d\]" % (k, T)):
            m.partial_dependence_codes(thr, 0, n_trees=k)
    for bad in (np.zeros((F + 1, B), np.float32), np.zeros((F, B - 1), np.float32)):
        with pytest.raises(RuntimeError, match="partial_dependence_codes: .* the model has"):
            m.partial_dependence_codes(bad, 0)
    with pytest.raises(RuntimeError, match="n_features, n_bins"):
        m.partial_dependence_codes(np.zeros(F * B, np.float32), 0)
    with pytest.raises(RuntimeError, match="the model has no trees"):
        _empty().partial_dependence_codes(np.zeros((4, 256), np.float32), 0)
    lib = _lib()
    out, count = np.zeros(B + 1, np.int32), C.c_int(0)
    args = (thr.ctypes.data, F, B, 0, -1)
    assert lib.gbrl_hip_partial_dependence_codes(None, *args, out.ctypes.data, C.byref(count)) == E_INVALID and b"null model" in lib.gbrl_hip_last_error()
    assert lib.gbrl_hip_partial_dependence_codes(m._handle(), *args, None, C.byref(count)) == E_INVALID
    assert lib.gbrl_hip_partial_dependence_codes(m._handle(), *args, out.ctypes.data, None) == E_INVALID
    assert lib.gbrl_hip_partial_dependence_codes(m._handle(), None, F, B, 0, -1, out.ctypes.data, C.byref(count)) == E_INVALID
    # a value outside the column's thresholds: condition_bins' refusal, the tree is named; another column's curve does not need it
    gone = thr.copy()
    f = int(np.asarray(m.get_ensemble_data()["feature_indices"])[0, 0])
    gone[f] = 1e30
    with pytest.raises(RuntimeError, match=r"tree 0, condition 0 \(feature %d > .* does not compare against one of the data set's thresholds" % f):
        m.partial_dependence_codes(gone, f)
    assert lib.gbrl_hip_partial_dependence_codes(m._handle(), gone.ctypes.data, F, B, f, -1, out.ctypes.data, C.byref(count)) == E_UNSUPPORTED
    other = (f + 1) % F
    assert np.array_equal(m.partial_dependence_codes(gone, other), m.partial_dependence_codes(thr, other))


def test_pd_core_check_runs_clean_under_the_sanitizers(tmp_path):
    """pd_core.h without a device (tests/cxx/pd_core_check.cpp, built with the address and undefined-behaviour sanitizers): the break rule against
    brute force on random condition tables, the segment of every code, the cells of an entry, and the launch plan against its budget."""
    exe = tmp_path / "pd_core_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gbrl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "pd_core_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "all sections passed" in out.stdout, out.stdout + out.stderr
    assert len(out.stdout.strip().split("\n")) == 4, out.stdout


def test_launch_plan_stays_inside_the_budget_and_never_below_one():
    g = cpp.partial_dependence_geometry()
    assert g == {"partial_rows": 64, "launch_variants": 64, "max_launch_variants": 64, "scratch_budget": 64 << 20}
    budget, most = g["scratch_budget"], g["max_launch_variants"]
    assert most == cpp.permutation_geometry()["launch_variants"]
    for m in (1, 63, 64, 65, 257, 4097, 65536, 1 << 20, (1 << 20) + 1, 1 << 24, 123456789, 2 ** 31 - 1):
        for D in (1, 3, 8, 64, 65, 128):
            per = cpp.partial_dependence_geometry(m, D)["launch_variants"]
            one = 8 * D * -(-m // 64)
            assert 1 <= per <= most, (m, D, per)
            assert per == 1 or per * one <= budget, (m, D, per)
            assert per == most or (per + 1) * one > budget, (m, D, per)          # and no launch is cut shorter than the budget asks
    assert cpp.partial_dependence_geometry(1 << 20, 8)["launch_variants"] == 64 and cpp.partial_dependence_geometry(1 << 20, 128)["launch_variants"] == 4
    assert cpp.partial_dependence_geometry(2 ** 31 - 1, 128)["launch_variants"] == 1       # one variant's partials alone pass the budget: it still runs
    lib = _lib()
    rows, per, top, bud = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    lib.gbrl_hip_partial_dependence_geometry(4097, 8, C.byref(rows), C.byref(per), C.byref(top), C.byref(bud))
    assert (rows.value, per.value, top.value, bud.value) == (64, 64, 64, 64 << 20)
    lib.gbrl_hip_partial_dependence_geometry(4097, 8, None, None, None, None)


def test_cells_of_an_entry_are_the_row_major_product():
    """gbrl_hip_partial_dependence_cells is pd_core.h's pd_append_cells, the list the Python layer launches: its order is the order of the result's
    cell axes"""
    lib = _lib()
    a, b = np.array([0, 3, 7], np.int32), np.array([0, 5], np.int32)
    out = np.full((6, 4), -9, np.int32)
    assert lib.gbrl_hip_partial_dependence_cells(4, a.ctypes.data, 3, -1, None, 0, out.ctypes.data) == 0
    assert out[:3].tolist() == [[4, 0, -1, 0], [4, 3, -1, 0], [4, 7, -1, 0]] and (out[3:] == -9).all()
    assert lib.gbrl_hip_partial_dependence_cells(4, a.ctypes.data, 3, 9, b.ctypes.data, 2, out.ctypes.data) == 0
    assert out.tolist() == [[4, g0, 9, g1] for g0 in a.tolist() for g1 in b.tolist()]
    assert out.reshape(3, 2, 4)[2, 1].tolist() == [4, 7, 9, 5]
    for args in ((-1, a.ctypes.data, 3, -1, None, 0), (4, None, 3, -1, None, 0), (4, a.ctypes.data, 0, -1, None, 0), (4, a.ctypes.data, 3, 4, b.ctypes.data, 2),
                 (4, a.ctypes.data, 3, 9, None, 2), (4, a.ctypes.data, 3, 9, b.ctypes.data, 0)):
        assert lib.gbrl_hip_partial_dependence_cells(*args, out.ctypes.data) == E_INVALID, args
    assert lib.gbrl_hip_partial_dependence_cells(4, a.ctypes.data, 3, -1, None, 0, None) == E_INVALID


def test_pd_generic_hook_is_in_the_table_and_documented():
    names = re.findall(r"^\s+X\(([A-Z0-9_]+)\)", open(os.path.join(ROOT, "gbrl_amd", "csrc", "hooks.h")).read(), re.M)
    assert "PD_GENERIC" in names and names == sorted(names)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`GBRL_HIP_PD_GENERIC=1`" in doc[doc.index("## 5"):]
    assert "partial_dependence_prepared" in doc[doc.index("## 4"):doc.index("## 5")]
    assert "hooks::PD_GENERIC" in open(os.path.join(ROOT, "gbrl_amd", "csrc", "engine_pd.hip")).read()


def test_symbols_and_signatures():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for sym in ("gbrl_hip_partial_dependence_codes", "gbrl_hip_partial_dependence_prepared", "gbrl_hip_partial_dependence_geometry", "gbrl_hip_partial_dependence_cells"):
        assert hasattr(lib, sym), sym
    m = _empty()
    sig = m.partial_dependence_codes.__doc__.splitlines()[0]   # (how pybind11 spells an int depends on its version)
    assert "(self: gbrl_cpp.GBRL, thresholds: object, col: " in sig and ", n_trees: object = None)" in sig
    sig = m.partial_dependence_prepared.__doc__.splitlines()[0]
    assert "(self: gbrl_cpp.GBRL, ds: object, features: object, n_trees: object = None, rows: object = None, ice: bool = False, max_cells: " in sig and sig.endswith("= 4096) -> dict")
    assert "np.searchsorted(codes, g, side='right') - 1" in m.partial_dependence_prepared.__doc__


def test_refusals_that_need_no_data_set(tmp_path):
    m = _loaded("obl_l2_q", tmp_path)
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    before = p.read_bytes()
    with pytest.raises(RuntimeError, match="null data set"):
        m.partial_dependence_prepared(None, [0])
    with pytest.raises(RuntimeError, match="null data set"):
        m.partial_dependence_prepared(ds=None, features=[(0, 1)], n_trees=1, rows=np.arange(4, dtype=np.int32), ice=True, max_cells=8)
    with pytest.raises((RuntimeError, TypeError)):
        m.partial_dependence_prepared(object(), [0])
    lib = _lib()
    D = m.get_metadata()["output_dim"]
    variants, sums = np.array([[-1, 0, -1, 0], [0, 0, -1, 0]], np.int32), np.zeros((2, D), np.float64)
    stale = C.c_int(0)
    h, err = m._handle(), lib.gbrl_hip_last_error
    for ds, what in ((None, b"null data set"), (C.addressof(stale), b"destroyed")):
        assert lib.gbrl_hip_partial_dependence_prepared(h, ds, variants.ctypes.data, 2, None, 0, 16, -1, sums.ctypes.data, None, 0) == E_INVALID and what in err()
    assert lib.gbrl_hip_partial_dependence_prepared(None, None, variants.ctypes.data, 2, None, 0, 16, -1, sums.ctypes.data, None, 0) == E_INVALID and b"null model" in err()
    assert m.save(str(p)) == 0 and p.read_bytes() == before
