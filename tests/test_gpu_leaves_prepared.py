"""`predict_leaves_prepared` / `leaf_counts_prepared` (include/gbrl_hip.h): where the rows of a prepared data set land.  The reference is the NumPy
walk of tests/test_gpu_leaves.py over the FLOAT matrix the data set was made from, and np.bincount of it; everything is integers, compared exactly.
Models: T trees grown by step_prepared on 300 rows and random gradients at D = 2; the routed rows are a bound data set of n fresh rows."""
import ctypes

import numpy as np
import pytest

import gbrl_amd
from test_gpu_leaves import _grow, _model, _np_leaves

pytestmark = pytest.mark.gpu
D, NT, _CACHE = 2, 300, {}


def _grown(policy, F, T, depth, rows=NT):
    key = (policy, F, T, depth, rows)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * F + 10 * T + depth + (7 if policy == "greedy" else 0))
        m = _model(F, 0, D, depth, policy)
        X = rng.standard_normal((rows, F)).astype(np.float32)
        ds = m.prepare_dataset(X)
        for _ in range(T):
            m.step_prepared(ds, rng.standard_normal((rows, D)).astype(np.float32))
        assert m.get_num_trees() == T
        _CACHE[key] = (m, ds, X, m.get_ensemble_data(), rng)
    return _CACHE[key]


def _check(m, e, policy, ds, X, a=0, b=0, rows=None, rows_arg=None):
    """both calls against the walk on X (X[rows]) over [a, b); called twice: the same bytes"""
    stop = b if b else m.get_num_trees()
    n_leaves = np.asarray(e["values"]).shape[0]
    want = _np_leaves(e, policy, X if rows is None else X[rows], None, a, stop)
    rows_arg = rows if rows_arg is None else rows_arg
    leaves = [np.asarray(m.predict_leaves_prepared(ds, a, b, rows=rows_arg)) for _ in range(2)]
    counts = [m.leaf_counts_prepared(ds, a, b, rows=rows_arg) for _ in range(2)]
    assert leaves[0].dtype == np.int32 and leaves[0].shape == want.shape and counts[0].dtype == np.int64 and counts[0].shape == (n_leaves,)
    assert np.array_equal(leaves[0], want), "leaves differ from the NumPy walk at %s" % np.argwhere(leaves[0] != want)[:5].tolist()
    assert np.array_equal(counts[0], np.bincount(want[want >= 0].ravel(), minlength=n_leaves))
    assert leaves[0].tobytes() == leaves[1].tobytes() and counts[0].tobytes() == counts[1].tobytes()
    return counts[0]


# (F, T, depth, n, start, stop): n walks the tile edges, F one group / a full group / a partial last group / three groups, T the partial tree groups and
# T % 4 == 0 or not (16-byte or scalar index stores); depth 1 takes the in-wave aggregation of leaf_counts_prepared; one sub-range
TABLE = [(16, 16, 3, 1, 0, 0), (16, 16, 3, 63, 0, 0), (16, 16, 3, 64, 0, 0), (16, 16, 3, 65, 0, 0), (1, 17, 3, 200, 0, 0), (17, 20, 1, 65, 0, 0),
         (40, 33, 3, 200, 0, 0), (17, 15, 3, 64, 0, 0), (16, 1, 3, 65, 0, 0), (40, 33, 3, 65, 3, 30), (17, 20, 1, 200, 2, 19)]


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("F,T,depth,n,a,b", TABLE)
def test_against_the_numpy_walk_on_a_bound_data_set(policy, F, T, depth, n, a, b):
    m, ds, _, e, rng = _grown(policy, F, T, depth)
    Xv = rng.standard_normal((n, F)).astype(np.float32)
    counts = _check(m, e, policy, m.prepare_dataset(Xv, reference=ds), Xv, a, b)
    assert counts.sum() == n * ((b if b else T) - a)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_the_general_kernels(policy, monkeypatch):
    monkeypatch.setenv("GBRL_HIP_LEAVES_GENERIC", "1")
    for F, T, depth, n in ((16, 16, 3, 1), (17, 20, 1, 65)):
        m, ds, X, e, _ = _grown(policy, F, T, depth)
        _check(m, e, policy, ds, X, rows=np.arange(n, dtype=np.int32))
    _check(m, e, policy, ds, X, 2, 19)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("where", ["numpy", "device"])
def test_rows_with_duplicates_out_of_order(policy, where):
    import torch
    m, ds, X, e, _ = _grown(policy, 17, 20, 1)
    rows = np.array([299, 5, 5, 0, 64, 63, 127, 1] * 9 + [2], np.int32)   # 73 positions: two tiles
    t = torch.from_numpy(rows).cuda()
    arg = rows if where == "numpy" else (t.data_ptr(), (rows.size,), "torch.int32", "cuda")
    _check(m, e, policy, ds, X, rows=rows, rows_arg=arg)
    m3, ds3, X3, e3, _ = _grown(policy, 40, 33, 3)
    _check(m3, e3, policy, ds3, X3, 3, 30, rows=rows, rows_arg=arg)


def test_a_range_that_crosses_one_counter_chunk():
    F, depth, n = 8, 6, 4096
    chunk = gbrl_amd.GBRL.leaves_prepared_geometry((F + 15) // 16)[1]
    T = chunk // (1 << depth) + 5
    m, ds, X, e, _ = _grown("oblivious", F, T, depth, rows=n)
    n_leaves = np.asarray(e["values"]).shape[0]
    assert chunk < n_leaves <= 2 * chunk, "the trees came out too shallow to cross one chunk boundary: %d leaves" % n_leaves
    assert _check(m, e, "oblivious", ds, X).sum() == n * T


def test_cover_importance_from_a_data_set():
    m, ds, X, e, _ = _grown("oblivious", 17, 15, 3)
    got = m.feature_importance("cover", leaf_counts=m.leaf_counts_prepared(ds))
    assert np.array_equal(got, m.feature_importance("cover", leaf_counts=m.leaf_counts(X, None)))


@pytest.mark.parametrize("what,msg", [("foreign", "tree 0.*does not compare against one of the data set's thresholds"), ("destroyed", "destroyed"),
                                      ("range", "invalid tree range"), ("rows", "outside"), ("categorical", "categorical columns")])
def test_refusals(what, msg):
    m, ds, X, e, rng = _grown("oblivious", 16, 16, 3)
    bad, bad_ds, kw = m, ds, {}
    if what == "foreign":
        bad_ds = m.prepare_dataset(X * 3.0)
    elif what == "range":
        kw = dict(start_tree_idx=5, stop_tree_idx=17)
    elif what == "rows":
        kw = dict(rows=np.array([0, NT], np.int32))
    elif what == "categorical":
        bad = _model(3, 2, D, 3)
        _grow(bad, rng, 2, 3, 2, D)
    if what == "destroyed":   # (the C ABI owns this one)
        lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.gbrl_hip_dataset_create.argtypes, lib.gbrl_hip_dataset_create.restype = [vp, vp, ci, ci, ci], vp
        lib.gbrl_hip_dataset_destroy.argtypes, lib.gbrl_hip_last_error.restype = [vp], ctypes.c_char_p
        h = lib.gbrl_hip_dataset_create(m._handle(), X.ctypes.data, 0, NT, 16)
        lib.gbrl_hip_dataset_destroy(h)
        out, cnt = np.zeros((NT, 16), np.int32), np.zeros(np.asarray(e["values"]).shape[0], np.int64)
        lib.gbrl_hip_predict_leaves_prepared.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, ci]
        lib.gbrl_hip_leaf_counts_prepared.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]
        assert lib.gbrl_hip_predict_leaves_prepared(m._handle(), h, None, 0, NT, 0, 0, out.ctypes.data, 0) == -1 and msg.encode() in lib.gbrl_hip_last_error()
        assert lib.gbrl_hip_leaf_counts_prepared(m._handle(), h, None, 0, NT, 0, 0, cnt.ctypes.data) == -1 and msg.encode() in lib.gbrl_hip_last_error()
        assert not out.any() and not cnt.any()
    else:
        for call in (bad.predict_leaves_prepared, bad.leaf_counts_prepared):
            with pytest.raises(RuntimeError, match=call.__name__ + ".*" + msg if what != "rows" else msg):
                call(bad_ds, **kw)
    _check(m, e, "oblivious", ds, X)
