"""SHAP values on a prepared data set, on the GPU (GBRL.shap_prepared / GBRL.shap_importance_prepared; include/gbrl_hip.h, "SHAP values on a data set").

The oracle is built from calls that existed before them: ensemble_shap / tree_shap on the float32 observations the codes were made from, under
GBRL_HIP_SHAP_HOST=1 (the host evaluation, pinned to the reference's fixtures by tests/test_explain.py and tests/test_shap_edges_host.py).  Every
assertion is equality of the bytes; there is no tolerance anywhere in this file.

  1. the matrix equals the oracle: row counts around the samples per block of the launch plan, F on both sides of the 32-byte code record, D in
     {1, 3, 8}, oblivious depth 3 and greedy depth 4 (256 threads), oblivious depth 8 (128 threads), depth 12 (64 threads); tree_idx for the first,
     middle and last tree; a Linear schedule; two optimizers over disjoint outputs;
  2. edge rows: cells on a used threshold and one ulp to either side, NaN, +-inf, +-0.0 and a subnormal in every split column; "on the threshold"
     equals "one ulp below" in bytes;
  3. rows= with duplicates, from the host and from a device tensor: shap_prepared(ds, rows=r) == shap_prepared(ds)[r];
  4. the importance: sum / sum_abs equal gbrl_cpp.shap_sums_host of the matrix at m in {1, 63, 64, 65, 257, 4097}, across chunk_rows in {64, 128,
     default}, across two calls and across rows=None against arange(n); mean == sum / m; a column no tree tests gets exact zeros;
  5. the caches: ensemble_shap, shap_prepared on two data sets with different thresholds and a step_prepared between them, each equal to its oracle;
  6. the model's file bytes and ds.codes() are unchanged;
  7. the refusals.
The data and model recipe is tests/test_gpu_partial_dependence.py's: fit_prepared on 512 training rows with n_bins = 32, other rows bound with
reference=; the targets lean on columns 0, 15, 16 and F - 1 so that the trees use them (asserted)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases as K
import gbrl_amd
import shap_edges as E

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp

N_TRAIN, N_BINS = 512, 32


def _model(F, D, policy, depth, lr=0.1, n_bins=N_BINS, opts=None):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func="L2" if policy == "oblivious" else "Cosine",
                      generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=N_TRAIN)
    for o in opts or [dict(algo="SGD", scheduler="Const", init_lr=lr, start_idx=0, stop_idx=D)]:
        m.set_optimizer(**o)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _tested(F):
    return sorted({c for c in (0, 15, 16, F - 1) if 0 <= c < F})


def _data(rows, F, D, rng, W):
    X = rng.standard_normal((rows, F)).astype(np.float32)
    Y = (X @ W + 0.2 * rng.standard_normal((rows, D))).astype(np.float32)
    return X, (np.ascontiguousarray(Y[:, 0]) if D == 1 else np.ascontiguousarray(Y))


class _Env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        os.environ[self.name] = self.value

    def __exit__(self, *a):
        os.environ.pop(self.name, None)


class Case:
    """A model grown by fit_prepared on N_TRAIN rows, and n other rows under the same thresholds to explain."""

    def __init__(self, n, F, D, policy, T, depth=None, opts=None, seed=0, planned=True):
        self.n, self.F, self.D, self.T = n, F, D, T
        self.depth = depth or (3 if policy == "oblivious" else 4)
        rng = np.random.default_rng(1000 * n + 10 * F + D + T + seed)
        w = np.full(F, 0.4)
        for c, s in zip(_tested(F), (3.0, 2.5, 2.0, 1.5)):
            w[c] = s
        self.W = w[:, None] * rng.choice([-1.0, 1.0], size=(F, D))
        self.rng = rng
        self.m = _model(F, D, policy, self.depth, opts=opts)
        self.Xt, self.yt = _data(N_TRAIN, F, D, rng, self.W)
        self.ds_train = self.m.prepare_dataset(self.Xt)
        self.m.fit_prepared(self.ds_train, self.yt, T)
        assert self.m.get_num_trees() == T
        base, norm, offset = K.poly_vectors(self.depth)
        self.poly = (norm, base, offset)
        self.nt, self.per = E.plan(self.depth, D)
        assert (self.per >= 1) == planned
        self.bind(n)

    def bind(self, n):
        self.n = n
        self.X, _ = _data(n, self.F, self.D, self.rng, self.W)
        self.ds = self.m.prepare_dataset(self.X, reference=self.ds_train)
        self._oracle = {}

    def used(self):
        e = self.m.get_ensemble_data()
        depths, fidx = np.asarray(e["depths"]), np.asarray(e["feature_indices"])
        live = np.arange(fidx.shape[1])[None, :] < depths[:, None]
        return set(int(f) for f in fidx[live])

    def oracle(self, tree=None, X=None):
        """float32 [n, F, D] from the host evaluation on the observations (X: other rows than the case's own); the case's own are computed once per
        tree, shared, never written"""
        if X is None and tree in self._oracle:
            return self._oracle[tree]
        with _Env("GBRL_HIP_SHAP_HOST", "1"):
            obs = self.X if X is None else X
            phi = self.m.ensemble_shap(obs, None, *self.poly) if tree is None else self.m.tree_shap(tree, obs, None, *self.poly)
        phi = np.asarray(phi, np.float32)
        assert np.isfinite(phi).all()
        phi.setflags(write=False)
        if X is None:
            self._oracle[tree] = phi
        return phi

    def run(self, ds=None, **kw):
        return np.asarray(self.m.shap_prepared(self.ds if ds is None else ds, *self.poly, **kw))

    def importance(self, ds=None, **kw):
        return self.m.shap_importance_prepared(self.ds if ds is None else ds, *self.poly, **kw)


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bits = np.uint32 if a.dtype.itemsize == 4 else np.uint64 if a.dtype.itemsize == 8 else np.uint16
        bad = np.argwhere(a.view(bits) != b.view(bits))
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: %r against %r" % (what, len(bad), a.size, list(at), a[at], b[at]))
    return True


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


# F, D, policy, T, depth: every (F, D) of the issue's lists appears; the plans are 256 threads (depth 3, 4), 128 (depth 8) and 64 (depth 12)
MATRIX_CASES = [
    (1, 1, "oblivious", 4, 3, 256),
    (16, 3, "greedy", 5, 4, 256),
    (17, 8, "oblivious", 6, 3, 256),
    (40, 3, "greedy", 5, 4, 256),
    (40, 8, "oblivious", 3, 8, 128),
    (17, 3, "greedy", 2, 12, 64),
]


@pytest.mark.parametrize("F,D,policy,T,depth,threads", MATRIX_CASES)
def test_matrix_equals_the_host_evaluation_on_the_observations(F, D, policy, T, depth, threads, tmp_path):
    per = E.plan(depth, D)[1]
    k = Case(max(300, 2 * per + 1), F, D, policy, T, depth=depth)          # (256 samples per block at D = 1: the third block needs 513 rows)
    assert k.nt == threads and k.per == per
    tested, used = _tested(F), k.used()
    print("F %d: tested columns %s, used %s" % (F, tested, sorted(used)))
    assert 2 * len([c for c in tested if c in used]) >= len(tested), (tested, sorted(used))      # a condition on the inputs, as the partial dependence test asks
    assert {c >> 4 for c in used} == {c >> 4 for c in range(F)}, sorted(used)                    # every 32-byte code record of a row is read
    file0, codes0 = _file(k.m, tmp_path), np.asarray(k.ds.codes()).copy()
    whole = k.oracle()
    for n in sorted({1, per - 1, per, per + 1, 2 * per + 1, 300} - {0}):
        rows = np.arange(n, dtype=np.int32)
        got = k.run(rows=rows)
        assert got.shape == (n, F, D) and got.dtype == np.float32
        _same(got, whole[:n], "%d rows of %d samples per block" % (n, per))
    _same(k.run(), whole, "every row")
    for t in E.tree_picks(T):
        _same(k.run(tree_idx=t), k.oracle(t), "tree %d" % t)
    assert np.abs(whole).max() > 0
    assert _file(k.m, tmp_path) == file0 and _same(np.asarray(k.ds.codes()), codes0)


@pytest.mark.parametrize("opts", [
    [dict(algo="SGD", scheduler="Linear", init_lr=0.1, stop_lr=0.01, T=50, start_idx=0, stop_idx=3)],
    [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=1), dict(algo="SGD", scheduler="Const", init_lr=0.3, start_idx=1, stop_idx=3)],
], ids=["linear", "two_optimizers"])
def test_schedules_and_optimizers(opts):
    k = Case(65, 17, 3, "oblivious", 7, opts=opts)
    _same(k.run(), k.oracle(), "ensemble")
    _same(k.run(tree_idx=6), k.oracle(6), "last tree")
    r = k.importance()
    s, a = cpp.shap_sums_host(k.oracle())
    _same(r["sum"], s) and _same(r["sum_abs"], a)


@pytest.mark.parametrize("F,D,policy,T,depth", [(17, 3, "oblivious", 6, 3), (40, 8, "greedy", 5, 4), (17, 3, "greedy", 2, 12)])
def test_edge_rows(F, D, policy, T, depth):
    """Cells exactly on a used threshold and one float32 ulp to either side; NaN, +-inf, +-0.0 and a subnormal in every split column, and in every
    column at once.  x > v <=> code > bin for every float, so the matrix equals the oracle and ON a threshold equals one ulp BELOW it."""
    k = Case(8, F, D, policy, T, depth=depth)
    xs, _, triples = E.edge_rows(k.m, k.X, None)
    assert len(triples) >= 1 and np.isnan(xs).any() and np.isinf(xs).any()
    ds = k.m.prepare_dataset(xs, reference=k.ds_train)
    got = k.run(ds)
    _same(got, k.oracle(X=xs), "edge rows")
    for t in E.tree_picks(T):
        _same(k.run(ds, tree_idx=t), k.oracle(t, X=xs), "edge rows, tree %d" % t)
    differ = 0
    for below, on, above in triples:
        assert got[on].tobytes() == got[below].tobytes(), on
        differ += got[on].tobytes() != got[above].tobytes()
    assert differ >= 1          # (the thresholds are used ones: crossing one changes some row)


def test_rows_with_duplicates_from_host_and_device():
    k = Case(130, 17, 3, "oblivious", 6)
    whole = k.run()
    _same(whole, k.oracle())
    r = np.array([129, 0, 5, 5, 64, 63, 0, 129, 129, 17, 100], np.int32)
    _same(k.run(rows=r), whole[r], "host rows")
    t = torch.from_numpy(r).to("cuda:0")
    _same(k.run(rows=(t.data_ptr(), (len(r),), "torch.int32", "cuda")), whole[r], "device rows")
    _same(k.run(rows=r, tree_idx=3), k.oracle(3)[r], "host rows, one tree")
    a, b = k.importance(rows=r), cpp.shap_sums_host(whole[r])
    _same(a["sum"], b[0]) and _same(a["sum_abs"], b[1])
    assert a["n_rows"] == len(r)
    d = k.importance(rows=(t.data_ptr(), (len(r),), "torch.int32", "cuda"))
    _same(d["sum"], b[0]) and _same(d["sum_abs"], b[1])


@pytest.mark.parametrize("n,F,D,policy,T", [(1, 1, 1, "oblivious", 3), (63, 16, 3, "greedy", 5), (64, 17, 8, "oblivious", 6), (65, 40, 3, "greedy", 5),
                                            (257, 17, 1, "oblivious", 6), (4097, 40, 8, "greedy", 5)])
def test_importance_is_the_tile_rule_on_the_matrix(n, F, D, policy, T, tmp_path):
    k = Case(n, F, D, policy, T)
    file0, codes0 = _file(k.m, tmp_path), np.asarray(k.ds.codes()).copy()
    phi = k.run()
    _same(phi, k.oracle())
    s, a = cpp.shap_sums_host(phi)
    default = cpp.shap_geometry(F, D)["default_chunk_rows"]
    first = k.importance()
    assert first["chunk_rows"] == default and first["n_rows"] == n
    for key in ("sum", "sum_abs", "mean", "mean_abs"):
        assert first[key].dtype == np.float64 and first[key].shape == (F, D), key
    _same(first["sum"], s, "sum") and _same(first["sum_abs"], a, "sum_abs")
    _same(first["mean"], s / n) and _same(first["mean_abs"], a / n)
    for other, what in ((k.importance(), "a second call"), (k.importance(chunk_rows=64), "chunk_rows 64"), (k.importance(chunk_rows=128), "chunk_rows 128"),
                        (k.importance(chunk_rows=default), "the default, named"), (k.importance(rows=np.arange(n, dtype=np.int32)), "arange(n)")):
        for key in ("sum", "sum_abs", "mean", "mean_abs"):
            _same(other[key], first[key], what + ": " + key)
    assert k.importance(chunk_rows=64)["chunk_rows"] == 64 and k.importance(chunk_rows=128)["chunk_rows"] == 128
    unused = sorted(set(range(F)) - k.used())
    if F == 40:
        assert unused, "every column of the case is tested"
    for c in unused:          # a column no tree tests: exact zeros, +0.0
        assert first["sum"][c].tobytes() == np.zeros(D).tobytes() and first["sum_abs"][c].tobytes() == np.zeros(D).tobytes(), c
    assert (first["sum_abs"][sorted(k.used())] > 0).any()
    assert _file(k.m, tmp_path) == file0 and _same(np.asarray(k.ds.codes()), codes0)


def test_the_two_program_caches_do_not_disturb_each_other():
    """ensemble_shap (the float form's cached program), shap_prepared on two data sets with different thresholds (the codes form's, keyed on the
    model version and the thresholds id) and a step_prepared between them, interleaved: every call equals its oracle."""
    k = Case(70, 17, 3, "oblivious", 5)
    X2 = (k.X * 1.5 + 0.25).astype(np.float32)
    Xo, _ = _data(300, k.F, k.D, k.rng, k.W)
    own = k.m.prepare_dataset(Xo)                              # thresholds of its own (other rows: no value in common): another thresholds id
    assert not np.isin(np.asarray(own.thresholds()), np.asarray(k.ds_train.thresholds())).any()

    def device_float(X):
        with _Env("GBRL_HIP_SHAP_DEVICE_ONLY", "1"):
            return np.asarray(k.m.ensemble_shap(X, None, *k.poly))

    _same(device_float(k.X), k.oracle(), "1 float form")
    _same(k.run(), k.oracle(), "2 codes form")
    _same(device_float(X2), k.oracle(X=X2), "3 float form again")
    _same(k.run(), k.oracle(), "4 codes form again (cached program)")
    _same(k.run(tree_idx=2), k.oracle(2), "5 one tree (overwrites the codes form's program)")
    _same(k.run(), k.oracle(), "6 codes form (rebuilt)")
    # a tree grown on the data set with other thresholds: ds_train's thresholds cannot express it, own's can only express the new tree
    G = (Xo @ k.W).astype(np.float32)
    k.m.step_prepared(own, np.ascontiguousarray(G))
    assert k.m.get_num_trees() == 6
    k._oracle = {}
    with pytest.raises(RuntimeError, match=r"shap_prepared: tree 5, condition \d+ .* does not compare against one of the data set's thresholds"):
        k.run()
    with pytest.raises(RuntimeError, match=r"shap_prepared: tree 0, condition \d+ .* does not compare against"):
        k.run(own)
    _same(k.run(own, tree_idx=5), k.oracle(5, X=Xo), "7 the new tree on its own data set")
    _same(k.run(tree_idx=4), k.oracle(4), "8 an old tree on the first data set (other thresholds id)")
    _same(device_float(k.X), k.oracle(), "9 float form after the step")
    _same(k.run(tree_idx=0), k.oracle(0), "10")


def _collective():
    reduce_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)

    class Collective(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    never = reduce_t(lambda ctx, buf, n: 1)
    return Collective(None, 2, 0, never, never, never, never), never


def test_refusals(tmp_path):
    k = Case(65, 17, 3, "oblivious", 7)
    m, ds, F, D = k.m, k.ds, k.F, k.D
    norm, base, offset = k.poly
    file0, codes0 = _file(m, tmp_path), np.asarray(ds.codes()).copy()
    calls = (("shap_prepared", m.shap_prepared), ("shap_importance_prepared", m.shap_importance_prepared))

    for name, call in calls:
        def refused(word, *a, **kw):
            with pytest.raises(RuntimeError, match=word):
                call(*a, **kw)

        refused("null data set", None, *k.poly)
        # rows: step_prepared's rules
        refused(name + ": no rows", ds, *k.poly, rows=np.zeros(0, np.int32))
        refused(r"index 65 \(entry 1\) is outside \[0, 65\)", ds, *k.poly, rows=np.array([0, 65], np.int32))
        refused(r"index -1 \(entry 0\) is outside", ds, *k.poly, rows=np.array([-1], np.int32))
        refused("Expected array of format", ds, *k.poly, rows=np.array([0, 1], np.int64))
        # a missing polynomial array, or one whose shape is not max_depth's
        refused(name + ": norm_values is missing", ds, None, base, offset)
        refused(name + ": base_poly is missing", ds, norm, None, offset)
        refused(name + ": offset is missing", ds, norm, base, None)
        b4, n4, o4 = K.poly_vectors(4)
        refused(r"norm_values has 20 elements, the model's max_depth 3 needs shape \(4, 3\)", ds, n4, base, offset)
        refused(r"base_poly has 4 elements, the model's max_depth 3 needs shape \(3,\)", ds, norm, b4, offset)
        refused(r"offset has 16 elements, the model's max_depth 3 needs shape \(3, 3\)", ds, norm, base, o4)
        # a model without trees
        fresh = _model(F, D, "oblivious", 3)
        with pytest.raises(RuntimeError, match=name + ": the model has no trees"):
            getattr(fresh, name)(fresh.prepare_dataset(k.X), *k.poly)
        # what predict_continue_prepared refuses: another bin count, thresholds the trees do not compare against (the tree is named), output_dim > 128
        with pytest.raises(RuntimeError, match="n_bins"):
            call(_model(F, D, "oblivious", 3, n_bins=16).prepare_dataset(k.X), *k.poly)
        with pytest.raises(RuntimeError, match=name + r": tree \d+, condition \d+ .* does not compare against one of the data set's thresholds"):
            call(m.prepare_dataset(k.X), *k.poly)
        wide = _model(F, 129, "oblivious", 3)
        with pytest.raises(RuntimeError, match="output_dim > 128"):
            getattr(wide, name)(wide.prepare_dataset(k.X), *k.poly)
    with pytest.raises(RuntimeError, match=r"tree_idx 7 is outside \[0, 7\)"):
        m.shap_prepared(ds, *k.poly, tree_idx=7)
    with pytest.raises(RuntimeError, match=r"tree_idx -1 is outside \[0, 7\)"):
        m.shap_prepared(ds, *k.poly, tree_idx=-1)
    for bad in (-64, 0, 1, 63, 100):
        with pytest.raises(RuntimeError, match=r"shap_importance_prepared: chunk_rows %d is not a positive multiple of 64" % bad):
            m.shap_importance_prepared(ds, *k.poly, chunk_rows=bad)
    # a row-sharded model
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_set_collective.argtypes = [vp, vp]
    lib.gbrl_hip_shap_prepared.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci]
    lib.gbrl_hip_shap_importance_prepared.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp]
    coll, keep = _collective()
    assert lib.gbrl_hip_set_collective(m._handle(), C.byref(coll)) == 0, lib.gbrl_hip_last_error()
    try:
        for name, call in calls:
            with pytest.raises(RuntimeError, match=name + ": not available on a model with a communicator or collective hooks"):
                call(ds, *k.poly)
    finally:
        assert lib.gbrl_hip_set_collective(m._handle(), None) == 0
    # a shape with no launch plan: both are named, and there is no host evaluation to hand over to
    assert E.plan(17, 1) == (0, 0)
    deep = Case(8, 4, 1, "greedy", 1, depth=17, planned=False)
    for name in ("shap_prepared", "shap_importance_prepared"):
        with pytest.raises(RuntimeError, match=name + ": k_shap has no launch plan for max_depth 17, output_dim 1"):
            getattr(deep.m, name)(deep.ds, *deep.poly)
    # the C ABI: the documented status codes, nothing written
    nv, bp, of = norm.ctypes.data, base.ctypes.data, offset.ctypes.data
    h, d, err = m._handle(), ds._handle(), lib.gbrl_hip_last_error
    out, s, a = np.zeros((65, F, D), np.float32), np.zeros((F, D)), np.zeros((F, D))
    assert lib.gbrl_hip_shap_prepared(h, d, None, 0, 65, -1, nv, bp, of, None, 0) == -1 and b"no place for the result" in err()
    assert lib.gbrl_hip_shap_prepared(h, d, None, 0, 64, -1, nv, bp, of, out.ctypes.data, 0) == -1 and b"has 64 rows, the data set 65" in err()
    assert lib.gbrl_hip_shap_prepared(h, d, None, 0, 65, -2, nv, bp, of, out.ctypes.data, 0) == -1 and b"tree_idx -2 is outside" in err()
    assert lib.gbrl_hip_shap_prepared(h, d, None, 0, 65, -1, nv, None, of, out.ctypes.data, 0) == -1 and b"base_poly is missing" in err()
    assert lib.gbrl_hip_shap_importance_prepared(h, d, None, 0, 65, nv, bp, of, 0, None, a.ctypes.data, None) == -1 and b"no place for the result" in err()
    assert lib.gbrl_hip_shap_importance_prepared(h, d, None, 0, 65, nv, bp, of, 96, s.ctypes.data, a.ctypes.data, None) == -1 and b"chunk_rows 96" in err()
    assert lib.gbrl_hip_shap_importance_prepared(h, d, None, 0, 65, nv, bp, of, -64, s.ctypes.data, a.ctypes.data, None) == -1 and b"chunk_rows -64" in err()
    assert lib.gbrl_hip_shap_prepared(deep.m._handle(), deep.ds._handle(), None, 0, 8, -1, nv, bp, of, out.ctypes.data, 0) == -5 and b"no launch plan" in err()
    assert not out.any() and not s.any() and not a.any()
    # m * F * D >= 2^31: refused before anything is allocated or read through the pointers
    big = (1 << 31) // (F * D) + 1
    rows = np.zeros(big, np.int32)
    small = np.zeros(16, np.float32)
    assert big * F * D >= 1 << 31
    assert lib.gbrl_hip_shap_prepared(h, d, rows.ctypes.data, 0, big, -1, nv, bp, of, small.ctypes.data, 0) == -5
    assert b"pass rows= to explain fewer rows, or use shap_importance_prepared" in err() and not small.any()
    with pytest.raises(RuntimeError, match=r"2\^31 elements or more: pass rows= to explain fewer rows, or use shap_importance_prepared"):
        m.shap_prepared(ds, *k.poly, rows=rows)
    used = C.c_int(0)
    assert lib.gbrl_hip_shap_importance_prepared(h, d, None, 0, 65, nv, bp, of, 0, s.ctypes.data, a.ctypes.data, C.byref(used)) == 0, err()
    ws, wa = cpp.shap_sums_host(k.oracle())
    assert _same(s, ws) and _same(a, wa) and used.value == cpp.shap_geometry(F, D)["default_chunk_rows"]
    assert _file(m, tmp_path) == file0 and _same(np.asarray(ds.codes()), codes0)
