"""The walk over a prepared data set's bin codes on the GPU (GBRL.predict_continue_prepared, GBRL.fit_prepared; include/gbrl_hip.h).  Every
comparison is exact (bytes):
  * predict_continue_prepared against predict_continue on the observations the data set was made from -- both kernels (the streaming one and
    GBRL_HIP_CONTINUE_GENERIC=1), every range form, a NumPy base and a device base updated in place, all rows and an unsorted subset with
    duplicates -- at the tile edges (n around 64, F around the 16-feature code groups), every output width family, both policies and generators;
  * the same at cells that equal a threshold exactly, a constant column, signed zeros, infinities and a NaN, and independently the rule itself:
    a NumPy walk over ds.codes() and condition_bins(ds.thresholds()) with `code > bin` reaches the leaves predict_leaves reports;
  * the refusals that need a live data set;
  * fit_prepared against the loop a caller could write from public calls, against fit(shuffle=False) on fresh models (file bytes and the loss),
    warm starts, ensembles of depth-0 trees, and determinism.
"""
import ctypes as C
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -5
PREP_PHASES = ("transpose", "candidates", "binning")


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, opts="const", batch_size=5000, min_data_in_leaf=0):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size, min_data_in_leaf=min_data_in_leaf)
    if opts == "const":
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    elif opts == "linear":
        m.set_optimizer(algo="SGD", scheduler="Linear", init_lr=0.3, start_idx=0, stop_idx=D, stop_lr=0.01, T=9)
    else:   # two optimizers that split the outputs
        assert D >= 2
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D // 2)
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.25, start_idx=D // 2, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _data(n, F, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    W = rng.standard_normal((F, D)).astype(np.float32)
    Y = (np.tanh(X @ W) + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    return X, Y


def _shape(A, D):
    """[n, D] as the binding wants it: [n] when D == 1"""
    return np.ascontiguousarray(A[:, 0]) if D == 1 else np.ascontiguousarray(A)


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _dev(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _bias_base(m, n, D):
    return _shape(np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (n, 1)), D)


def _grow_on(m, ds, X, Y, trees, D, seed):
    """`trees` trees grown on the data set from gradients that depend on the observations"""
    rng = np.random.default_rng(seed)
    for _ in range(trees):
        G = (Y * rng.uniform(0.5, 1.5) + 0.2 * rng.standard_normal(Y.shape)).astype(np.float32)
        m.step_prepared(ds, _shape(G, D))


def _prepared_both(m, ds, base, a, b, rows=None):
    """the streaming kernel (where it takes the shape) and GBRL_HIP_CONTINUE_GENERIC=1: the same bits; returns them"""
    out = []
    for generic in ("0", "1"):
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            keep = base.copy()
            got = m.predict_continue_prepared(ds, base, a, b, rows)
            assert base.tobytes() == keep.tobytes(), "a NumPy base was modified"
            out.append(np.asarray(got))
    assert out[0].dtype == np.float32 and out[0].shape == base.shape
    assert out[0].tobytes() == out[1].tobytes(), "k_continue_codes and k_continue_codes_general differ over [%d, %d)" % (a, b)
    return out[0]


def _check_continue(m, ds, X, D, T, seed):
    """every range form, base form and row form of predict_continue_prepared against predict_continue on X"""
    import torch
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    k = T // 2
    bias = _bias_base(m, n, D)
    for a, b in ((0, T), (k, T), (k, k + 1), (k, k), (0, 0)):
        base = bias if a == 0 else np.asarray(m.predict_continue(X, None, bias, 0, a))
        stop = b if b != 0 else T          # (0 means n_trees)
        want = np.asarray(m.predict_continue(X, None, base, a, b))
        got = _prepared_both(m, ds, base, a, b)
        assert got.tobytes() == want.tobytes(), "[%d, %d): differs from predict_continue at rows %s" % (a, stop, np.argwhere(got != want)[:3].tolist())
        if a == b and b != 0:
            assert got.tobytes() == base.tobytes()
        # an unsorted subset with duplicates, host and device rows
        rows = rng.integers(0, n, size=max(1, (3 * n) // 4 + 1)).astype(np.int32)
        rows[-1] = rows[0]
        want_r = np.asarray(m.predict_continue(np.ascontiguousarray(X[rows]), None, np.ascontiguousarray(base[rows]), a, b))
        got_r = _prepared_both(m, ds, np.ascontiguousarray(base[rows]), a, b, rows)
        assert got_r.tobytes() == want_r.tobytes(), "[%d, %d) on a row subset differs" % (a, stop)
        # a device base is updated in place; device rows
        t = torch.from_numpy(base.copy()).cuda()
        assert m.predict_continue_prepared(ds, _dev(t), a, b) is None
        assert t.cpu().numpy().tobytes() == want.tobytes(), "[%d, %d): device base" % (a, stop)
        tr = torch.from_numpy(np.ascontiguousarray(base[rows])).cuda()
        drows = torch.from_numpy(rows).cuda()
        assert m.predict_continue_prepared(ds, _dev(tr), a, b, rows=_dev(drows)) is None
        assert tr.cpu().numpy().tobytes() == want_r.tobytes(), "[%d, %d): device base and rows" % (a, stop)


# ---- 1. continue from codes == continue from obs -------------------------------------------------------------------------------------------
CONTINUE_CASES = [
    # n, F, D, policy, depth, opts, n_bins, generator
    (1, 1, 1, "oblivious", 1, "const", 2, "Quantile"),
    (63, 16, 3, "greedy", 6, "const", 256, "Uniform"),
    (64, 17, 8, "oblivious", 6, "linear", 300, "Quantile"),
    (65, 33, 64, "greedy", 1, "two", 256, "Quantile"),
    (65, 1, 1, "greedy", 1, "linear", 300, "Uniform"),
    (4097, 16, 8, "oblivious", 6, "two", 256, "Quantile"),
    (4097, 128, 65, "oblivious", 6, "const", 256, "Uniform"),      # D > 64: the general kernel
    (4097, 128, 128, "greedy", 6, "const", 2, "Quantile"),
    (4097, 128, 3, "greedy", 6, "two", 256, "Uniform"),
    (4097, 33, 1, "oblivious", 1, "const", 2, "Uniform"),
]


@pytest.mark.parametrize("n,F,D,policy,depth,opts,n_bins,gen", CONTINUE_CASES)
def test_continue_from_codes_is_continue_from_obs(n, F, D, policy, depth, opts, n_bins, gen):
    X, Y = _data(n, F, D, seed=7000 + n + 31 * F + D)
    m = _model(F, D, policy=policy, depth=depth, n_bins=n_bins, opts=opts, gen=gen, score="Cosine" if policy == "greedy" else "L2")
    ds = m.prepare_dataset(X)
    T = 4
    _grow_on(m, ds, X, Y, T, D, seed=n + F)
    assert m.get_num_trees() == T
    if n > 1:
        assert np.asarray(m.get_ensemble_data()["depths"]).max() >= 1, "the trees have no conditions to walk"
    _check_continue(m, ds, X, D, T, seed=F + D)


# ---- 2. edge values ---------------------------------------------------------------------------------------------------------------------
def _edge_matrix(n, F, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-2, 3, size=(n, F)).astype(np.float32)      # five small integers: many cells equal a threshold exactly
    X[:, 1] = 1.5                                                # a constant column
    X[:, 2] = rng.standard_normal(n).astype(np.float32)
    X[rng.integers(0, n, 9), 3] = np.float32(-0.0)
    X[rng.integers(0, n, 9), 3] = np.float32(0.0)
    X[rng.integers(0, n, 5), 4] = np.inf
    X[rng.integers(0, n, 5), 4] = -np.inf
    X[rng.integers(0, n, 3), 2] = np.inf
    X[7, 5] = np.nan                                             # one NaN cell: below every threshold, it passes no condition
    return X


def _leaves_from_codes(e, md, codes, bins, n):
    """the global leaf of every (row, tree) from the codes alone: a numeric condition holds iff code > bin"""
    ti, depths, fi = (np.asarray(e[k]) for k in ("tree_indices", "depths", "feature_indices"))
    ineq = np.asarray(e["inequality_directions"])
    T, L = ti.shape[0], ineq.shape[0]
    code = lambda f: codes[f // 16, :, f % 16].astype(np.int64)
    out = np.full((n, T), -1, np.int64)
    for t in range(T):
        if md["grow_policy"] == "Oblivious":
            leaf = np.zeros(n, np.int64)
            for d in range(int(depths[t])):
                leaf |= (code(int(fi[t, d])) > bins[t, d]).astype(np.int64) << (int(depths[t]) - 1 - d)
            out[:, t] = ti[t] + leaf
        else:
            for leaf in range(L - 1, int(ti[t]) - 1, -1):       # the FIRST leaf in storage order that passes wins: assign from the back
                dep = int(depths[leaf])
                if dep == 0:
                    continue                                      # a depth-0 leaf never passes
                ok = np.ones(n, bool)
                for d in range(dep):
                    ok &= (code(int(fi[leaf, d])) > bins[leaf, d]) == bool(ineq[leaf, d])
                out[ok, t] = leaf
    return out


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_edge_values_and_the_rule_itself(policy):
    n, F, D, T = 500, 6, 2, 5
    X = _edge_matrix(n, F, seed=11)
    rng = np.random.default_rng(12)
    Y = (np.nan_to_num(X, nan=0.0, posinf=3.0, neginf=-3.0) @ rng.standard_normal((F, D)) + 0.1 * rng.standard_normal((n, D))).astype(np.float32)
    m = _model(F, D, policy=policy, depth=4, n_bins=16, score="L2")
    ds = m.prepare_dataset(X)                                    # (a NaN cell is accepted: its ordered key lies below every other)
    thr = ds.thresholds()
    assert not np.isnan(thr).any()
    codes = ds.codes()
    assert codes[0, 7, 5] == 0, "the NaN cell lies below every threshold"
    want_codes = np.zeros_like(codes)
    for f in range(F):
        want_codes[0, :, f] = (thr[f][None, :] < X[:, f][:, None]).sum(axis=1)
    assert codes.tobytes() == want_codes.tobytes()
    _grow_on(m, ds, X, Y, T, D, seed=13)
    _check_continue(m, ds, X, D, T, seed=14)
    # the rule, independently of the kernels' arithmetic
    bins = m.condition_bins(thr)
    got = _leaves_from_codes(m.get_ensemble_data(), m.get_metadata(), codes, bins, n)
    want = np.asarray(m.predict_leaves(X, None, 0, 0))
    assert np.array_equal(got, want), "code > bin routes rows %s differently" % np.argwhere(got != want)[:3].tolist()
    assert (bins >= 0).any()


# ---- 3. refusals with a live data set -----------------------------------------------------------------------------------------------------
def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_predict_continue_prepared.argtypes = [vp, vp, vp, ci, ci, vp, ci, ci, ci, vp]
    lib.gbrl_hip_fit_prepared.argtypes = [vp, vp, vp, ci, ci, vp]
    lib.gbrl_hip_dataset_destroy.argtypes = [vp]
    lib.gbrl_hip_dataset_destroy.restype = None
    lib.gbrl_hip_dataset_create.argtypes = [vp, vp, ci, ci, ci]
    lib.gbrl_hip_dataset_create.restype = vp
    return lib


def test_refusals_with_a_live_data_set(tmp_path):
    import torch
    n, F, D = 300, 5, 2
    X, Y = _data(n, F, D, seed=21)
    m = _model(F, D)
    ds = m.prepare_dataset(X)
    lib = _lib()
    err = lib.gbrl_hip_last_error
    # a tree from a plain step() on OTHER data: its thresholds are not the data set's
    X2, Y2 = _data(n, F, D, seed=22)
    m.step_prepared(ds, Y)
    m.step(X2, None, Y2)
    assert m.get_num_trees() == 2
    before = _file(m, tmp_path)
    base = _bias_base(m, n, D)
    keep = base.copy()
    with pytest.raises(RuntimeError, match=r"tree 1, condition \d+ \(feature \d+"):
        m.predict_continue_prepared(ds, base, 0, 0)
    with pytest.raises(RuntimeError, match="tree 1,"):
        m.predict_continue_prepared(ds, base, 1, 2)
    rc = lib.gbrl_hip_predict_continue_prepared(m._handle(), ds._handle(), None, 0, n, base.ctypes.data, 0, 0, 0, base.ctypes.data)
    assert rc == E_UNSUPPORTED and b"tree 1," in err()
    with pytest.raises(RuntimeError, match="tree 1,"):
        m.fit_prepared(ds, Y, 2)                       # a warm start continues from every tree
    assert np.asarray(m.predict_continue_prepared(ds, base, 0, 1)).tobytes() == np.asarray(m.predict_continue(X, None, base, 0, 1)).tobytes()
    assert base.tobytes() == keep.tobytes() and _file(m, tmp_path) == before
    # base of the wrong shape
    for bad in (np.zeros((n - 1, D), np.float32), np.zeros((n, D + 1), np.float32), np.zeros(n, np.float32)):
        with pytest.raises(RuntimeError, match="Expected base of shape"):
            m.predict_continue_prepared(ds, bad, 0, 1)
    with pytest.raises(RuntimeError, match="Expected base of shape"):
        m.predict_continue_prepared(ds, base, 0, 1, rows=np.arange(5, dtype=np.int32))
    with pytest.raises(RuntimeError, match="Expected targets of shape"):
        _model(F, D).fit_prepared(ds, Y[:-1], 2)
    # bad ranges
    for a, b in ((2, 1), (0, 3), (-1, 1)):
        with pytest.raises(RuntimeError, match="invalid tree range"):
            m.predict_continue_prepared(ds, base, a, b)
    # a data set with another n_bins, generator or width
    for kw, what in ((dict(n_bins=64), "n_bins"), (dict(gen="Uniform"), "generator_type")):
        other = _model(F, D, **kw)
        with pytest.raises(RuntimeError, match=what):
            other.predict_continue_prepared(ds, base, 0, 0)
        with pytest.raises(RuntimeError, match=what):
            other.fit_prepared(ds, Y, 1)
        assert other.get_num_trees() == 0
    wide = _model(F + 1, D)
    with pytest.raises(RuntimeError, match="Total number of features"):
        wide.predict_continue_prepared(ds, base, 0, 0)
    with pytest.raises(RuntimeError, match="Total number of features"):
        wide.fit_prepared(ds, Y, 1)
    # an out-of-range row, host and device: found before anything reads through it
    good = _model(F, D)
    good.step_prepared(ds, Y)
    for bad_row in (n, -1):
        rows = np.array([0, 3, bad_row, 2], np.int32)
        b4 = np.zeros((4, D), np.float32)
        with pytest.raises(RuntimeError, match="rows: index %d" % bad_row):
            good.predict_continue_prepared(ds, b4, 0, 1, rows=rows)
        t = torch.zeros((4, D), dtype=torch.float32, device="cuda")
        with pytest.raises(RuntimeError, match="rows: index %d" % bad_row):
            good.predict_continue_prepared(ds, _dev(t), 0, 1, rows=_dev(torch.from_numpy(rows).cuda()))
        assert not t.cpu().numpy().any()
    # batch_size <= 0
    with pytest.raises(RuntimeError, match="batch_size must be positive"):
        _model(F, D, batch_size=0).fit_prepared(ds, Y, 1)
    # output_dim 129
    big = _model(F, 129)
    with pytest.raises(RuntimeError, match="output_dim > 128"):
        big.predict_continue_prepared(ds, np.zeros((n, 129), np.float32), 0, 0)
    with pytest.raises(RuntimeError, match="output_dim > 128"):
        big.fit_prepared(ds, np.zeros((n, 129), np.float32), 1)
    # a destroyed data set (C ABI: the handle is looked up, never dereferenced)
    h = lib.gbrl_hip_dataset_create(good._handle(), X.ctypes.data, 0, n, F)
    assert h is not None
    lib.gbrl_hip_dataset_destroy(h)
    loss = C.c_float(0.0)
    assert lib.gbrl_hip_predict_continue_prepared(good._handle(), h, None, 0, n, base.ctypes.data, 0, 0, 0, base.ctypes.data) == E_INVALID and b"destroyed" in err()
    assert lib.gbrl_hip_fit_prepared(good._handle(), h, Y.ctypes.data, 0, 1, C.byref(loss)) == E_INVALID and b"destroyed" in err()
    assert base.tobytes() == keep.tobytes() and good.get_num_trees() == 1


# ---- 4. fit_prepared == the loop a caller could write today --------------------------------------------------------------------------------
def _batches(n, bs, iterations):
    """fit()'s batches: contiguous ranges of bs rows in row order, wrapping to row 0 (fitter.cpp:120, 228-231)"""
    start = 0
    for _ in range(iterations):
        bn = bs if start + bs < n else n - start
        yield start, bn
        start += bn
        if start >= n:
            start = 0


def _manual_loop(m, ds, X, Y, D, bs, iterations, bias):
    n = X.shape[0]
    m.set_bias(np.asarray(bias, np.float32))
    P = _bias_base(m, n, D)
    through = {}
    for start, bn in _batches(n, bs, iterations):
        sl = slice(start, start + bn)
        T = m.get_num_trees()
        a = through.get(start, 0)
        if a < T:
            P[sl] = np.asarray(m.predict_continue(np.ascontiguousarray(X[sl]), None, np.ascontiguousarray(P[sl]), a, T))
        through[start] = T
        g = np.ascontiguousarray((P[sl] - _shape(Y, D)[sl]).astype(np.float32))
        m.step_prepared(ds, g, rows=None if bn == n else np.arange(start, start + bn, dtype=np.int32))


@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("n,bs,T", [(4096, 5000, 6), (1000, 384, 7), (4100, 4096, 5)])
def test_fit_prepared_is_the_loop_a_caller_could_write(n, bs, T, policy, score, gen, tmp_path):
    F, D = 7, 3
    X, Y = _data(n, F, D, seed=40 + n)
    a = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    ds = a.prepare_dataset(X)
    a.fit_prepared(ds, Y, T)
    assert a.get_num_trees() == T
    b = _model(F, D, policy=policy, score=score, gen=gen, batch_size=bs)
    _manual_loop(b, ds, X, Y, D, bs, T, a.get_bias())
    assert _file(a, tmp_path) == _file(b, tmp_path)


# ---- 5. fit_prepared == fit(shuffle=False) on fresh models ---------------------------------------------------------------------------------
def _fit_both(n, bs, T, F, D, tmp_path, **kw):
    X, Y = _data(n, F, D, seed=50 + n + D)
    a = _model(F, D, batch_size=bs, **kw)
    loss_a = a.fit(X, None, _shape(Y, D), T, False, "MultiRMSE")
    b = _model(F, D, batch_size=bs, **kw)
    ds = b.prepare_dataset(X)
    loss_b = b.fit_prepared(ds, _shape(Y, D), T)
    print("fit loss %r  fit_prepared loss %r  trees %d / %d" % (loss_a, loss_b, a.get_num_trees(), b.get_num_trees()))
    assert a.get_num_trees() == b.get_num_trees() == T
    assert np.asarray(b.get_ensemble_data()["depths"]).min() >= 1, "a tree without a split"
    assert _file(a, tmp_path) == _file(b, tmp_path), "the saved files differ"
    assert np.float32(loss_a).tobytes() == np.float32(loss_b).tobytes(), "loss %r != %r" % (loss_a, loss_b)


@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("n,bs,T", [(4096, 5000, 6), (1000, 384, 7), (4100, 4096, 5)])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_fit_prepared_is_fit_without_shuffle(D, n, bs, T, policy, score, gen, tmp_path):
    _fit_both(n, bs, T, 7, D, tmp_path, policy=policy, score=score, gen=gen)


@pytest.mark.parametrize("opts,D", [("linear", 3), ("two", 8)])
def test_fit_prepared_is_fit_with_a_schedule_and_with_two_optimizers(opts, D, tmp_path):
    _fit_both(1000, 384, 7, 7, D, tmp_path, policy="oblivious", score="L2", gen="Quantile", opts=opts)


# ---- 6. warm start --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs", [(1000, 5000), (999, 333)])      # one batch per cycle; three, so that 3 iterations are a whole cycle
def test_a_warm_start_continues_the_loop(n, bs, tmp_path):
    F, D = 7, 3
    X, Y = _data(n, F, D, seed=60 + n)
    a = _model(F, D, batch_size=bs)
    ds = a.prepare_dataset(X)
    a.fit_prepared(ds, Y, 3)
    bias = np.asarray(a.get_bias()).copy()
    loss_a = a.fit_prepared(ds, Y, 2)
    assert np.asarray(a.get_bias()).tobytes() == bias.tobytes(), "a warm start keeps the bias"
    b = _model(F, D, batch_size=bs)
    loss_b = b.fit_prepared(ds, Y, 5)
    assert a.get_num_trees() == b.get_num_trees() == 5
    assert _file(a, tmp_path) == _file(b, tmp_path)
    assert np.float32(loss_a).tobytes() == np.float32(loss_b).tobytes()


# ---- 7. stumps ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [5000, 200])
def test_an_ensemble_of_depth_zero_trees(bs, tmp_path):
    n, F, D, T = 500, 5, 2, 3
    X, Y = _data(n, F, D, seed=70)
    kw = dict(policy="greedy", score="Cosine", gen="Uniform", batch_size=bs, min_data_in_leaf=n + 1)
    a = _model(F, D, **kw)
    loss_a = a.fit(X, None, Y, T, False, "MultiRMSE")
    b = _model(F, D, **kw)
    ds = b.prepare_dataset(X)
    loss_b = b.fit_prepared(ds, Y, T)
    e = b.get_ensemble_data()
    assert b.get_num_trees() == T and np.asarray(e["depths"]).tolist() == [0] * T, "every tree is a depth-0 stump"
    assert _file(a, tmp_path) == _file(b, tmp_path)
    assert np.float32(loss_a).tobytes() == np.float32(loss_b).tobytes(), "loss %r != %r" % (loss_a, loss_b)


# ---- 8. determinism and phases ----------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_no_preparation_phase(tmp_path):
    n, F, D, T = 3000, 20, 4, 5
    X, Y = _data(n, F, D, seed=80)
    files, losses = [], []
    for _ in range(2):
        m = _model(F, D, batch_size=1024)
        ds = m.prepare_dataset(X)
        m.set_profiling(2)
        losses.append(m.fit_prepared(ds, Y, T))
        phases = m.last_phase_times()
        assert "continue_codes" in phases and "grad_stats" in phases, sorted(phases)
        assert not any(p in phases for p in PREP_PHASES), sorted(phases)
        m.set_profiling(0)
        files.append(_file(m, tmp_path))
    assert files[0] == files[1] and np.float32(losses[0]).tobytes() == np.float32(losses[1]).tobytes()
