"""GBRL.quantile_leaves_prepared on the GPU (include/gbrl_hip.h, "Quantile regression"; gbrl_amd/csrc/leaf_quantile.hip) against the host rule, bytes only.
tests/test_quantile_host.py holds gbrl_cpp.leaf_quantile_host and gbrl_cpp.quantile_rank to np.sort and to fractions; here a tree or two are grown with
step_prepared, the rows are routed with predict_leaves on the observations, the residuals are fl32(pred - targets) in NumPy, and
  1. values, counts and ranks are the host rule's with no tolerance, through the select path and the general (sort) path, which return the same bytes;
  2. the model holds those values for that tree and every other tree is untouched; predict sees them (the mirror was sent again);
  3. rows= (duplicates, a subset that misses a leaf) indexes pred and targets by position; tree=0 of two trees takes the tiled bias;
  4. what the kernel refuses (a target or a prediction that is not finite) leaves the model bytes as they were;
  5. GBRL.objective_gradient(..., 'quantile', alpha=) gives the host gradient's bytes and the float64 pinball loss within the summation bound;
  6. 1. again on the key families of tests/golden/quantile_cases.py (keys that share a prefix down to the last digit, denormals, the largest
     floats), with the rank on the edge of a tie run, at the row counts where the count pass, the target pass and the sort's scan take another
     trip (up to 131073 rows), at 128 outputs and on a tree whose leaf ids need two bytes; every such test asserts the path and the geometry it is for.
"""
import math
import os

import numpy as np
import pytest

import gbrl_amd
import quantile_cases as Q   # tests/golden (conftest.py puts it on the path)

pytestmark = pytest.mark.gpu

cpp = gbrl_amd.gbrl_cpp
f32 = np.float32
GEO = cpp.leaf_quantile_geometry()


def _model(F, D, policy, depth, n_bins=16, min_leaf=None):
    kw = {} if min_leaf is None else {"min_data_in_leaf": min_leaf}
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func="L2", generator_type="Quantile",
                      grow_policy=policy, device="cpu", batch_size=5000, **kw)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


def _levels(D):
    return np.array([0.05, 0.5, 0.95], f32) if D == 3 else np.linspace(0.05, 0.95, D).astype(f32)   # one level per output


N_GROW = 200   # the trees are grown on this many rows; the leaves are taken on rows of data sets bound to the same thresholds
_CASES = {}


def _targets(rng, n, D):
    return rng.integers(0, 3, (n, D)).astype(f32)   # drawn from {0, 1, 2}: massive ties


def _case(F, D, policy, depth, trees=1, n_grow=N_GROW):
    """a model of `trees` trees grown on the pinball gradient, its data, and the prediction in front of every tree"""
    key = (F, D, policy, depth, trees, n_grow)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * F + 10 * D + depth + (7 if policy == "greedy" else 0))
        X = rng.standard_normal((n_grow, F)).astype(f32)
        T = _targets(rng, n_grow, D)
        a = _levels(D)
        m = _model(F, D, policy, depth, min_leaf=1 if n_grow != N_GROW else None)
        m.set_bias(rng.normal(1.0, 0.5, D).astype(f32))
        ds = m.prepare_dataset(X)
        P = np.tile(np.asarray(m.get_bias(), f32).reshape(1, D), (n_grow, 1))
        before = []
        for t in range(trees):
            before.append(P.copy())
            G = cpp.objective_gradient_host(_shape(P, D), _shape(T, D), "quantile", alpha=a).reshape(n_grow, D)
            # a signal the tree can split on, whatever the targets: the gradient plus a smooth function of the features
            G = (G + 0.5 * np.sign(X[:, :1]) + 0.25 * np.sign(X[:, 1:2]) + (0.1 * X[:, 2:3] * X[:, 3:4] if n_grow != N_GROW else 0)).astype(f32)
            m.step_prepared(ds, _shape(G, D))
            P = np.asarray(m.predict_continue_prepared(ds, _shape(P, D), t, t + 1)).reshape(n_grow, D)
        _CASES[key] = (m, ds, X, T, before)
    return _CASES[key]


def _tree_span(m, tree):
    ens = m.get_ensemble_data()
    ti = np.asarray(ens["tree_indices"])
    leaf0 = int(ti[tree])
    leaf1 = int(ti[tree + 1]) if tree + 1 < len(ti) else int(np.asarray(ens["values"]).shape[0])
    return ens, leaf0, leaf1


def _check(m, ds_n, Xn, pred, T, D, tree, policy, alpha, rows=None, paths=("0", "1"), select=None):
    """both kernel paths against the host rule; returns (values the model holds afterwards, counts).  select = True / False: the calls are
    profiled, and the one without GBRL_HIP_CONTINUE_GENERIC must say that the select path took it (True) or the sort (False); the other the sort"""
    if select is not None:
        m.set_profiling(2)
        try:
            return _check(m, ds_n, Xn, pred, T, D, tree, policy, alpha, rows=rows, paths=tuple((g, select and g == "0") for g in paths))
        finally:
            m.set_profiling(0)
    sel = np.arange(Xn.shape[0]) if rows is None else rows
    ens0, leaf0, leaf1 = _tree_span(m, tree)
    NL = leaf1 - leaf0
    dep = np.asarray(ens0["depths"])
    depths = np.full(NL, dep[tree], np.int32) if policy == "oblivious" else dep[leaf0:leaf1].astype(np.int32)
    n = len(sel)
    leaves = (np.asarray(m.predict_leaves(np.ascontiguousarray(Xn[sel]), None, tree, tree + 1)).reshape(n) - leaf0).astype(np.int32)
    x = (pred.reshape(n, D) - T.reshape(n, D)).astype(f32)
    host = cpp.leaf_quantile_host(x, leaves, NL, alpha)
    old = np.asarray(ens0["values"], f32).reshape(-1, D).copy()
    keep = (host["counts"] == 0) | (depths <= 0)
    want = np.where(keep[:, None], old[leaf0:leaf1], host["values"]).astype(f32)
    kw = {} if rows is None else {"rows": np.asarray(rows, np.int32)}
    got = []
    for generic in paths:   # the select path (where the tree fits it) and the general one
        generic, took_select = generic if isinstance(generic, tuple) else (generic, None)
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            r = m.quantile_leaves_prepared(ds_n, _shape(pred, D), _shape(T.reshape(n, D), D), alpha, tree=tree, **kw)
        if took_select is not None:
            assert dict(m.last_phase_times())["quantile_select"] == (1.0 if took_select else 0.0), "generic = %s took the other path" % generic
        assert sorted(r) == ["counts", "ranks", "values"]
        assert r["values"].dtype == f32 and r["values"].shape == (NL, D) and r["counts"].dtype == np.int64 and r["counts"].shape == (NL,)
        assert r["ranks"].dtype == np.int64 and r["ranks"].shape == (NL, D)
        assert r["counts"].tobytes() == host["counts"].tobytes(), "generic = %s: the counts differ\n%r\n%r" % (generic, r["counts"], host["counts"])
        assert r["ranks"].tobytes() == host["ranks"].tobytes(), "generic = %s: the ranks differ" % generic
        assert r["values"].tobytes() == want.tobytes(), "generic = %s: the values differ from the host rule's\n%r\n%r" % (generic, r["values"], want)
        now = np.asarray(m.get_ensemble_data()["values"], f32).reshape(-1, D)
        assert now[leaf0:leaf1].tobytes() == want.tobytes()
        assert now[:leaf0].tobytes() == old[:leaf0].tobytes() and now[leaf1:].tobytes() == old[leaf1:].tobytes(), "another tree's values changed"
        got.append((r["values"].tobytes(), r["counts"].tobytes(), r["ranks"].tobytes()))
    assert len(set(got)) == 1
    ok = (leaves >= 0) & (leaves < NL)
    assert int(host["counts"].sum()) == int(ok.sum()) and (NL == 1 or ok.all())
    return want, host["counts"]


SHAPES = [(n, 17, 3) for n in (1, 63, 64, 65, 200)] + [(65, 16, 1), (65, 16, 8), (65, 16, 65)]


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("depth", [1, 3, 6])
@pytest.mark.parametrize("n,F,D", SHAPES)
def test_values_are_the_host_rules(n, F, D, depth, policy):
    m, ds, X, T, before = _case(F, D, policy, depth)
    assert m.get_num_trees() == 1
    Xn = np.ascontiguousarray(X[:n])
    ds_n = ds if n == N_GROW else m.prepare_dataset(Xn, reference=ds)
    _check(m, ds_n, Xn, before[0][:n], T[:n], D, 0, policy, _levels(D))


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_one_row_more_than_a_chunk_and_all_rows_equal(policy):
    """rows_per_chunk + 1 rows: the count pass takes a second chunk of one row.  Then every row with the same targets at the tiled bias: one key per column"""
    D = 3
    m, ds, X, T, before = _case(17, D, policy, 3)
    n = GEO["rows_per_chunk"] + 1
    rng = np.random.default_rng(n)
    Xn = rng.standard_normal((n, 17)).astype(f32)
    ds_n = m.prepare_dataset(Xn, reference=ds)
    pred = np.tile(before[0][:1], (n, 1))
    _check(m, ds_n, Xn, pred, _targets(rng, n, D), D, 0, policy, _levels(D))
    Teq = np.tile(np.array([[2.0, -0.0, 1.0]], f32), (n, 1))
    want, counts = _check(m, ds_n, Xn, pred, Teq, D, 0, policy, _levels(D))
    x = (pred[0] - Teq[0]).astype(f32)
    assert all(want[l].tobytes() == x.tobytes() for l in range(len(counts)) if counts[l] > 0)
    _CASES.pop((17, D, policy, 3, 1, N_GROW))


def test_a_greedy_tree_with_more_leaves_than_the_select_path_takes():
    D, n = 3, 4000
    m, ds, X, T, before = _case(8, D, "greedy", 8, n_grow=n)
    ens, leaf0, leaf1 = _tree_span(m, 0)
    assert leaf1 - leaf0 > GEO["max_select_leaves"], "the tree has %d leaves: the case would run the select path" % (leaf1 - leaf0)
    m.set_profiling(2)
    try:
        _check(m, ds, X, before[0], T, D, 0, "greedy", _levels(D), paths=("0",))
        assert dict(m.last_phase_times())["quantile_select"] == 0.0
    finally:
        m.set_profiling(0)
    sub = np.random.default_rng(5).permutation(n)[:700].astype(np.int32)   # many leaves without a row
    want, counts = _check(m, ds, X, np.ascontiguousarray(before[0][sub]), np.ascontiguousarray(T[sub]), D, 0, "greedy", _levels(D), rows=sub)
    assert (counts == 0).any()


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_rows_index_pred_by_position(policy):
    D = 3
    m, ds, X, T, before = _case(17, D, policy, 3)
    rng = np.random.default_rng(3)
    for rows in (np.int32([5, 5, 7, 0, 199, 5, 64, 63]), rng.permutation(N_GROW)[:131].astype(np.int32)):
        _check(m, ds, X, np.ascontiguousarray(before[0][rows]), np.ascontiguousarray(T[rows]), D, 0, policy, _levels(D), rows=rows)
    # a subset that misses a leaf: that leaf keeps its value and counts 0
    ens, leaf0, leaf1 = _tree_span(m, 0)
    leaves = np.asarray(m.predict_leaves(X, None, 0, 1)).reshape(-1) - leaf0
    present = np.unique(leaves)
    assert len(present) >= 2
    gone = int(present[0])
    rows = np.nonzero(leaves != gone)[0].astype(np.int32)
    old = np.asarray(ens["values"], f32).reshape(-1, D)[leaf0 + gone].copy()
    want, counts = _check(m, ds, X, np.ascontiguousarray(before[0][rows]), np.ascontiguousarray(T[rows]), D, 0, policy, _levels(D), rows=rows)
    assert counts[gone] == 0 and want[gone].tobytes() == old.tobytes()


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_tree_zero_of_two_and_the_last(policy, tmp_path):
    D = 3
    m, ds, X, T, before = _case(16, D, policy, 3, trees=2)
    assert m.get_num_trees() == 2
    a = _levels(D)
    bias = np.tile(np.asarray(m.get_bias(), f32).reshape(1, D), (N_GROW, 1))
    assert before[0].tobytes() == bias.tobytes()
    _check(m, ds, X, before[0], T, D, 0, policy, a)            # pred = the tiled bias
    # tree 1 at the prediction over the NEW tree 0; tree = -1 names it
    P1 = np.asarray(m.predict_continue_prepared(ds, bias, 0, 1)).reshape(N_GROW, D)
    want, _ = _check(m, ds, X, P1, T, D, 1, policy, a)
    r = m.quantile_leaves_prepared(ds, P1, T, a)
    assert r["values"].tobytes() == want.tobytes()
    # predict reads the new values: the walk over the observations, the walk over the codes and a model loaded from the file agree
    pa = np.asarray(m.predict(X, None))
    pb = np.asarray(m.predict_continue_prepared(ds, bias, 0, 2))
    p = tmp_path / "m.gbrl_model"
    assert m.save(str(p)) == 0
    pc = np.asarray(gbrl_amd.GBRL.load(str(p)).predict(X, None))
    assert pa.tobytes() == pb.tobytes() == pc.tobytes()
    _CASES.pop((16, D, policy, 3, 2, N_GROW))


@pytest.mark.parametrize("generic", ["0", "1"])
def test_refusals_leave_the_model_bytes(generic, tmp_path):
    D = 3
    m, ds, X, T, before = _case(16, D, "oblivious", 3)
    a = _levels(D)
    keep = _file(m, tmp_path)
    bad = []
    for v in (np.inf, -np.inf, np.nan):
        t = T.copy(); t[77, 1] = v
        bad.append((before[0], t, "target"))
        p = before[0].copy(); p[130, 2] = v
        bad.append((p, T, "prediction"))
    big = before[0].copy(); big[3, 0] = f32(3e38)
    tbig = T.copy(); tbig[3, 0] = f32(-3e38)
    bad.append((big, tbig, "residual"))
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        for p, t, what in bad:
            with pytest.raises(RuntimeError, match=what):
                m.quantile_leaves_prepared(ds, p, t, a)
            assert _file(m, tmp_path) == keep
        for kw, what in ((dict(tree=1), "tree"), (dict(tree=-2), "tree")):
            with pytest.raises(RuntimeError, match=what):
                m.quantile_leaves_prepared(ds, before[0], T, a, **kw)
        for alpha, what in (([0.5, 0.5, 1.0], r"alpha\[2\]"), ([0.5, 0.5], "one level per output"), (float("nan"), r"alpha\[0\]"), (None, "needs alpha")):
            with pytest.raises(RuntimeError, match=what):
                m.quantile_leaves_prepared(ds, before[0], T, alpha)
        with pytest.raises(RuntimeError):
            m.quantile_leaves_prepared(ds, before[0][:50], T[:50], a)
        assert _file(m, tmp_path) == keep
        # and the same call with clean inputs goes through, twice with the same bytes
        r1 = m.quantile_leaves_prepared(ds, before[0], T, a)
        f1 = _file(m, tmp_path)
        r2 = m.quantile_leaves_prepared(ds, before[0], T, a)
        assert _file(m, tmp_path) == f1 and f1 != keep
        assert all(r1[k].tobytes() == r2[k].tobytes() for k in r1)
    _CASES.pop((16, D, "oblivious", 3, 1, N_GROW))   # the shared model now holds quantile values: the next user grows its own


@pytest.mark.parametrize("depth,generic,select", [(3, "0", 1.0), (6, "0", 1.0), (3, "1", 0.0)])
def test_the_kernel_path_is_the_one_named(depth, generic, select):
    """the phase list of a profiled call names the step and says which path took it: both paths are really run above"""
    D = 3
    m, ds, X, T, before = _case(17, D, "oblivious", depth)
    m.set_profiling(2)
    try:
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            m.quantile_leaves_prepared(ds, before[0], T, _levels(D))
        phases = dict(m.last_phase_times())
    finally:
        m.set_profiling(0)
    assert "quantile_leaves" in phases and phases["quantile_leaves"] > 0.0
    assert phases["quantile_select"] == select


# ---- the key families of tests/golden/quantile_cases.py and the row counts at which the kernels' loops take another trip ----------------------------------
# tests/test_quantile_host.py holds the host rule to np.sort on every family; pred = 0 and targets = -x make fl32(pred - targets) the family's x.
MAX_COUNT_BLOCKS = 32    # kMaxCountBlocks of leaf_quantile.hip: the count pass has at most this many blocks per output, each striding over the chunks
SORT_TILE = 2048         # kRadixSortTile: the elements of one tile of radix_sort.hip
SCAN_SLICE = 4096        # kScanSlice: the words k_radix_scan takes per trip, of the 256 per tile of a segment
_BOUND = {}


def _bound(m, ds, n, F):
    """n rows of fresh observations and their data set on the thresholds of ds"""
    key = (id(ds), n)
    if key not in _BOUND:
        if len(_BOUND) >= 3:
            _BOUND.clear()
        Xn = np.random.default_rng(n).standard_normal((n, F)).astype(f32)
        _BOUND[key] = (ds, Xn, m.prepare_dataset(Xn, reference=ds))
    return _BOUND[key][1:]


def _last_row_decides(targets):
    """the last row gets the largest residual of every column (above every value of the distinct family): where it is alone in its chunk or
    its tile, a pass that loses it moves every rank of its leaf, and with distinct keys every value"""
    out = targets.copy()
    out[-1] = -np.array([0x50000001], np.uint32).view(f32)[0]
    return out


def _geometry(n):
    """(count blocks per output, chunks block 0 takes, slices of the sort's scan) at n rows"""
    chunks = -(-n // GEO["rows_per_chunk"])
    blocks = min(chunks, MAX_COUNT_BLOCKS)
    return blocks, -(-chunks // blocks), -(-256 * -(-n // SORT_TILE) // SCAN_SLICE)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("name", Q.FAMILIES)
def test_key_families_are_the_host_rules(name, policy):
    D, n = 3, 2049
    m, ds, X, T, before = _case(17, D, policy, 3)
    Xn, ds_n = _bound(m, ds, n, 17)
    pred, targets = Q.family(name, n, D, seed=1)
    want, counts = _check(m, ds_n, Xn, pred, targets, D, 0, policy, _levels(D), select=True)
    assert (counts > 0).sum() >= 2
    if name == "denormal_by_subtraction":   # the values are denormals, not zeros: nothing was flushed
        live = want[counts > 0]
        assert (np.abs(live) < Q.SMALLEST_NORMAL).all() and (live != 0).any()


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("c", [64, 256])
def test_the_rank_on_the_edge_of_a_tie_run(c, policy):
    """every leaf has c (then c + 1) rows, the larger half of them b and the others a < b, two neighbouring floats: at the levels 1/4, 1/2, 3/4
    the k-th largest is inside the run of b, on its edge (the last b at c rows, the first a at c + 1 rows with c / 2 of b, the last b again with
    c / 2 + 1 of b) and inside the run of a.  Only the last digit tells a from b"""
    D = 3
    alpha = np.array([0.25, 0.5, 0.75], f32)
    m, ds, X, T, before = _case(17, D, policy, 3)
    ens, leaf0, leaf1 = _tree_span(m, 0)
    leaves = np.asarray(m.predict_leaves(X, None, 0, 1)).reshape(-1) - leaf0
    present = np.unique(leaves)
    assert len(present) >= 2 and c % 4 == 0
    a, b = np.array([0x3f800010, 0x3f800011], np.uint32).view(f32)
    assert a < b
    rng = np.random.default_rng(c)
    for per_leaf, n_b in ((c, c // 2), (c + 1, c // 2), (c + 1, c // 2 + 1)):
        rows = rng.permutation(np.concatenate([rng.choice(np.nonzero(leaves == l)[0], per_leaf) for l in present])).astype(np.int32)
        x = np.empty((len(rows), D), f32)
        for l in present:
            at = np.nonzero(leaves[rows] == l)[0]
            assert len(at) == per_leaf
            for d in range(D):
                col = np.full(per_leaf, a, f32)
                col[rng.permutation(per_leaf)[:n_b]] = b
                x[at, d] = col
        want, counts = _check(m, ds, X, np.zeros_like(x), np.ascontiguousarray(-x), D, 0, policy, alpha, rows=rows, select=True)
        k = [cpp.quantile_rank(per_leaf, float(v)) for v in alpha]
        assert k[1] in (n_b, n_b + 1) and k[0] < n_b < k[2]            # the middle rank is the last b or the first a
        expect = np.array([b if kk <= n_b else a for kk in k], f32)
        assert expect[0] == b and expect[2] == a and expect[1] == (b if k[1] == n_b else a)
        for l in present:
            assert counts[l] == per_leaf and want[l].tobytes() == expect.tobytes(), (per_leaf, n_b, l, want[l], expect)


LOOP_SIZES = {   # rows: (count blocks, chunks of block 0, scan slices) -- what _geometry must say, or the sizes no longer reach what they are here for
    2047: (1, 1, 1), 2048: (1, 1, 1), 4097: (3, 1, 1), 6145: (4, 1, 1),
    32768: (16, 1, 1),      # the largest column one scan slice covers: 16 tiles x 256 digits
    32769: (17, 1, 2),      # the scan carries its sum into a second slice
    65535: (32, 1, 2), 65536: (32, 1, 2),   # every count block one chunk
    65537: (32, 2, 3),      # block 0 strides to a second chunk of one row
    131073: (32, 3, 5),     # every block a second full chunk, block 0 a third of one row
}


@pytest.mark.parametrize("n", sorted(LOOP_SIZES))
@pytest.mark.parametrize("name", ["distinct", "shared_prefix_ties"])
def test_row_counts_that_reach_every_loop(name, n):
    D, R = 3, GEO["rows_per_chunk"]
    assert sorted(LOOP_SIZES) == [R - 1, R, 2 * R + 1, 3 * R + 1, 16 * SORT_TILE, 16 * SORT_TILE + 1, MAX_COUNT_BLOCKS * R - 1, MAX_COUNT_BLOCKS * R,
                                  MAX_COUNT_BLOCKS * R + 1, 2 * MAX_COUNT_BLOCKS * R + 1]
    assert _geometry(n) == LOOP_SIZES[n]
    if n >= 65537:
        assert n > MAX_COUNT_BLOCKS * R          # a block of the count pass takes more than one chunk
    if n >= 32769:
        assert n > 16 * SORT_TILE and 256 * 16 == SCAN_SLICE   # the scan makes more than one trip
    m, ds, X, T, before = _case(17, D, "oblivious", 3)
    Xn, ds_n = _bound(m, ds, n, 17)
    pred, targets = Q.family(name, n, D, seed=2)
    if name == "distinct":
        targets = _last_row_decides(targets)
    want, counts = _check(m, ds_n, Xn, pred, targets, D, 0, "oblivious", _levels(D), select=True)
    assert (counts > 0).sum() >= 2 and counts.sum() == n


BIG = 65537   # MAX_COUNT_BLOCKS * rows_per_chunk + 1: the smallest size at which a count block takes a second chunk


def test_a_greedy_tree_of_64_leaves_at_a_second_chunk():
    """the largest tree of the select path (its counters need the LDS opt-in) where block 0 takes two chunks"""
    D = 3
    assert BIG > MAX_COUNT_BLOCKS * GEO["rows_per_chunk"]
    m, ds, X, T, before = _case(17, D, "greedy", 6, n_grow=4000)
    ens, leaf0, leaf1 = _tree_span(m, 0)
    assert leaf1 - leaf0 == GEO["max_select_leaves"] == 64, "the tree has %d leaves" % (leaf1 - leaf0)
    Xn, ds_n = _bound(m, ds, BIG, 17)
    for name in ("distinct", "shared_prefix_ties"):
        pred, targets = Q.family(name, BIG, D, seed=3)
        if name == "distinct":
            targets = _last_row_decides(targets)
        want, counts = _check(m, ds_n, Xn, pred, targets, D, 0, "greedy", _levels(D), select=True)
        assert (counts > 0).sum() > 32


def test_one_output_at_a_second_chunk():
    D = 1
    assert BIG > MAX_COUNT_BLOCKS * GEO["rows_per_chunk"]
    m, ds, X, T, before = _case(17, D, "oblivious", 3)
    Xn, ds_n = _bound(m, ds, BIG, 17)
    for name in ("distinct", "shared_prefix_ties"):
        pred, targets = Q.family(name, BIG, D, seed=4)
        if name == "distinct":
            targets = _last_row_decides(targets)
        _check(m, ds_n, Xn, pred, targets, D, 0, "oblivious", _levels(D), select=True)


def test_rows_from_a_larger_data_set_at_a_second_chunk():
    """rows= draws 65537 positions with duplicates from 70001 rows; then from the rows of every leaf but one: that leaf keeps its value and counts 0"""
    D, n_all = 3, 70001
    assert BIG > MAX_COUNT_BLOCKS * GEO["rows_per_chunk"]
    m, ds, X, T, before = _case(17, D, "oblivious", 3)
    Xall, ds_all = _bound(m, ds, n_all, 17)
    rng = np.random.default_rng(BIG)
    rows = rng.integers(0, n_all, BIG).astype(np.int32)
    assert len(np.unique(rows)) < BIG and rows.max() >= BIG
    pred, targets = Q.family("distinct", BIG, D, seed=5)
    targets = _last_row_decides(targets)
    want, counts = _check(m, ds_all, Xall, pred, targets, D, 0, "oblivious", _levels(D), rows=rows, select=True)
    assert counts.sum() == BIG
    ens, leaf0, leaf1 = _tree_span(m, 0)
    leaves = np.asarray(m.predict_leaves(Xall, None, 0, 1)).reshape(-1) - leaf0
    present = np.unique(leaves)
    assert len(present) >= 2
    gone = int(present[0])
    pool = np.nonzero(leaves != gone)[0]
    rows = pool[rng.integers(0, len(pool), BIG)].astype(np.int32)
    old = np.asarray(ens["values"], f32).reshape(-1, D)[leaf0 + gone].copy()
    pred, targets = Q.family("shared_prefix_ties", BIG, D, seed=6)
    want, counts = _check(m, ds_all, Xall, pred, targets, D, 0, "oblivious", _levels(D), rows=rows, select=True)
    assert counts[gone] == 0 and counts.sum() == BIG and want[gone].tobytes() == old.tobytes()


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_the_widest_model(policy):
    D, n = 128, 2049
    m, ds, X, T, before = _case(16, D, policy, 3)
    Xn, ds_n = _bound(m, ds, n, 16)
    pred, targets = Q.family("distinct", n, D, seed=7)
    want, counts = _check(m, ds_n, Xn, pred, targets, D, 0, policy, _levels(D), select=True)
    assert (counts > 0).sum() >= 2
    pred, targets = Q.family("shared_prefix_ties", n, D, seed=7)
    _check(m, ds_n, Xn, pred, targets, D, 0, policy, _levels(D), select=True)


@pytest.mark.parametrize("generic", ["0", "1"])
def test_one_output_more_than_the_widest_is_refused(generic, tmp_path):
    D, n = 129, 65
    m = _model(16, D, "oblivious", 3)
    X = np.random.default_rng(D).standard_normal((n, 16)).astype(f32)
    ds = m.prepare_dataset(X)
    keep = _file(m, tmp_path)
    pred, targets = Q.family("distinct", n, D, seed=8)
    with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
        with pytest.raises(RuntimeError, match="output_dim"):
            m.quantile_leaves_prepared(ds, pred, targets, _levels(D))
    assert _file(m, tmp_path) == keep


def test_a_tree_of_more_than_255_leaves():
    """the leaf ids need a second byte: the sort by id makes two passes (lq_id_passes).  Depth 9 on 4000 rows is the smallest of the grids
    depth {9, 10} x rows {4000, 8000, 20000} and reaches 380 leaves"""
    D, n = 3, 4000
    m, ds, X, T, before = _case(8, D, "greedy", 9, n_grow=n)
    ens, leaf0, leaf1 = _tree_span(m, 0)
    assert leaf1 - leaf0 >= 256, "the tree has %d leaves: the sort by leaf id would make one pass" % (leaf1 - leaf0)
    pred, targets = Q.family("distinct", n, D, seed=9)
    want, counts = _check(m, ds, X, pred, targets, D, 0, "greedy", _levels(D), select=False)
    assert (counts[256:] > 0).any() and (counts[:256] > 0).any()
    sub = np.random.default_rng(9).permutation(n)[:700].astype(np.int32)   # many leaves without a row
    pred, targets = Q.family("shared_prefix_ties", 700, D, seed=9)
    want, counts = _check(m, ds, X, pred, targets, D, 0, "greedy", _levels(D), rows=sub, select=False)
    assert (counts == 0).any() and (counts[256:] > 0).any()


@pytest.mark.parametrize("n,D", [(1, 1), (65, 3), (200, 8), (257, 65)])
def test_objective_gradient_and_loss(n, D):
    """the device gradient is the host's bytes; the loss is the float64 mean pinball loss within (n D + 8) 2^-52, the bound of a sum of n D
    non-negative terms in any order that tests/test_gpu_objective.py uses for the logistic loss"""
    rng = np.random.default_rng(n * 131 + D)
    m = _model(4, D, "oblivious", 3)
    a = _levels(D) if D > 1 else np.array([0.3], f32)
    P = rng.standard_normal((n, D)).astype(f32)
    Y = np.where(rng.random((n, D)) < 0.2, P, _targets(rng, n, D)).astype(f32)
    g, loss = m.objective_gradient(_shape(P, D), _shape(Y, D), "quantile", alpha=a)
    want = cpp.objective_gradient_host(_shape(P, D), _shape(Y, D), "quantile", alpha=a)
    assert g.dtype == f32 and g.tobytes() == want.tobytes() and isinstance(loss, float)
    g2, loss2 = m.objective_gradient(_shape(P, D), _shape(Y, D), "quantile", alpha=a)
    assert g2.tobytes() == g.tobytes() and np.float64(loss2).tobytes() == np.float64(loss).tobytes()
    u = Y.astype(np.float64) - P.astype(np.float64)
    terms = np.where(u >= 0, a.astype(np.float64) * u, (a.astype(np.float64) - 1.0) * u)
    ref = math.fsum(terms.ravel().tolist()) / n
    print("n=%d D=%d: loss %.17g reference %.17g bound %.3g" % (n, D, loss, ref, (n * D + 8) * 2.0 ** -52 * abs(ref)))
    assert abs(loss - ref) <= (n * D + 8) * 2.0 ** -52 * abs(ref)
    with pytest.raises(RuntimeError, match="needs alpha"):
        m.objective_gradient(_shape(P, D), _shape(Y, D), "quantile")
    with pytest.raises(RuntimeError, match="alpha"):
        m.objective_gradient(_shape(P, D), _shape(Y, D), "rmse", alpha=a)
    with pytest.raises(RuntimeError, match="weights"):
        m.objective_gradient(_shape(P, D), _shape(Y, D), "quantile", weights=np.ones(n, f32), alpha=a)
