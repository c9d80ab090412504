"""`refit_leaves` (include/gbrl_hip.h): the leaf values of a tree range fitted again on a batch, the structure kept.  Every comparison is EXACT.

The oracle uses only what other files already test: `predict_leaves` for the routing, `predict_continue` on the refitted model to advance the
running prediction one tree at a time, and NumPy integers for the sums.  Per tree t of the range it restates the contract:

  g = P - Y in float32;  lbits = min(60, floor(log2(4.0e18 / (n * max|g|))) - 1), 40 when max|g| == 0 (the step's rule for its leaf sums)
  q = rint((double)g * 2^lbits) as int64;  S[leaf] += q, cnt[leaf] += 1 over the rows whose leaf lies inside the tree
  mean = ((double)S / 2^lbits) / cnt;  value = float32(mean), or float32(decay * (double)old + (1 - decay) * mean) (two products, one sum)
  a leaf without rows and a leaf of depth 0 keep their bits

Every case refits four fresh clones of the same model -- the default path twice, GBRL_HIP_REFIT_GENERIC=1 twice -- and the four results must
have the same bytes, the returned loss included; the loss must be what `staged_loss(..., stops=[stop])` returns right after.  The trees are
grown as in test_gpu_leaves.py: 256 .. 384-row steps at n_bins = 32.
"""
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKENS = np.array(["tok%d" % i for i in range(6)], dtype="S128")
BATCHES = (1, 63, 64, 65, 200, 64 * 37 + 5)     # the last: 38 tiles, several blocks flush into the same accumulators
OPTS = {   # optimizers by name (start_idx / stop_idx default to every output)
    "const": [dict(algo="SGD", scheduler="Const", init_lr=0.1)],
    "const_0.125": [dict(algo="SGD", scheduler="Const", init_lr=0.125)],
    "linear": [dict(algo="SGD", scheduler="Linear", init_lr=0.1, stop_lr=0.01, T=50)],
    "two_and_an_orphan": [dict(algo="SGD", scheduler="Const", init_lr=0.125, start_idx=0, stop_idx=2),
                          dict(algo="SGD", scheduler="Linear", init_lr=0.1, stop_lr=0.01, T=50, start_idx=2, stop_idx=3)],
}


def _model(F, Fc, D, depth, policy="oblivious", opts="const", name="refit", min_data_in_leaf=0):
    import gbrl_amd
    m = gbrl_amd.GBRL(input_dim=F + Fc, output_dim=D, policy_dim=D, max_depth=depth, min_data_in_leaf=min_data_in_leaf, n_bins=32, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy=policy,
                      verbose=0, device="cpu", learner_name=name)
    m.set_feature_weights(np.ones(F + Fc, np.float32))
    for o in OPTS[opts]:
        m.set_optimizer(**dict(dict(start_idx=0, stop_idx=D), **o))
    m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))
    m.set_bias(np.asarray(0.25 + 0.5 * np.arange(D), np.float32))
    return m


def _batch(rng, n, F, Fc):
    X = rng.standard_normal((n, F)).astype(np.float32) if F else None
    Xc = TOKENS[rng.integers(0, 6, (n, Fc))] if Fc else None
    return X, Xc


def _targets(rng, X, Xc, D):
    n = (X if X is not None else Xc).shape[0]
    Y = rng.standard_normal((n, D)).astype(np.float32)
    if X is not None:
        Y[:, 0] += 1.5 * X[:, 0] - X[:, -1]
    if Xc is not None:
        Y[:, -1] += (Xc[:, 0] == TOKENS[1]) * 2.0
    return np.ascontiguousarray(Y)


def _grow(m, rng, trees, F, Fc, D, rows=384):
    for _ in range(trees):
        X, Xc = _batch(rng, rows, F, Fc)
        G = rng.standard_normal((rows, D)).astype(np.float32)
        if F:
            G[:, 0] += X[:, 0] * 2.0
        if Fc:
            G[:, -1] += (Xc[:, 0] == TOKENS[1]) * 3.0
        m.step(X, Xc, np.ascontiguousarray(G.astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _grown(F, Fc, D, depth, policy, T, opts="const", rows=384):
    """A model with T trees, grown once per shape and never modified: every refit below works on a clone."""
    rng = np.random.default_rng(1000 * F + 100 * Fc + 10 * T + D + depth + (7 if policy == "greedy" else 0))
    m = _model(F, Fc, D, depth, policy, opts)
    _grow(m, rng, T, F, Fc, D, rows)
    assert m.get_num_trees() == T
    return m


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _values(m):
    return np.ascontiguousarray(np.asarray(m.get_ensemble_data()["values"], np.float32).reshape(-1, np.asarray(m.get_bias()).size))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _base(m, n):
    bias = np.asarray(m.get_bias(), np.float32).reshape(-1)
    return np.ascontiguousarray(np.tile(bias, (n, 1))) if bias.size > 1 else np.full(n, bias[0], np.float32)


def _refit_four(m0, X, Xc, Y, a=0, b=0, decay=0.0):
    """Four fresh clones of m0 refitted: default and GBRL_HIP_REFIT_GENERIC=1, twice each.  The same value bytes and the same loss bits; the
    loss is staged_loss's right after.  Returns (one refitted clone, its loss)."""
    import gbrl_amd
    stop = b if b else m0.get_num_trees()
    got = []
    for generic in ("0", "1", "0", "1"):
        c = gbrl_amd.GBRL(m0)
        with _env("GBRL_HIP_REFIT_GENERIC", generic):
            loss = c.refit_leaves(X, Xc, Y, a, b, decay)
        assert isinstance(loss, float)
        after = float(np.asarray(c.staged_loss(X, Xc, Y, stops=[stop]))[0])
        assert np.float64(loss).tobytes() == np.float64(after).tobytes(), (generic, loss, after)
        got.append((c, _values(c).tobytes(), np.float64(loss).tobytes()))
    for g in got[1:]:
        assert g[1] == got[0][1] and g[2] == got[0][2], "streaming / general / repeated refits differ"
    return got[0][0], np.frombuffer(got[0][2], np.float64)[0]


def _lbits(n, gmax):
    gmax = float(gmax)
    if not (0.0 < gmax < math.inf):
        return 40
    return min(60, (math.frexp(4.0e18 / (float(n) * gmax))[1] - 1) - 1)


def _oracle(m0, mr, X, Xc, Y, a, stop, decay):
    """Expected `values` [n_leaves, D] of the refit of m0's trees [a, stop); mr is the refitted model (its predict_continue advances P)."""
    e = m0.get_ensemble_data()
    ti = np.asarray(e["tree_indices"]); dep = np.asarray(e["depths"])
    old = _values(m0)
    L, D = old.shape
    n = Y.shape[0]
    oblivious = len(dep) == len(ti)
    leaves = np.asarray(m0.predict_leaves(X, Xc, a, stop))
    P = _base(m0, n)
    if a > 0:
        P = np.asarray(m0.predict_continue(X, Xc, P, 0, a))
    want = old.copy()
    for t in range(a, stop):
        g = (P.reshape(n, D) - Y.reshape(n, D)).astype(np.float32)
        assert g.dtype == np.float32
        gmax = np.abs(g).max()
        lb = _lbits(n, gmax)
        q = np.rint(g.astype(np.float64) * 2.0 ** lb).astype(np.int64)
        l0, l1 = int(ti[t]), (int(ti[t + 1]) if t + 1 < len(ti) else L)
        leaf = leaves[:, t - a].astype(np.int64)
        inside = (leaf >= l0) & (leaf < l1)
        S = np.zeros((L, D), np.int64)
        np.add.at(S, leaf[inside], q[inside])
        cnt = np.bincount(leaf[inside], minlength=L)
        for l in range(l0, l1):
            depth = int(dep[t]) if oblivious else int(dep[l])
            if cnt[l] == 0 or depth == 0:
                continue
            mean = (S[l].astype(np.float64) / 2.0 ** lb) / np.float64(cnt[l])
            if decay == 0.0:
                want[l] = mean.astype(np.float32)
            else:
                want[l] = (np.float64(decay) * old[l].astype(np.float64) + (1.0 - decay) * mean).astype(np.float32)
        P = np.asarray(mr.predict_continue(X, Xc, P, t, t + 1))
    return want, P


def _check(m0, X, Xc, Y, a=0, b=0, decay=0.0):
    T = m0.get_num_trees()
    stop = b if b else T
    before = m0.get_ensemble_data()
    mr, loss = _refit_four(m0, X, Xc, Y, a, b, decay)
    want, P = _oracle(m0, mr, X, Xc, Y, a, stop, decay)
    got = _values(mr)
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want)), "refitted values differ from the oracle at %s" % np.argwhere(_bits(got) != _bits(want))[:5].tolist()
    # only `values` of the range has changed
    after = mr.get_ensemble_data()
    for k in before:
        if k != "values":
            assert np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes(), k
    ti = np.asarray(before["tree_indices"])
    outside = np.ones(want.shape[0], bool)
    outside[ti[a]:(ti[stop] if stop < T else want.shape[0])] = False
    assert np.array_equal(_bits(got[outside]), _bits(_values(m0)[outside]))
    assert mr.get_num_trees() == T and mr.get_iteration() == m0.get_iteration()
    assert np.asarray(mr.get_bias()).tobytes() == np.asarray(m0.get_bias()).tobytes()
    # the loss is MultiRMSE of the final running prediction
    g = (P.reshape(Y.shape[0], -1) - Y.reshape(Y.shape[0], -1)).astype(np.float32).astype(np.float64)
    # (two float64 sums of the same g.size non-negative terms in different orders: each within g.size * 2^-53 of the exact sum, relative)
    assert abs(loss - math.sqrt(0.5 * float((g * g).sum()) / Y.shape[0])) <= 2.0 * g.size * 2.0 ** -53 * loss
    return mr, got, loss


# ---- 1. routing, staging and flush -------------------------------------------------------------------------------------------------------
# F = 5 stages the tile with scalar loads, F = 8 with 16-byte loads; depth 1 and 2 (2 and 4 leaves) take the in-wave reduction, depth 4 the LDS
# atomics; D = 1, 3 read the rows with scalar loads, D = 8 with 16-byte loads
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("F,T,D,depth", [(5, 19, 1, 4), (8, 5, 3, 2), (8, 19, 8, 1), (5, 5, 8, 4), (8, 5, 1, 1), (5, 19, 3, 2)])
def test_against_the_oracle(policy, F, T, D, depth):
    m0 = _grown(F, 0, D, depth, policy, T)
    rng = np.random.default_rng(17 * F + T + D + depth)
    for n in BATCHES:
        X, _ = _batch(rng, n, F, 0)
        Y = _targets(rng, X, None, D)
        _, got, _ = _check(m0, X, None, Y if D > 1 or n % 2 else Y.reshape(n))
        if n >= 200:
            assert not np.array_equal(_bits(got), _bits(_values(m0))), "the refit changed nothing"


# ---- 2. categorical columns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_categorical_columns_raw_cells_and_device_cells(policy):
    import torch
    F, Fc, D, T = 3, 2, 2, 9
    m0 = _grown(F, Fc, D, 4, policy, T)
    assert (np.asarray(m0.get_ensemble_data()["is_numerics"]) == 0).any(), "no categorical condition was grown"
    rng = np.random.default_rng(23)
    dev = torch.device("cuda:0")
    for n in (65, 200):
        X, Xc = _batch(rng, n, F, Fc)
        Y = _targets(rng, X, Xc, D)
        _, raw, loss = _check(m0, X, Xc, Y)
        cells = torch.from_numpy(np.frombuffer(Xc.tobytes(), np.uint8).reshape(n, Fc, 128).copy()).to(dev)
        on_dev, loss_dev = _refit_four(m0, X, (cells.data_ptr(), (n, Fc), "S128", "cuda"), Y)
        assert _values(on_dev).tobytes() == raw.tobytes() and loss_dev == loss


# ---- 3. arguments and schedules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_ranges_and_decay_rates(policy):
    F, D, T = 8, 3, 7
    m0 = _grown(F, 0, D, 3, policy, T)
    rng = np.random.default_rng(31)
    X, _ = _batch(rng, 200, F, 0)
    Y = _targets(rng, X, None, D)
    for (a, b), decay in (((0, 0), 0.5), ((2, 5), 0.0), ((2, 5), 0.3), ((T - 1, T), 0.5), ((3, 0), 0.3), ((0, 1), 0.0), ((0, T), 1.0)):
        _, got, _ = _check(m0, X, None, Y, a, b, decay)
        if decay == 1.0:
            assert got.tobytes() == _values(m0).tobytes()      # 1 * v + 0 * mean: every value keeps its bits


@pytest.mark.parametrize("opts", ["const_0.125", "const", "linear"])
def test_learning_rates(opts):
    F, D, T = 8, 3, 6
    rng = np.random.default_rng(37)
    X, _ = _batch(rng, 200, F, 0)
    Y = _targets(rng, X, None, D)
    for policy in ("oblivious", "greedy"):
        m0 = _grown(F, 0, D, 3, policy, T, opts)
        _check(m0, X, None, Y)
        _check(m0, X, None, Y, 2, 5, 0.3)


def test_two_optimizers_and_an_output_nobody_owns():
    F, D, T, n = 8, 4, 6, 200
    rng = np.random.default_rng(41)
    X, _ = _batch(rng, n, F, 0)
    Y = _targets(rng, X, None, D)
    for policy in ("oblivious", "greedy"):
        m0 = _grown(F, 0, D, 3, policy, T, "two_and_an_orphan")
        mr, got, _ = _check(m0, X, None, Y)
        # output 3 has no optimizer: its P never moves, so every tree stores the leaf means of bias - y
        bias = np.asarray(m0.get_bias(), np.float32)
        assert np.asarray(mr.predict(X, None))[:, 3].tobytes() == np.full(n, bias[3], np.float32).tobytes()
        g3 = (np.full(n, bias[3], np.float32) - Y[:, 3]).astype(np.float32)
        leaves = np.asarray(mr.predict_leaves(X, None))
        for t in range(T):
            for l in np.unique(leaves[:, t]):
                rows = leaves[:, t] == l
                mean = float(g3[rows].astype(np.float64).sum()) / int(rows.sum())
                # float32 rounding of the mean (2^-24 relative) and the fixed point's 2^-lbits per row, lbits > 40 here; the exact bits are
                # the oracle's, above
                assert abs(float(got[l, 3]) - mean) <= 2e-7 * max(1.0, abs(mean)), (t, l)


# ---- 4. empty leaves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_leaves_without_rows_keep_their_bits(policy):
    F, D, T = 8, 3, 6
    m0 = _grown(F, 0, D, 3, policy, T)
    rng = np.random.default_rng(43)
    X = (np.abs(rng.standard_normal((200, F))) + 4.0).astype(np.float32)     # beyond every threshold: one side of every split
    Y = _targets(rng, X, None, D)
    counts = np.asarray(m0.leaf_counts(X, None))
    assert (counts == 0).any() and (counts > 0).any()
    for decay in (0.0, 0.5):
        _, got, _ = _check(m0, X, None, Y, 0, 0, decay)
        old = _values(m0)
        assert np.array_equal(_bits(got[counts == 0]), _bits(old[counts == 0]))
        assert not np.array_equal(_bits(got[counts > 0]), _bits(old[counts > 0]))


def _with_a_stump(policy, D=2):
    """[full, full, depth 0, full, full]: min_data_in_leaf = 60 and one step of 100 rows, where no candidate survives (test_gpu_edges.py)."""
    F = 8
    rng = np.random.default_rng(97 if policy == "greedy" else 98)
    m = _model(F, 0, D, 3, policy, min_data_in_leaf=60)
    for rows in (300, 300, 100, 300, 300):
        X, _ = _batch(rng, rows, F, 0)
        G = rng.standard_normal((rows, D)).astype(np.float32)
        G[:, 0] += X[:, 0] * 2.0
        m.step(X, None, np.ascontiguousarray(G))
    e = m.get_ensemble_data()
    ti, dep = np.asarray(e["tree_indices"]), np.asarray(e["depths"])
    assert m.get_num_trees() == 5
    leaves = np.diff(np.append(ti, np.asarray(e["values"]).shape[0]))
    assert leaves.tolist()[2] == 1 and min(leaves.tolist()[:2] + leaves.tolist()[3:]) >= 2, "expected [full, full, stump, full, full], got %s leaves" % leaves.tolist()
    assert (dep[2] if policy == "oblivious" else dep[ti[2]]) == 0
    return m, int(ti[2])


def test_an_oblivious_tree_of_depth_0_keeps_its_value():
    """A stump between full trees: every row reaches its one leaf, the leaf keeps its bits (cnt > 0 does not matter at depth 0), P is advanced
    with the kept value as predict_continue does, the other trees match the oracle and the loss is staged_loss's."""
    m0, stump_leaf = _with_a_stump("oblivious")
    rng = np.random.default_rng(5)
    for n in (65, 200):
        X, _ = _batch(rng, n, 8, 0)
        Y = _targets(rng, X, None, 2)
        assert int(np.asarray(m0.leaf_counts(X, None))[stump_leaf]) == n
        for (a, b), decay in (((0, 0), 0.0), ((0, 0), 0.3), ((2, 3), 0.0), ((1, 4), 0.5), ((3, 5), 0.0)):
            _, got, _ = _check(m0, X, None, Y, a, b, decay)
            assert np.array_equal(_bits(got[stump_leaf]), _bits(_values(m0)[stump_leaf]))
            if (a, b) != (2, 3):
                assert not np.array_equal(_bits(got), _bits(_values(m0)))


def test_a_greedy_tree_of_depth_0_in_or_right_before_the_range_is_refused():
    """A greedy leaf of depth 0 never passes: predict_continue applies a leaf of the NEXT tree at the stump's rate there, a value the refit does
    not know yet.  A range that holds the stump, or starts right behind it, is refused (unsupported) and changes nothing; the ranges in front of
    it and further behind it are refitted and match the oracle, whose running prediction walks through the stump like every predict call."""
    import gbrl_amd
    m0, stump_leaf = _with_a_stump("greedy")
    rng = np.random.default_rng(6)
    X, _ = _batch(rng, 200, 8, 0)
    Y = _targets(rng, X, None, 2)
    c = gbrl_amd.GBRL(m0)
    before = np.asarray(c.predict(X, None)).tobytes()
    for a, b in ((0, 0), (0, 3), (2, 3), (1, 4), (3, 5), (3, 4)):
        with pytest.raises(RuntimeError, match="depth 0"):
            c.refit_leaves(X, None, Y, a, b)
        assert _values(c).tobytes() == _values(m0).tobytes() and np.asarray(c.predict(X, None)).tobytes() == before
    for a, b in ((0, 2), (1, 2), (4, 5)):
        _, got, _ = _check(m0, X, None, Y, a, b, 0.3)
        assert not np.array_equal(_bits(got), _bits(_values(m0)))


def test_the_streaming_kernel_takes_the_shapes_it_is_meant_for():
    """`last_phase_times()["refit_streamed_trees"]` (profiling on) counts the trees whose sums k_refit_accum took: all of them by default, none
    under GBRL_HIP_REFIT_GENERIC=1 or when the rows are too wide for the LDS tile."""
    import gbrl_amd
    rng = np.random.default_rng(7)
    for policy in ("oblivious", "greedy"):
        for F, D, depth, T, rows, want in ((8, 8, 4, 5, 384, 5), (8, 3, 1, 5, 384, 5), (640, 2, 3, 5, 256, 0)):
            m0 = _grown(F, 0, D, depth, policy, T, "const", rows)
            X, _ = _batch(rng, 200, F, 0)
            Y = _targets(rng, X, None, D)
            for generic, expect in (("0", want), ("1", 0)):
                c = gbrl_amd.GBRL(m0)
                c.set_profiling(1)
                with _env("GBRL_HIP_REFIT_GENERIC", generic):
                    c.refit_leaves(X, None, Y)
                assert int(c.last_phase_times()["refit_streamed_trees"]) == expect, (policy, F, D, depth, generic)


def test_trees_grown_on_gradients_constant_in_x():
    """Gradients that are constant in X: at these settings (256 rows, F = 8, max_depth = 3, n_bins = 32, all-ones and all-zero gradients) the
    grower emits full-depth trees under both policies (see test_gpu_leaves.py), not stumps -- the depth-0 cases are the two tests above.  The
    trees it does grow from such gradients are refitted against the oracle like any others."""
    F, D = 8, 2
    rng = np.random.default_rng(95)
    for policy in ("oblivious", "greedy"):
        m = _model(F, 0, D, 3, policy)
        X, _ = _batch(rng, 256, F, 0)
        m.step(X, None, rng.standard_normal((256, D)).astype(np.float32))
        m.step(X, None, np.ones((256, D), np.float32))
        m.step(X, None, np.zeros((256, D), np.float32))
        Y = _targets(rng, X[:65], None, D)
        for a, b in ((0, 0), (1, 3)):
            _check(m, X[:65], None, Y, a, b)


# ---- 5. identity: refit stores what fit would have stored ----------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("D", [1, 3])
def test_refit_on_the_fitted_data_changes_nothing(policy, D):
    """fit() with one batch that holds the whole data set, unshuffled: tree t was grown on g = predict([0, t)) - y over exactly these rows, and
    its leaves hold the means of that g.  refit_leaves on the same data with decay_rate = 0 recomputes every one of them: the same bits."""
    F, n, T = 8, 300, 4
    rng = np.random.default_rng(53 + D)
    m = _model(F, 0, D, 3, policy)
    X, _ = _batch(rng, n, F, 0)
    Y = _targets(rng, X, None, D)
    m.fit(X, None, Y, T, shuffle=False)
    assert m.get_num_trees() == T
    old = _values(m)
    staged = np.asarray(m.staged_loss(X, None, Y))
    mr, loss = _refit_four(m, X, None, Y)
    assert np.array_equal(_bits(_values(mr)), _bits(old)), "refit on the fitted data moved %d values" % int((_bits(_values(mr)) != _bits(old)).sum())
    assert np.float64(loss).tobytes() == np.float64(staged[-1]).tobytes()


# ---- 7. no stale mirror ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("n", [64, 4096])
def test_every_predict_route_sees_the_new_values(policy, n, tmp_path):
    import gbrl_amd
    import cases as K
    F, Fc, D, T = 3, 2, 2, 9
    m = gbrl_amd.GBRL(_grown(F, Fc, D, 4, policy, T))
    rng = np.random.default_rng(61 + n)
    X, Xc = _batch(rng, n, F, Fc)
    Y = _targets(rng, X, Xc, D)
    base_poly, norm, offset = (np.ascontiguousarray(v, np.float32) for v in K.poly_vectors(4))
    before = np.asarray(m.predict(X, Xc)).copy()               # a mirror exists, and can go stale
    ids, token = m.encode_categorical(Xc)
    ids = np.asarray(ids).copy()
    m.ensemble_shap(X[:64], Xc[:64], norm, base_poly, offset)
    m.refit_leaves(X, Xc, Y, 2, 8, 0.3)
    _, token_after = m.encode_categorical(Xc[:8])
    assert token_after == token
    p = tmp_path / "refitted.gbrl_model"
    assert m.save(str(p)) == 0
    fresh = gbrl_amd.GBRL.load(str(p))
    assert _values(fresh).tobytes() == _values(m).tobytes()
    base = _base(m, n)
    stops = [0, 3, 8, T]
    for call in (lambda g: g.predict(X, Xc), lambda g: g.predict(X, Xc, 1, 7), lambda g: g.predict_continue(X, Xc, base, 0, T),
                 lambda g: g.predict_staged(X, Xc, stops), lambda g: g.ensemble_shap(X[:64], Xc[:64], norm, base_poly, offset)):
        assert np.asarray(call(m)).tobytes() == np.asarray(call(fresh)).tobytes()
    after = np.asarray(m.predict(X, Xc))
    assert after.tobytes() != before.tobytes()
    assert np.asarray(m.predict_encoded(X, ids, token)).tobytes() == after.tobytes()      # ids encoded before the refit still serve
    clone = gbrl_amd.GBRL(m)
    assert _values(clone).tobytes() == _values(m).tobytes()
    assert np.asarray(clone.predict(X, Xc)).tobytes() == after.tobytes()


# ---- 8. width fallback -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_fallback_rows_too_wide_for_the_lds_tile(policy):
    """F = 640: the 64-row tile would be 160 KiB, so the accumulate pass runs the one-thread-per-row kernel on rows in global memory."""
    F, D, T, n = 640, 2, 5, 65
    m0 = _grown(F, 0, D, 3, policy, T, "const", 256)
    rng = np.random.default_rng(81)
    X, _ = _batch(rng, n, F, 0)
    _check(m0, X, None, _targets(rng, X, None, D))


# ---- 9. failure leaves no trace ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_a_nan_target_is_refused_and_nothing_changes(policy):
    import gbrl_amd
    F, D, T, n = 8, 3, 6, 200
    m = gbrl_amd.GBRL(_grown(F, 0, D, 3, policy, T))
    rng = np.random.default_rng(71)
    X, _ = _batch(rng, n, F, 0)
    Y = _targets(rng, X, None, D)
    before_values = _values(m).tobytes()
    before_pred = np.asarray(m.predict(X, None)).tobytes()
    for bad in (np.nan, np.inf):
        Yb = Y.copy()
        Yb[137, 1] = bad
        for generic in ("0", "1"):
            with _env("GBRL_HIP_REFIT_GENERIC", generic):
                with pytest.raises(RuntimeError, match="not finite"):
                    m.refit_leaves(X, None, Yb, 1, 5, 0.5)
            assert _values(m).tobytes() == before_values
            assert np.asarray(m.predict(X, None)).tobytes() == before_pred
    # and the model still refits
    m.refit_leaves(X, None, Y)
    assert _values(m).tobytes() != before_values


# ---- 10. device-resident inputs ------------------------------------------------------------------------------------------------------------------
def test_a_cuda_model_with_device_tuples():
    import gbrl_amd
    import torch
    F, D, T, n = 8, 3, 6, 200
    m0 = _grown(F, 0, D, 3, "oblivious", T)
    rng = np.random.default_rng(91)
    X, _ = _batch(rng, n, F, 0)
    Y = _targets(rng, X, None, D)
    ref, want_loss = _refit_four(m0, X, None, Y, 1, 0, 0.3)
    dev = torch.device("cuda:0")
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    c = gbrl_amd.GBRL(m0)
    c.to_device("cuda")
    try:
        loss = c.refit_leaves((Xd.data_ptr(), (n, F), "torch.float32", "cuda"), None, (Yd.data_ptr(), (n, D), "torch.float32", "cuda"), 1, 0, 0.3)
    finally:
        c.to_device("cpu")
    assert isinstance(loss, float) and loss == want_loss
    assert _values(c).tobytes() == _values(ref).tobytes()
