"""`predict_leaves` / `leaf_counts` and their `_encoded` variants (include/gbrl_hip.h): where a row lands.  Leaf routing is integer, so every
comparison here is EXACT.  The yardstick is a NumPy walk of `get_ensemble_data()` that restates the two definitions of the contract:

  oblivious  leaf = tree_indices[t] + sum_d pass(cond[t, d]) << (depths[t] - 1 - d); pass = x[f] > threshold, or cell == category
  greedy     the first leaf in storage order from tree_indices[t] on whose conditions all hold, each against its inequality direction; a leaf
             of depth 0 never passes (predictor.cpp:208-228: `passed` starts false and the loop over its conditions is empty), and a search
             that runs off the ensemble gives -1

Every case runs the default path (the streaming kernels k_leaves / k_leaf_counts where they take the shape) and GBRL_HIP_LEAVES_GENERIC=1
(k_leaves_general / k_leaf_counts_general), twice each: all four results must have the same bytes.  The trees are grown on 256 .. 384-row steps
at n_bins = 32, each step on fresh gradients so that the trees differ.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKENS = np.array(["tok%d" % i for i in range(6)], dtype="S128")
KG = 16          # trees per group of k_leaves (predict_leaves.hip: kLeavesG)
BATCHES = (1, 63, 64, 65, 200)


def _model(F, Fc, D, depth, policy="oblivious", lr=0.1, name="leaves", min_data_in_leaf=0):
    import gbrl_amd
    m = gbrl_amd.GBRL(input_dim=F + Fc, output_dim=D, policy_dim=D, max_depth=depth, min_data_in_leaf=min_data_in_leaf, n_bins=32, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy=policy,
                      verbose=0, device="cpu", learner_name=name)
    m.set_feature_weights(np.ones(F + Fc, np.float32))
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=lr, start_idx=0, stop_idx=D)
    m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))
    m.set_bias(np.asarray(0.25 + 0.5 * np.arange(D), np.float32))
    return m


def _batch(rng, n, F, Fc, n_tokens=6):
    X = rng.standard_normal((n, F)).astype(np.float32) if F else None
    Xc = TOKENS[rng.integers(0, n_tokens, (n, Fc))] if Fc else None
    return X, Xc


def _grow(m, rng, trees, F, Fc, D, rows=384):
    for _ in range(trees):
        X, Xc = _batch(rng, rows, F, Fc)
        G = rng.standard_normal((rows, D)).astype(np.float32)
        if F:
            G[:, 0] += X[:, 0] * 2.0
        if Fc:
            G[:, -1] += (Xc[:, 0] == TOKENS[1]) * 3.0
        m.step(X, Xc, np.ascontiguousarray(G.astype(np.float32)))


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _np_leaves(e, policy, X, Xc, start, stop):
    """The two definitions of the contract, restated: int32 [n, stop - start] global leaf indices."""
    ti = np.asarray(e["tree_indices"]); dep = np.asarray(e["depths"]); fi = np.asarray(e["feature_indices"])
    fv = np.asarray(e["feature_values"]); isn = np.asarray(e["is_numerics"]); cv = np.asarray(e["categorical_values"])
    ineq = np.asarray(e["inequality_directions"]); n_leaves = np.asarray(e["values"]).shape[0]
    n = (X if X is not None else Xc).shape[0]

    def test(s, d):   # condition d of split row s (a tree when oblivious, a leaf when greedy), for every row
        return (X[:, fi[s, d]] > fv[s, d]) if isn[s, d] else (Xc[:, fi[s, d]] == cv[s, d])

    out = np.empty((n, stop - start), np.int32)
    for t in range(start, stop):
        if policy == "oblivious":
            leaf = np.full(n, int(ti[t]), np.int64)
            for d in range(int(dep[t])):
                leaf += test(t, d).astype(np.int64) << (int(dep[t]) - 1 - d)
        else:
            leaf = np.full(n, -1, np.int64)
            for l in range(int(ti[t]), n_leaves):
                if not (leaf < 0).any():
                    break
                passed = np.zeros(n, bool) if dep[l] == 0 else np.ones(n, bool)
                for d in range(int(dep[l]) - 1, -1, -1):
                    passed &= test(l, d) == bool(ineq[l, d])
                leaf[(leaf < 0) & passed] = l
        out[:, t - start] = leaf
    return out


def _four(call):
    """default and GBRL_HIP_LEAVES_GENERIC=1, twice each: the same bytes; returns one of them."""
    got = []
    for generic in ("0", "1", "0", "1"):
        with _env("GBRL_HIP_LEAVES_GENERIC", generic):
            got.append(np.asarray(call()))
    for g in got[1:]:
        assert g.dtype == got[0].dtype and g.shape == got[0].shape and g.tobytes() == got[0].tobytes(), "streaming / general / repeated calls differ"
    return got[0]


def _check(m, e, policy, X, Xc, a, b, encoded=None):
    """predict_leaves == the NumPy walk, leaf_counts == its bincount, over [a, b) (b == 0: all trees)."""
    T = m.get_num_trees()
    n = (X if X is not None else Xc).shape[0]
    n_leaves = np.asarray(e["values"]).shape[0]
    if encoded is None:
        leaves = _four(lambda: m.predict_leaves(X, Xc, a, b))
        counts = _four(lambda: m.leaf_counts(X, Xc, a, b))
    else:
        leaves = _four(lambda: m.predict_leaves_encoded(X, encoded[0], encoded[1], a, b))
        counts = _four(lambda: m.leaf_counts_encoded(X, encoded[0], encoded[1], a, b))
    stop = b if b else T
    want = _np_leaves(e, policy, X, Xc, a, stop)
    assert leaves.dtype == np.int32 and leaves.shape == (n, stop - a)
    assert np.array_equal(leaves, want), "leaves differ from the NumPy walk at %s" % np.argwhere(leaves != want)[:5].tolist()
    assert counts.dtype == np.int64 and counts.shape == (n_leaves,)
    assert np.array_equal(counts, np.bincount(want[want >= 0].ravel(), minlength=n_leaves).astype(np.int64))
    return leaves, counts


def _per_tree_sums(e, counts, a, b):
    ti = np.asarray(e["tree_indices"]); n_leaves = counts.shape[0]
    ends = np.append(ti[1:], n_leaves)
    return [int(counts[ti[t]:ends[t]].sum()) for t in range(a, b)]


# (F, T, D, depth): F = 5 stages the tile with scalar loads, F = 8 with 16-byte loads; T = 19 is no multiple of the group of 16 trees (and no
# multiple of 4: scalar index stores), T = 16 is (16-byte index stores); D must not matter
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("F,T,D,depth", [(5, 19, 1, 4), (8, 16, 3, 3), (8, 19, 1, 1), (5, 16, 3, 2)])
def test_against_a_numpy_walk(policy, F, T, D, depth):
    assert (T % KG != 0) == (T == 19)
    rng = np.random.default_rng(1000 * F + 10 * T + D + (7 if policy == "greedy" else 0))
    m = _model(F, 0, D, depth, policy)
    _grow(m, rng, T, F, 0, D)
    assert m.get_num_trees() == T
    e = m.get_ensemble_data()
    n_leaves = np.asarray(e["values"]).shape[0]
    for n in BATCHES:
        X, _ = _batch(rng, n, F, 0)
        for a, b in ((0, 1), (3, 11), (T - 1, T), (0, T), (0, 0)):
            leaves, counts = _check(m, e, policy, X, None, a, b)
            stop = b if b else T
            assert leaves.min() >= 0
            assert _per_tree_sums(e, counts, a, stop) == [n] * (stop - a)       # every tree of the range routes every row
            ti = np.asarray(e["tree_indices"])
            outside = np.ones(n_leaves, bool)
            outside[ti[a]:(ti[stop] if stop < T else n_leaves)] = False
            assert not counts[outside].any()                                     # leaves of trees outside the range are 0


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_categorical_columns_raw_cells_device_cells_and_encoded_ids(policy):
    import torch
    F, Fc, D, T = 3, 2, 2, 14
    rng = np.random.default_rng(11 if policy == "greedy" else 12)
    m = _model(F, Fc, D, 4, policy)
    _grow(m, rng, T, F, Fc, D)
    e = m.get_ensemble_data()
    assert (np.asarray(e["is_numerics"]) == 0).any(), "no categorical condition was grown"
    dev = torch.device("cuda:0")
    for n in BATCHES:
        X, Xc = _batch(rng, n, F, Fc)
        ids, token = m.encode_categorical(Xc)
        ids = np.asarray(ids)
        cells = torch.from_numpy(np.frombuffer(Xc.tobytes(), np.uint8).reshape(n, Fc, 128).copy()).to(dev)
        cells_arg = (cells.data_ptr(), (n, Fc), "S128", "cuda")
        for a, b in ((0, 0), (3, 11)):
            raw, raw_counts = _check(m, e, policy, X, Xc, a, b)
            enc, enc_counts = _check(m, e, policy, X, Xc, a, b, encoded=(ids, token))
            on_dev = _four(lambda: m.predict_leaves(X, cells_arg, a, b))
            on_dev_counts = _four(lambda: m.leaf_counts(X, cells_arg, a, b))
            assert raw.tobytes() == enc.tobytes() == on_dev.tobytes()
            assert raw_counts.tobytes() == enc_counts.tobytes() == on_dev_counts.tobytes()


def test_a_stale_dictionary_token_is_refused():
    F, Fc, D = 4, 2, 2
    rng = np.random.default_rng(3)
    tokens20 = np.array(["c%02d" % i for i in range(20)], dtype="S128")
    m = _model(F, Fc, D, 3, policy="greedy")
    X = rng.standard_normal((384, F)).astype(np.float32)
    Xc = tokens20[rng.integers(0, 20, (384, Fc))]
    m.step(X, Xc, rng.standard_normal((384, D)).astype(np.float32))
    ids, token = m.encode_categorical(Xc)
    ids = np.asarray(ids)
    assert np.asarray(m.predict_leaves_encoded(X, ids, token)).tobytes() == np.asarray(m.predict_leaves(X, Xc)).tobytes()
    refused = False
    for _ in range(40):
        G = rng.standard_normal((384, D)).astype(np.float32) + (Xc[:, :1] == tokens20[rng.integers(0, 20)]) * 4.0
        m.step(X, Xc, np.ascontiguousarray(G.astype(np.float32)))
        _, t2 = m.encode_categorical(Xc[:8])
        if t2 != token:
            with pytest.raises(RuntimeError, match="another category dictionary"):
                m.predict_leaves_encoded(X, ids, token)
            with pytest.raises(RuntimeError, match="another category dictionary"):
                m.leaf_counts_encoded(X, ids, token)
            refused = True
            break
    assert refused, "the dictionary never grew in 40 steps on 20 tokens x 2 columns"


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("D", [1, 8])
def test_tie_to_predict_continue_bit_for_bit(policy, D):
    """With the power-of-two rate 0.125, lr * v is exact in float32, so fma(-lr, v, p) is the single float32 subtraction p - lr * v, which
    NumPy performs exactly: the chain restated from the leaf matrix has the bytes of predict_continue(tiled bias, 0, T)."""
    F, T = 8, 15
    rng = np.random.default_rng(40 + D + (100 if policy == "greedy" else 0))
    m = _model(F, 0, D, 3, policy, lr=0.125)
    _grow(m, rng, T, F, 0, D)
    e = m.get_ensemble_data()
    values = np.asarray(e["values"], np.float32).reshape(-1, D)
    bias = np.asarray(m.get_bias(), np.float32).reshape(-1)
    for n in BATCHES:
        X, _ = _batch(rng, n, F, 0)
        leaves = _four(lambda: m.predict_leaves(X, None, 0, T))
        assert leaves.min() >= 0
        p = np.ascontiguousarray(np.tile(bias, (n, 1)))
        for t in range(T):
            p = p - np.float32(0.125) * values[leaves[:, t]]
            assert p.dtype == np.float32
        base = np.ascontiguousarray(np.tile(bias, (n, 1))) if D > 1 else np.full(n, bias[0], np.float32)
        got = np.asarray(m.predict_continue(X, None, base, 0, T))
        assert got.tobytes() == p.reshape(got.shape).tobytes()


def test_leaf_counts_many_tiles_and_many_flushing_blocks():
    """5 000 rows are 79 tiles: with one tile per block every block flushes its counters into the same global ones."""
    F, D, T = 8, 2, 12
    rng = np.random.default_rng(61)
    for policy in ("oblivious", "greedy"):
        m = _model(F, 0, D, 4, policy)
        _grow(m, rng, T, F, 0, D)
        e = m.get_ensemble_data()
        X, _ = _batch(rng, 5000, F, 0)
        for a, b in ((0, 0), (2, 9)):
            _, counts = _check(m, e, policy, X, None, a, b)
            stop = b if b else T
            assert _per_tree_sums(e, counts, a, stop) == [5000] * (stop - a)


def test_leaf_counts_over_a_range_that_spans_two_counter_chunks():
    """One launch of k_leaf_counts keeps at most GBRL.leaf_counts_chunk() counters on chip; a range with more leaves is cut into runs of whole
    trees.  Depth-6 oblivious trees have 64 leaves, so chunk / 64 + 5 of them do not fit one chunk; a sub-range that starts inside the first
    run and ends inside the second is checked too."""
    import gbrl_amd
    chunk = gbrl_amd.GBRL.leaf_counts_chunk()
    depth = 6
    T = chunk // (1 << depth) + 5
    F, D = 8, 1
    rng = np.random.default_rng(71)
    m = _model(F, 0, D, depth)
    _grow(m, rng, T, F, 0, D, rows=256)
    e = m.get_ensemble_data()
    n_leaves = np.asarray(e["values"]).shape[0]
    assert n_leaves > chunk, "the trees came out too shallow to span two chunks: %d leaves" % n_leaves
    ti = np.asarray(e["tree_indices"])
    first_run = int(np.searchsorted(ti, chunk, side="right")) - 1        # trees [0, first_run) fit the first chunk
    assert 0 < first_run < T
    for n in (65, 200):
        X, _ = _batch(rng, n, F, 0)
        for a, b in ((0, 0), (first_run - 2, first_run + 2), (1, T)):
            _, counts = _check(m, e, "oblivious", X, None, a, b)
            stop = b if b else T
            assert _per_tree_sums(e, counts, a, stop) == [n] * (stop - a)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_fallback_rows_too_wide_for_the_lds_tile(policy):
    """F = 640: the 64-row tile would be 160 KiB, so both calls run the one-thread-per-row kernels on rows in global memory."""
    F, D, T, n = 640, 2, 12, 65
    rng = np.random.default_rng(81)
    m = _model(F, 0, D, 3, policy)
    _grow(m, rng, T, F, 0, D, rows=256)
    e = m.get_ensemble_data()
    X, _ = _batch(rng, n, F, 0)
    for a, b in ((0, 0), (3, 11)):
        _check(m, e, policy, X, None, a, b)


def test_trees_grown_on_gradients_constant_in_x():
    """The contract's fallback list names a model with a depth-0 stump, which gradients that are constant in X were expected to produce.  At
    these settings (256 rows, F = 8, max_depth = 3, n_bins = 32, all-ones and all-zero gradients) the grower never emits one -- it still grows
    full-depth trees under both policies.  The trees it does grow from such gradients are checked like any others; the NumPy walk holds
    whatever their depth.  The depth-0 case is test_a_depth0_tree_in_the_middle_and_last below, which grows one with min_data_in_leaf."""
    F, D = 8, 2
    rng = np.random.default_rng(95)
    for policy in ("oblivious", "greedy"):
        m = _model(F, 0, D, 3, policy)
        X, _ = _batch(rng, 256, F, 0)
        m.step(X, None, rng.standard_normal((256, D)).astype(np.float32))
        m.step(X, None, np.ones((256, D), np.float32))
        m.step(X, None, np.zeros((256, D), np.float32))
        e = m.get_ensemble_data()
        for a, b in ((0, 0), (1, 3)):
            _check(m, e, policy, X[:65], None, a, b)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("where", ["middle", "last"])
def test_a_depth0_tree_in_the_middle_and_last(where, policy):
    """Grown as tests/test_gpu_edges.py grows it: min_data_in_leaf = 60, a step on 300 rows splits, a step on 100 rows appends a single depth-0
    leaf.  "middle": 3 trees, the depth-0 tree, 2 trees; "last": 3 trees, then two depth-0 trees.  Oblivious: the depth-0 tree routes every row
    to its one leaf.  Greedy: that leaf never passes, so the tree reports a leaf of the following tree, and -1 where no tree follows -- those
    rows join no count."""
    F, D = 4, 2
    plan = {"middle": (300, 300, 300, 100, 300, 300), "last": (300, 300, 300, 100, 100)}[where]
    T = len(plan)
    rng = np.random.default_rng(81 + (where == "last") + 2 * (policy == "greedy"))
    m = _model(F, 0, D, 3, policy, min_data_in_leaf=60)
    for rows in plan:
        _grow(m, rng, 1, F, 0, D, rows=rows)
    assert m.get_num_trees() == T
    e = m.get_ensemble_data()
    ti = np.asarray(e["tree_indices"]); dep = np.asarray(e["depths"]); n_leaves = np.asarray(e["values"]).shape[0]
    ends = np.append(ti[1:], n_leaves)
    depths = [int(dep[t]) if policy == "oblivious" else int(dep[ti[t]:ends[t]].max()) for t in range(T)]
    assert [d == 0 for d in depths] == [rows == 100 for rows in plan], depths
    for n in (65, 200):
        X, _ = _batch(rng, n, F, 0)
        for a, b in [(0, 0), (1, T)] + [(t, t + 1) for t in range(T)]:
            leaves, counts = _check(m, e, policy, X, None, a, b)
            if (a, b) != (0, 0):
                continue
            for t in range(T):
                if depths[t] > 0 or policy == "oblivious":
                    assert ((leaves[:, t] >= ti[t]) & (leaves[:, t] < ends[t])).all()
                elif where == "middle":
                    assert ((leaves[:, t] >= ti[t + 1]) & (leaves[:, t] < ends[t + 1])).all()      # a leaf of the following tree
                else:
                    assert (leaves[:, t] == -1).all()                                              # the search ran off the ensemble


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_width_independence_130_outputs(policy):
    """Leaf routing reads no leaf value: a model with 130 outputs, which `step` grows and `predict` refuses, is routed like any other."""
    F, D, T = 8, 130, 12
    rng = np.random.default_rng(97)
    m = _model(F, 0, D, 3, policy)
    _grow(m, rng, T, F, 0, D, rows=256)
    assert m.get_num_trees() == T
    e = m.get_ensemble_data()
    for n in (65, 200):
        X, _ = _batch(rng, n, F, 0)
        for a, b in ((0, 0), (3, 11)):
            _check(m, e, policy, X, None, a, b)
        with pytest.raises(RuntimeError, match="output_dim > 128"):
            m.predict(X, None)
    # the route for wide models: the indices select the rows of `values`
    leaves = np.asarray(m.predict_leaves(X, None))
    assert np.asarray(e["values"]).reshape(-1, D)[leaves].shape == (200, T, D)


def test_a_cuda_model_returns_an_int32_capsule_on_the_device():
    import torch
    F, D, T, n = 8, 3, 13, 200
    rng = np.random.default_rng(91)
    m = _model(F, 0, D, 3)
    _grow(m, rng, T, F, 0, D)
    X, _ = _batch(rng, n, F, 0)
    want = np.asarray(m.predict_leaves(X, None))
    want_sub = np.asarray(m.predict_leaves(X, None, 3, 11))
    want_counts = m.leaf_counts(X, None)
    m.to_device("cuda")
    try:
        for generic in ("0", "1"):
            with _env("GBRL_HIP_LEAVES_GENERIC", generic):
                got = torch.from_dlpack(m.predict_leaves(X, None))
                sub = torch.from_dlpack(m.predict_leaves(X, None, 3, 11))
                counts = m.leaf_counts(X, None)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, T) and got.device.type == "cuda"
            assert got.cpu().numpy().tobytes() == want.tobytes()
            assert tuple(sub.shape) == (n, 8) and sub.cpu().numpy().tobytes() == want_sub.tobytes()
            assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.tobytes() == want_counts.tobytes()
    finally:
        m.to_device("cpu")
