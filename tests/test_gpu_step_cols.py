"""step_prepared on a column subset, on the GPU (GBRL.step_prepared(ds, G, cols=c); include/gbrl_hip.h, "Column subsampling").  The definition under test:

    A.step_prepared(ds, G, cols=c)                   A: input_dim = F, feature weights w, ds = A.prepare_dataset(X)
 == B.step_prepared(B.prepare_dataset(X[:, c]), G)   B: input_dim = len(c), feature weights w[c]

Every per-tree array of get_ensemble_data() is equal bit for bit, except that the feature indices of used conditions satisfy A == c[B] (the
arrays of length input_dim -- mapping and weights -- have the models' own lengths), and A.predict(X) has the bits of B.predict(X[:, c]).  Nothing
here has a tolerance."""
import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

F, N_BINS, DEPTH = 20, 16, 3
W = np.array([1.0, 0.5, 2.0, 0.25, 1.5, 1.0, 0.75, 3.0, 0.1, 1.25, 0.9, 1.1, 2.5, 0.6, 1.0, 0.3, 1.7, 0.8, 1.4, 0.45], np.float32)
TREE_ARRAYS = ("bias", "tree_indices", "depths", "values", "feature_values", "edge_weights", "is_numerics", "inequality_directions", "categorical_values")
COLS = (np.array([0, 3, 4, 9, 11, 17, 19], np.int32), np.array([1, 2, 3, 8, 15, 16, 18], np.int32), np.array([5, 6, 7, 10, 12, 13, 14], np.int32))


def _model(n_in, D, policy, score, gen, parity="default", fw=None):
    m = gbrl_amd.GBRL(input_dim=n_in, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=N_BINS, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", parity_mode=parity)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(n_in, np.float32) if fw is None else np.ascontiguousarray(fw, np.float32))
    m.set_feature_mapping(np.arange(n_in, dtype=np.int32), np.ones(n_in, dtype=bool))
    return m


_DATA = {}


def _data(n, D):
    if (n, D) not in _DATA:
        rng = np.random.default_rng(17 * n + D)
        X = rng.standard_normal((n, F)).astype(np.float32)
        Wm = rng.standard_normal((F, D)).astype(np.float32)
        Y = (np.tanh(X @ Wm) + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
        _DATA[(n, D)] = (X, Y)
    return _DATA[(n, D)]


def _grads(m, X, Y):
    P = np.asarray(m.predict(X, None, 0, 0), np.float32).reshape(Y.shape)
    G = np.ascontiguousarray((P - Y).astype(np.float32))
    return G[:, 0].copy() if Y.shape[1] == 1 else G


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _split_row_cols(e, policy, cols_per_tree):
    """the column list that the conditions of every split row were grown on: a row per tree (oblivious) or per leaf (greedy)"""
    ti = np.asarray(e["tree_indices"])
    S = np.asarray(e["depths"]).size
    if policy == "oblivious":
        return [cols_per_tree[s] for s in range(S)]
    return [cols_per_tree[int(np.searchsorted(ti, s, side="right")) - 1] for s in range(S)]


def _assert_a_is_b_through_cols(a, b, policy, cols_per_tree, what=""):
    ea, eb = a.get_ensemble_data(), b.get_ensemble_data()
    for k in TREE_ARRAYS:
        va, vb = np.asarray(ea[k]), np.asarray(eb[k])
        assert va.shape == vb.shape and va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), "%s ensemble array %s differs" % (what, k)
    fa, fb = np.asarray(ea["feature_indices"]), np.asarray(eb["feature_indices"])
    depths = np.asarray(ea["depths"])
    assert fa.shape == fb.shape
    fa, fb = fa.reshape(depths.size, -1), fb.reshape(depths.size, -1)
    rows = _split_row_cols(ea, policy, cols_per_tree)
    n_used = 0
    for s in range(depths.size):
        for d in range(fa.shape[1]):
            if d < depths[s]:
                assert fa[s, d] == rows[s][fb[s, d]], "%s split row %d, condition %d: feature %d, the subset model has %d" % (what, s, d, fa[s, d], fb[s, d])
                assert fa[s, d] in rows[s].tolist(), "a feature outside cols"
                n_used += 1
            else:
                assert fa[s, d] == fb[s, d]
    return n_used


@pytest.mark.parametrize("parity", ["default", "exact_argmax"])
@pytest.mark.parametrize("n", [600, 9000])           # one-launch growth, the level loop
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("gen", ["Quantile", "Uniform"])
@pytest.mark.parametrize("score", ["L2", "Cosine"])
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_a_step_on_a_column_subset_is_the_step_on_the_subset_data_set(policy, score, gen, D, n, parity):
    X, Y = _data(n, D)
    a = _model(F, D, policy, score, gen, parity, fw=W)
    ds = a.prepare_dataset(X)
    b = _model(COLS[0].size, D, policy, score, gen, parity, fw=W[COLS[0]])
    for k, c in enumerate(COLS):   # three steps in a row, each on other columns (of one width: B's input_dim)
        G = _grads(a, X, Y)
        b.set_feature_weights(np.ascontiguousarray(W[c]))
        a.step_prepared(ds, G, cols=c)
        b.step_prepared(b.prepare_dataset(np.ascontiguousarray(X[:, c])), G)
        assert a.get_num_trees() == b.get_num_trees() == k + 1
        if k == 0:
            _assert_a_is_b_through_cols(a, b, policy, [c], "after step 0:")
            pa = np.asarray(a.predict(X, None, 0, 0), np.float32)
            pb = np.asarray(b.predict(np.ascontiguousarray(X[:, c]), None, 0, 0), np.float32)
            assert pa.tobytes() == pb.tobytes(), "the predictions differ"
    used = _assert_a_is_b_through_cols(a, b, policy, list(COLS), "after three steps:")
    assert used > 0, "the premise: the trees have conditions"
    md = a.get_metadata()
    assert md["input_dim"] == F and md["iteration"] == 3


@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("n", [600, 9000])
def test_every_column_is_the_call_without_cols(policy, score, gen, n, tmp_path):
    D = 3
    X, Y = _data(n, D)
    files, phases = [], []
    for cols in (None, np.arange(F, dtype=np.int32), list(range(F))):
        m = _model(F, D, policy, score, gen, fw=W)
        ds = m.prepare_dataset(X)
        m.set_profiling(2)
        m.step_prepared(ds, _grads(m, X, Y), cols=cols)
        phases.append(sorted(k for k in m.last_phase_times() if k.startswith("gather")))
        m.set_profiling(0)
        files.append(_file(m, tmp_path))
    assert files[0] == files[1] == files[2]
    assert phases == [[], [], []], phases
    m = _model(F, D, policy, score, gen, fw=W)
    ds = m.prepare_dataset(X)
    m.set_profiling(2)
    m.step_prepared(ds, _grads(m, X, Y), cols=COLS[0])
    assert "gather_cols" in m.last_phase_times() and "gather_codes" not in m.last_phase_times()
    assert _file(m, tmp_path) != files[0]


@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform"), ("oblivious", "Cosine", "Uniform")])
@pytest.mark.parametrize("n", [600, 9000])
def test_rows_and_cols_together(policy, score, gen, n):
    import torch
    D, c = 3, COLS[1]
    X, Y = _data(n, D)
    rng = np.random.default_rng(n)
    rows = rng.integers(0, n, 2 * n // 3).astype(np.int32)   # unordered, with duplicates
    for dev_rows in (False, True):
        a = _model(F, D, policy, score, gen, fw=W)
        ds = a.prepare_dataset(X)
        b = _model(c.size, D, policy, score, gen, fw=W[c])
        dsb = b.prepare_dataset(np.ascontiguousarray(X[:, c]))
        G = np.ascontiguousarray(_grads(a, X, Y)[rows])
        a.set_profiling(2)
        if dev_rows:
            t = torch.from_numpy(rows).cuda()
            a.step_prepared(ds, G, rows=(t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda"), cols=c)
        else:
            a.step_prepared(ds, G, rows=rows, cols=c)
        ph = a.last_phase_times()
        assert "gather_cols" in ph and "gather_codes" not in ph, sorted(ph)   # rows and columns in one pass
        b.step_prepared(dsb, G, rows=rows)
        assert _assert_a_is_b_through_cols(a, b, policy, [c]) > 0


@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")])
@pytest.mark.parametrize("n", [600, 9000])
def test_a_step_without_cols_after_a_step_with_cols(policy, score, gen, n, tmp_path):
    """the per-model step constants (candidate tables and their device copy) are those of the full step again: the bytes are those a model
    leaves that has the same trees and never saw cols (the saved model, loaded)"""
    D = 3
    X, Y = _data(n, D)
    a = _model(F, D, policy, score, gen, fw=W)
    ds = a.prepare_dataset(X)
    a.step_prepared(ds, _grads(a, X, Y))                  # the constants of the full step are built and uploaded
    a.step_prepared(ds, _grads(a, X, Y), cols=COLS[2])    # a subset step in between
    p = tmp_path / "between.gbrl_model"
    assert a.save(str(p)) == 0
    fresh = gbrl_amd.GBRL.load(str(p))
    G = _grads(a, X, Y)
    a.step_prepared(ds, G)
    fresh.step_prepared(fresh.prepare_dataset(X), G)
    assert a.get_num_trees() == fresh.get_num_trees() == 3
    assert _file(a, tmp_path) == _file(fresh, tmp_path)
    # ... and a subset step after a subset step on other columns of the same width
    a.step_prepared(ds, G, cols=COLS[0])
    fresh.step_prepared(fresh.prepare_dataset(X), G, cols=COLS[0])
    assert _file(a, tmp_path) == _file(fresh, tmp_path)


def test_a_refused_call_leaves_the_model_unchanged(tmp_path):
    n, D = 600, 3
    X, Y = _data(n, D)
    for steps_before in (0, 1):
        m = _model(F, D, "oblivious", "L2", "Quantile", fw=W)
        ds = m.prepare_dataset(X)
        for _ in range(steps_before):
            m.step_prepared(ds, _grads(m, X, Y), cols=COLS[0])
        G = _grads(m, X, Y)   # (a model's first predict books the feature counts: before the file is read)
        before = _file(m, tmp_path)
        for cols, what in (([3, 2], "strictly ascending"), ([2, 2], "strictly ascending"), ([0, F], "outside"), ([-1, 3], "outside"), ([], "between 1 and"),
                           (list(range(F + 1)), "between 1 and")):
            with pytest.raises(RuntimeError, match=what):
                m.step_prepared(ds, G, cols=np.asarray(cols, np.int32))
            assert _file(m, tmp_path) == before, cols
        with pytest.raises(RuntimeError, match="outside"):
            m.step_prepared(ds, G[:2], rows=np.array([0, n], np.int32), cols=COLS[0])
        assert _file(m, tmp_path) == before
        assert m.get_metadata()["iteration"] == steps_before
