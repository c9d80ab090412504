"""Data sets bound to another data set's thresholds on the GPU (GBRL.prepare_dataset(obs, reference=ds); include/gbrl_hip.h:
gbrl_hip_dataset_create_like).  Every comparison is exact (bytes):
  * the records of a bound set made from X[idx] against the reference's own gathered records ds.codes(rows=idx), padding included -- NumPy obs, a
    device tuple, a chain of references, and with the reference destroyed before the bound set is used -- over n around the 64-row and 256-row
    tiles, F around the 16-feature groups, bin counts on the LDS path and n_bins = 4096 on the global-memory path, both generators;
  * fresh rows against the NumPy count rule on ds.thresholds(): cells equal to a threshold, below the minimum, above the maximum, a constant
    column, signed zeros, infinities, NaN;
  * thresholds() and thresholds_id;
  * predict_continue_prepared on a bound set against predict_continue on the fresh observations, both kernels and policies, also after
    interleaved calls on the reference, the bound set and an unrelated data set (the code tables are keyed on the thresholds id);
  * step_prepared on a bound set against the subset step on the reference, either side of the one-launch growth limit;
  * the refusals that need a live reference.
"""
import gc
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu


def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, batch_size=5000):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
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


def _rule_codes(thr, X):
    """[G, m, 16] by the count rule: code = #{b : thr[f][b] < x} (NumPy's float <: -0.0 == +0.0, NaN below everything); padding zero"""
    F, m = thr.shape[0], X.shape[0]
    out = np.zeros(((F + 15) // 16, m, 16), np.uint16)
    for f in range(F):
        out[f // 16, :, f % 16] = (thr[f][None, :] < X[:, f][:, None]).sum(axis=1)
    return out


# ---- 1. bound == gathered ---------------------------------------------------------------------------------------------------------------------
LIKE_CASES = [
    # n (reference rows), F, n_bins, generator, m (bound rows)
    (1, 1, 2, "Quantile", 1),
    (63, 15, 32, "Uniform", 65),
    (64, 16, 256, "Quantile", 63),
    (65, 17, 300, "Uniform", 257),
    (257, 33, 4096, "Quantile", 64),        # 16 * 4096 * 4 bytes = 256 KiB of keys per group: searched in global memory
    (4097, 128, 256, "Uniform", 4097),
    (4097, 16, 4096, "Uniform", 257),
    (257, 128, 2, "Quantile", 4097),
    (4097, 1, 300, "Quantile", 65),
    (63, 33, 32, "Quantile", 1),
    (65, 15, 4096, "Uniform", 4097),
    (4097, 17, 32, "Uniform", 64),
    (257, 17, 2000, "Quantile", 65),        # 125 KiB of keys per group: the LDS path behind the opt-in above 64 KiB
]


@pytest.mark.parametrize("n,F,n_bins,gen,m_rows", LIKE_CASES)
def test_a_bound_set_holds_the_reference_s_gathered_records(n, F, n_bins, gen, m_rows):
    import torch
    X, _ = _data(n, F, 1, seed=9000 + n + 31 * F + n_bins)
    rng = np.random.default_rng(n + F)
    idx = rng.integers(0, n, size=m_rows).astype(np.int32)      # unsorted, with duplicates
    idx[-1] = idx[0]
    Xi = np.ascontiguousarray(X[idx])
    m = _model(F, n_bins=n_bins, gen=gen)
    ds = m.prepare_dataset(X)
    want = ds.codes(rows=idx)
    thr, tid, ref_bytes = ds.thresholds(), ds.thresholds_id, ds.nbytes
    assert tid != 0
    b1 = m.prepare_dataset(Xi, reference=ds)
    t = torch.from_numpy(Xi).cuda()
    b2 = m.prepare_dataset(_dev(t), reference=ds)
    chain = m.prepare_dataset(Xi, reference=b1)
    other = m.prepare_dataset(Xi)
    del ds
    gc.collect()                                                 # the reference is destroyed before the bound sets are used
    G = (F + 15) // 16
    assert want.shape == (G, m_rows, 16)
    for name, b in (("numpy obs", b1), ("device obs", b2), ("bound to a bound set", chain)):
        got = b.codes()
        assert got.dtype == np.uint16 and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), "%s: records differ at %s" % (name, np.argwhere(got != want)[:3].tolist())
        assert b.thresholds().tobytes() == thr.tobytes(), name
        assert b.thresholds_id == tid, name
        assert (b.n_rows, b.n_features, b.n_bins, b.generator_type) == (m_rows, F, n_bins, gen)
        exact = G * m_rows * 32 + 3 * F * n_bins * 4             # codes + thresholds, their keys (device) and the host thresholds
        assert exact <= b.nbytes <= exact + exact // 8 + 3 * 256, (b.nbytes, exact)   # (device buffers are allocated with an eighth of slack)
    if F % 16:
        assert not want[-1, :, F % 16:].any(), "padding slots are zero"
    assert want.tobytes() == _rule_codes(thr, Xi).tobytes()
    assert other.thresholds_id not in (0, tid), "an independent data set has thresholds of its own"
    assert b1.codes(rows=np.array([m_rows - 1, 0], np.int32)).tobytes() == np.ascontiguousarray(want[:, [m_rows - 1, 0], :]).tobytes()
    assert ref_bytes > 0


# ---- 2. fresh rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n_bins,gen", [(6, 16, "Quantile"), (17, 300, "Uniform"), (33, 4096, "Quantile"), (16, 2, "Uniform")])
def test_fresh_rows_follow_the_count_rule(F, n_bins, gen):
    n, mv = 500, 321
    rng = np.random.default_rng(100 + F)
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[:, 1 % F] = 1.5                                            # a constant column: every threshold of it is the same value (or none below)
    X[rng.integers(0, n, 30), 0] = np.float32(0.0)               # zero among the candidates
    m = _model(F, n_bins=n_bins, gen=gen)
    ds = m.prepare_dataset(X)
    thr = ds.thresholds()
    Xv = (1.7 * rng.standard_normal((mv, F))).astype(np.float32)
    for f in range(F):                                           # cells equal to a threshold, to the smallest and to the largest
        rows = rng.integers(0, mv, 12)
        Xv[rows, f] = thr[f][rng.integers(0, n_bins, 12)]
        Xv[rng.integers(0, mv), f] = thr[f].min()
        Xv[rng.integers(0, mv), f] = thr[f].max()
    Xv[0, :] = -1e30                                             # below the reference's minimum: code 0
    Xv[1, :] = 1e30                                              # above its maximum: code n_bins
    Xv[2, :] = np.float32(-0.0)
    Xv[3, :] = np.float32(0.0)
    Xv[4, :] = np.inf
    Xv[5, :] = -np.inf
    Xv[6, :] = np.nan                                            # below every threshold
    Xv[7, :] = 1.5
    Xv[8, :] = np.nextafter(np.float32(1.5), np.float32(2.0))
    Xv[9, :] = np.nextafter(np.float32(1.5), np.float32(1.0))
    bound = m.prepare_dataset(Xv, reference=ds)
    got, want = bound.codes(), _rule_codes(thr, Xv)
    assert got.tobytes() == want.tobytes(), "cells %s differ from the count rule" % np.argwhere(got != want)[:5].tolist()
    f_all = np.arange(F)
    assert not got[f_all // 16, 0, f_all % 16].any() and not got[f_all // 16, 6, f_all % 16].any() and not got[f_all // 16, 5, f_all % 16].any()
    assert (got[f_all // 16, 1, f_all % 16] == n_bins).all() and (got[f_all // 16, 4, f_all % 16] == n_bins).all()
    assert got[:, 2, :].tobytes() == got[:, 3, :].tobytes(), "-0.0 and +0.0 have one code"


# ---- 3. continue on a bound set -----------------------------------------------------------------------------------------------------------------
def _continue_both(m, ds, base, a, b):
    out = []
    for generic in ("0", "1"):
        with _env("GBRL_HIP_CONTINUE_GENERIC", generic):
            out.append(np.asarray(m.predict_continue_prepared(ds, base, a, b)))
    assert out[0].tobytes() == out[1].tobytes(), "k_continue_codes and k_continue_codes_general differ over [%d, %d)" % (a, b)
    return out[0]


@pytest.mark.parametrize("policy,score,gen,F,D,n_bins", [("oblivious", "L2", "Quantile", 17, 3, 300), ("greedy", "Cosine", "Uniform", 33, 8, 32),
                                                          ("oblivious", "L2", "Uniform", 16, 1, 4096), ("greedy", "Cosine", "Quantile", 17, 65, 32)])
def test_continue_on_a_bound_set_is_continue_on_the_fresh_rows(policy, score, gen, F, D, n_bins):
    n, mv, T = 1000, 257, 4
    X, Y = _data(n, F, D, seed=200 + F)
    Xv, _ = _data(mv, F, D, seed=201 + F)
    m = _model(F, D, policy=policy, score=score, gen=gen, n_bins=n_bins)
    ds = m.prepare_dataset(X)
    rng = np.random.default_rng(5)
    for _ in range(T):
        m.step_prepared(ds, _shape((Y * rng.uniform(0.5, 1.5) + 0.2 * rng.standard_normal(Y.shape)).astype(np.float32), D))
    assert m.get_num_trees() == T and np.asarray(m.get_ensemble_data()["depths"]).max() >= 1
    bound = m.prepare_dataset(Xv, reference=ds)
    unrelated = m.prepare_dataset(Xv)
    bias_v = _shape(np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (mv, 1)), D)
    bias_x = _shape(np.tile(np.asarray(m.get_bias(), np.float32).reshape(1, D), (n, 1)), D)

    def check():
        for a, b in ((0, T), (2, T), (1, 2), (0, 0)):
            base = bias_v if a == 0 else np.asarray(m.predict_continue(Xv, None, bias_v, 0, a))
            want = np.asarray(m.predict_continue(Xv, None, base, a, b))
            got = _continue_both(m, bound, base, a, b)
            assert got.tobytes() == want.tobytes(), "[%d, %d): rows %s" % (a, b, np.argwhere(got != want)[:3].tolist())

    check()
    # interleaved: the reference (same thresholds id: the tables stay), an unrelated data set (they are reset), and back
    want_x = np.asarray(m.predict_continue(X, None, bias_x, 0, 0))
    assert _continue_both(m, ds, bias_x, 0, 0).tobytes() == want_x.tobytes()
    check()
    assert np.asarray(m.predict_continue_prepared(unrelated, bias_v, 2, 2)).tobytes() == bias_v.tobytes()   # an empty range names the data set, no more
    with pytest.raises(RuntimeError, match="does not compare against one of the data set's thresholds"):
        m.predict_continue_prepared(unrelated, bias_v, 0, 0)
    check()
    assert _continue_both(m, ds, bias_x, 0, 0).tobytes() == want_x.tobytes()
    # one more tree grown on the bound set itself: the reference's thresholds, so both data sets still express every tree
    m.step_prepared(bound, _shape(np.ascontiguousarray(Y[:mv]), D))
    T += 1
    check()
    assert _continue_both(m, ds, bias_x, 0, 0).tobytes() == np.asarray(m.predict_continue(X, None, bias_x, 0, 0)).tobytes()


# ---- 4. a step on a bound set ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,score", [("oblivious", "L2"), ("greedy", "Cosine")])
@pytest.mark.parametrize("n,F,m_rows", [(1000, 7, 300), (12000, 16, 9000)])      # either side of the one-launch growth limit
def test_a_step_on_a_bound_set_is_the_subset_step(n, F, m_rows, policy, score, tmp_path):
    D = 3
    X, Y = _data(n, F, D, seed=300 + n)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, n, size=m_rows).astype(np.int32)
    a = _model(F, D, policy=policy, score=score, n_bins=64)
    b = _model(F, D, policy=policy, score=score, n_bins=64)
    ds = a.prepare_dataset(X)
    bound = a.prepare_dataset(np.ascontiguousarray(X[idx]), reference=ds)
    for k in range(2):
        G = np.ascontiguousarray((Y[idx] * (1.0 + 0.5 * k) + 0.1 * rng.standard_normal((m_rows, D))).astype(np.float32))
        a.step_prepared(bound, G)
        b.step_prepared(ds, G, rows=idx)
    assert a.get_num_trees() == b.get_num_trees() == 2
    assert np.asarray(a.get_ensemble_data()["depths"]).max() >= 1
    assert _file(a, tmp_path) == _file(b, tmp_path)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_live_reference():
    n, F = 300, 5
    X, _ = _data(n, F, 1, seed=400)
    m = _model(F)
    ds = m.prepare_dataset(X)
    with pytest.raises(RuntimeError, match="n_bins"):
        _model(F, n_bins=64).prepare_dataset(X, reference=ds)
    with pytest.raises(RuntimeError, match="generator_type"):
        _model(F, gen="Uniform").prepare_dataset(X, reference=ds)
    with pytest.raises(RuntimeError, match="Total number of features"):
        _model(F + 1).prepare_dataset(X, reference=ds)
    with pytest.raises(RuntimeError, match="features, the reference"):
        m.prepare_dataset(np.zeros((10, F + 1), np.float32), reference=ds)
    with pytest.raises(RuntimeError, match="without obs"):
        m.prepare_dataset(np.zeros((0, F), np.float32), reference=ds)
    assert m.get_num_trees() == 0 and m.prepare_dataset(X[:3], reference=ds).n_rows == 3
