"""GBRL.rank_gradient on the GPU (include/gbrl_hip.h, "Ranking objectives"; gbrl_amd/csrc/rank.hip) against the host rule, bytes only.
tests/test_rank_host.py holds gbrl_cpp.rank_gradient_host to an independent NumPy walk; here
  1. grad, hess, ndcg, positions and pairs are the host rule's with no tolerance, for both objectives, with and without ndcg_at, from NumPy arrays and
     from device tuples, on layouts whose queries start at unaligned rows, cross wave and block boundaries, are all of size 2, or are one query of the
     largest size; two calls give the same bytes, the loss included;
  2. the device loss: lambdarank against 1 - mean(host ndcg), pairwise against a float64 NumPy evaluation, each within its summation bound;
  3. newton_leaves_prepared(group=): the int64 sums per leaf are those of newton_quantise over the host rule's g and h, leaves from predict_leaves,
     through the streaming and the general kernel, on oblivious and greedy trees of depth 1, 3 and 6; bits = newton_sum_bits(n, largest group);
  4. what is refused (a score that is not finite, a query of 1025 rows, a label of 31, sizes that do not sum to n) names the query or the row and
     leaves the model's file bytes as they were.
"""
import os

import numpy as np
import pytest
import torch

import gbrl_amd
import rank_cases as R   # tests/golden (conftest.py puts it on the path)

pytestmark = pytest.mark.gpu

cpp = gbrl_amd.gbrl_cpp
f32 = np.float32
LAYOUTS = {"mixed": R.LAYOUT, "twos": [2] * 3000, "one_1024": [1024], "two_1024_and_1": [1024, 1024, 1]}
KINDS = [("pairwise", None), ("lambdarank", None), ("lambdarank", 10)]


def _model():
    m = gbrl_amd.GBRL(input_dim=4, output_dim=1, policy_dim=1, max_depth=3, n_bins=16, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious",
                      device="cpu", batch_size=5000)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=1)
    return m


@pytest.fixture(scope="module")
def model():
    return _model()


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t, (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def _np(x):
    return x if isinstance(x, np.ndarray) else torch.from_dlpack(x).cpu().numpy()


def _same(r, want, what):
    for k in ("grad", "hess", "ndcg", "positions"):
        got = _np(r[k])
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k)
        assert got.tobytes() == want[k].tobytes(), (what, k, np.nonzero(got != want[k])[0][:5])
    assert r["pairs"] == want["pairs"], what


def _check_loss(r, want, s, y, group, objective, what):
    """lambdarank: Q terms in [0, 1], each bit-exact, summed in another order than np.mean's: (Q + 8) * 2^-52 relative.  pairwise: P terms of a float64
    libm expression, the bound tests/test_gpu_objective.py derives for the logistic loss with the pair count in place of n * D: (P + 8) * 2^-52 relative."""
    if objective == "lambdarank":
        ref, terms = 1.0 - float(np.mean(want["ndcg"])), len(group)
    else:
        ref, terms = R.pairwise_loss(s, y, group)
        assert terms == want["pairs"]
    scale = abs(ref)
    rel = abs(r["loss"] - ref) / scale if scale > 0 else abs(r["loss"] - ref)
    print("%s: loss %.17g reference %.17g relative difference %.3g bound %.3g" % (what, r["loss"], ref, rel, (terms + 8) * 2.0 ** -52))
    assert rel <= (terms + 8) * 2.0 ** -52, (what, r["loss"], ref, rel)


@pytest.mark.parametrize("objective,ndcg_at", KINDS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_device_is_the_host_rule(model, layout, objective, ndcg_at):
    group = LAYOUTS[layout]
    s, y = R.scores_and_labels(group, seed=len(group) + 3)
    want = cpp.rank_gradient_host(s, y, group, objective, ndcg_at)
    r = model.rank_gradient(s, y, group, objective, ndcg_at)
    assert sorted(r) == ["grad", "hess", "loss", "ndcg", "pairs", "positions"]
    _same(r, want, (layout, objective, ndcg_at, "numpy"))
    _check_loss(r, want, s, y, group, objective, (layout, objective, ndcg_at))
    again = model.rank_gradient(s, y, group, objective, ndcg_at)
    _same(again, want, "again")
    assert np.float64(again["loss"]).tobytes() == np.float64(r["loss"]).tobytes()
    # device tuples in, DLPack capsules out
    ts, ds = _dev(s)
    ty, dy = _dev(y)
    rd = model.rank_gradient(ds, dy, group, objective, ndcg_at)
    assert not isinstance(rd["grad"], np.ndarray)
    _same(rd, want, (layout, objective, ndcg_at, "device"))
    assert np.float64(rd["loss"]).tobytes() == np.float64(r["loss"]).tobytes()
    # objective_gradient forwards
    g, loss = model.objective_gradient(s, y, objective, group=group, ndcg_at=ndcg_at)
    assert g.tobytes() == want["grad"].tobytes() and np.float64(loss).tobytes() == np.float64(r["loss"]).tobytes()
    del ts, ty


@pytest.mark.parametrize("case", R.constructed(), ids=lambda c: c[0])
def test_constructed_cases(model, case):
    name, s, y, group = case
    for objective, ks in (("pairwise", [None]), ("lambdarank", [None, 1, 3, 2000])):
        for k in ks:
            want = cpp.rank_gradient_host(s, y, group, objective, k)
            r = model.rank_gradient(s, y, group, objective, k)
            _same(r, want, (name, objective, k))
            _check_loss(r, want, s, y, group, objective, (name, objective, k))
    if name in ("all_labels_zero", "all_labels_equal"):
        assert model.rank_gradient(s, y, group, "pairwise")["loss"] == 0.0      # P == 0


def test_refusals_leave_the_model_as_it_was(tmp_path):
    rng = np.random.default_rng(5)
    m = _model()
    X = rng.standard_normal((64, 4)).astype(f32)
    m.step(X, None, rng.standard_normal(64).astype(f32))
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    before = p.read_bytes()
    group = [3, 61]
    s, y = R.scores_and_labels(group, seed=1)
    for v in (np.nan, np.inf, -np.inf):
        for objective in ("pairwise", "lambdarank"):
            sb = s.copy(); sb[40] = v
            with pytest.raises(RuntimeError, match="not finite"):
                m.rank_gradient(sb, y, group, objective)
    yb = y.copy(); yb[7] = 31; yb[50] = -2
    with pytest.raises(RuntimeError, match=r"label 31 \(row 7\)"):
        m.rank_gradient(s, yb, group)
    ty, dy = _dev(yb)
    with pytest.raises(RuntimeError, match=r"label 31 \(row 7\)"):
        m.rank_gradient(s, dy, group)
    big = np.zeros(1028, f32)
    with pytest.raises(RuntimeError, match=r"group\[1\] = 1025 \(query 1\)"):
        m.rank_gradient(big, np.zeros(1028, np.int32), [3, 1025])
    with pytest.raises(RuntimeError, match="sum to 63"):
        m.rank_gradient(s, y, [3, 60])
    assert m.save(str(p)) == 0 and p.read_bytes() == before
    r = m.rank_gradient(s, y, group)        # and the next call is served
    assert r["grad"].tobytes() == cpp.rank_gradient_host(s, y, group, "lambdarank")["grad"].tobytes()


def _grower(F, policy, depth):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=1, policy_dim=1, max_depth=depth, n_bins=32, split_score_func="L2", generator_type="Quantile", grow_policy=policy,
                      device="cpu", batch_size=5000)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=1)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


@pytest.mark.parametrize("generic", ["0", "1"])
@pytest.mark.parametrize("objective,ndcg_at", KINDS)
@pytest.mark.parametrize("policy,depth", [("oblivious", 1), ("oblivious", 3), ("oblivious", 6), ("greedy", 1), ("greedy", 3), ("greedy", 6)])
def test_newton_leaves_from_the_rank_buffers(policy, depth, objective, ndcg_at, generic):
    F, group = 6, R.LAYOUT
    rng = np.random.default_rng(depth)
    n = int(np.sum(group))
    X = rng.standard_normal((n, F)).astype(f32)
    s, y = R.scores_and_labels(group, seed=depth + 11)
    m = _grower(F, policy, depth)
    ds = m.prepare_dataset(X)
    m.step_prepared(ds, (np.sign(X[:, 0]) + 0.5 * np.sign(X[:, 1]) + 0.1 * X[:, 2]).astype(f32))
    before = np.asarray(m.get_ensemble_data()["values"], f32).copy()
    want = cpp.rank_gradient_host(s, y, group, objective, ndcg_at)
    os.environ["GBRL_HIP_CONTINUE_GENERIC"] = generic
    try:
        m.set_profiling(2)
        r = m.newton_leaves_prepared(ds, s, y, objective, leaf_l2=1.0, group=group, ndcg_at=ndcg_at)
        phases = m.last_phase_times()
        m.set_profiling(0)
    finally:
        os.environ.pop("GBRL_HIP_CONTINUE_GENERIC", None)
    if generic == "1":
        assert phases["newton_streamed"] == 0.0      # the general kernel took the sums
    elif policy == "oblivious":
        assert phases["newton_streamed"] == 1.0      # ... and here the streaming kernel
    bits = cpp.newton_sum_bits(n, float(max(group)))
    assert r["bits"] == bits == 62 - n.bit_length() - 10 or r["bits"] == bits == 40
    leaves = np.asarray(m.predict_leaves(X, None)).reshape(n)
    NL = r["sums"].shape[0]
    scale = 2.0 ** bits
    sums = np.zeros((NL, 3), np.int64)
    qg = np.rint(want["grad"].astype(np.float64) * scale).astype(np.int64)
    qh = np.rint(want["hess"].astype(np.float64) * scale).astype(np.int64)
    leaves = leaves.astype(np.int64)       # (the first tree: its global leaf indices start at 0)
    assert leaves.min() >= 0 and leaves.max() < NL
    np.add.at(sums[:, 0], leaves, qg)
    np.add.at(sums[:, 1], leaves, qh)
    np.add.at(sums[:, 2], leaves, 1)
    assert r["sums"].dtype == np.int64 and r["sums"].tobytes() == sums.tobytes(), (r["sums"][:4], sums[:4])
    ens = m.get_ensemble_data()
    depths = np.asarray(ens["depths"], np.int32)
    ld = np.full(NL, depths[0], np.int32) if policy == "oblivious" else depths[:NL]
    assert r["values"].tobytes() == cpp.newton_values_host(sums, bits, before[:NL].reshape(NL, 1), ld, 1.0).tobytes()
