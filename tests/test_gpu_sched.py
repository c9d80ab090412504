"""GPU tests of the Linear learning-rate scheduler (predict_sched.hip; scheduler.h:124-134, optimizer.cpp:110-118).

* the fixtures written by the reference's CPU build go through the product: structure bit-identical, leaf values / predictions / every
  tree range / fit loss and bias within the project's 1e-5 parity bar;
* the three kernels agree BIT FOR BIT on ensembles grown here: the streaming kernel (large batches; GBRL_HIP_PREDICT_SCHED_MIN_ROWS moves
  its 32 768-row boundary) and the chain stage (GBRL_HIP_PREDICT_CHAIN=1 / 0: always / never) against the general kernel
  (GBRL_HIP_PREDICT_GENERIC=1);
* a Linear optimizer with stop_lr == init_lr has lr(t) == init_lr exactly: its model predicts the bits of a Const twin, which ties the new
  kernels to the existing ones;
* fit()'s internal predictions are those of a plain predict; device tensors and DLPack give the bits of the NumPy route.
"""
import os

import numpy as np
import pytest

import cases as K
import sched_cases as S
from helpers import GOLDEN, assert_structure_equal, assert_values_close, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
HOOKS = ("GBRL_HIP_PREDICT_GENERIC", "GBRL_HIP_PREDICT_CHAIN", "GBRL_HIP_PREDICT_SCHED_MIN_ROWS", "GBRL_HIP_PREDICT_NOSPLIT")
MODES = {
    "default": {},
    "general": {"GBRL_HIP_PREDICT_GENERIC": "1"},
    # (NOSPLIT: one chain per row also where kern::predict would spread the trees of a small batch over block columns)
    "stream": {"GBRL_HIP_PREDICT_CHAIN": "0", "GBRL_HIP_PREDICT_SCHED_MIN_ROWS": "1", "GBRL_HIP_PREDICT_NOSPLIT": "1"},
    "chain": {"GBRL_HIP_PREDICT_CHAIN": "1", "GBRL_HIP_PREDICT_NOSPLIT": "1"},                 # (takes up to 16 384 rows)
    "no_fast": {"GBRL_HIP_PREDICT_CHAIN": "0", "GBRL_HIP_PREDICT_SCHED_MIN_ROWS": "1000000000"},
}


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = S.BY_NAME[name]
    X, Xc, G, y = K.make_inputs(case)
    assert K.inputs_digest(X, Xc, G, y) == str(g["inputs_sha256"]), "input synthesis drifted from the fixture"
    return case, g, (X, Xc, G, y)


def _predict(m, X, Xc, monkeypatch, mode, start=0, stop=0):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    out = np.asarray(m.predict(X, Xc, start, stop)).copy()
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    return out


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_product_matches_reference_sched_golden(name, monkeypatch):
    import gbrl_amd
    case, g, (X, Xc, G, y) = load_golden(name)
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
    pred = np.asarray(K.drive(m, case, X, Xc, G, y))
    e = m.get_ensemble_data()
    assert m.get_num_trees() == int(g["n_trees"]) and m.get_iteration() == int(g["iteration"])
    assert_structure_equal(e, g, what=name + ": ")
    scale = float(np.abs(y).mean())
    assert_values_close(e, g, scale, TOL, what=name + ": ")
    assert rel_err(pred.reshape(g["pred"].shape), g["pred"], scale) <= TOL
    assert case["pred_ranges"]
    for a, b in case["pred_ranges"]:
        want = g["pred_%d_%d" % (a, b)]
        for mode in ("default", "general", "stream", "chain"):      # every kernel, at the ABSOLUTE tree indices of the range
            got = _predict(m, X, Xc, monkeypatch, mode, a, b)
            assert rel_err(got.reshape(want.shape), want, scale) <= TOL, (name, a, b, mode)
    got, want = np.asarray(m.get_scheduler_lrs(), np.float32), g["scheduler_lrs"]
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want))


@pytest.mark.parametrize("name", [c["name"] for c in S.FIT_CASES])
def test_fit_matches_reference_sched_golden(name):
    import gbrl_amd
    case, g, (X, Xc, G, y) = load_golden(name)
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
    loss, pred = K.drive_fit(m, case, X, y, Xc)
    e = m.get_ensemble_data()
    assert m.get_num_trees() == int(g["n_trees"]) == case["fit_iterations"] and m.get_iteration() == int(g["iteration"])
    assert_structure_equal(e, g)
    scale = float(np.abs(y).mean())
    assert_values_close(e, g, scale, TOL)
    assert rel_err(np.asarray(m.get_bias()), g["bias"], scale) <= TOL
    assert rel_err(pred, g["pred"], scale) <= TOL
    assert abs(loss - float(g["fit_loss"])) <= TOL * max(1.0, abs(float(g["fit_loss"])))


# ---------------------------------------------------------------------------------------------------- bitwise agreement between paths
def _opts(D, kind):
    if kind == "linear" or D == 1:
        return [S._lin(0.3, 0.04, 9, 0, D)]
    if kind == "mixed":      # actor-critic: Const policy range, Linear value range
        return [S._const(0.1, 0, D - 1), S._lin(0.05, 0.004, 6, D - 1, D)]
    return [S._lin(0.02, 0.3, 11, 0, D // 2), S._const(0.07, D // 2, D)]      # "mixed2": a rising schedule first


def _grown(policy, depth, D, F, Fc, trees, seed, opts, device="cpu"):
    import gbrl_amd
    case = dict(name="sch", seed=seed, N=2500, F=F, Fc=Fc, D=D, depth=depth, n_bins=64, score="Cosine" if D > 1 else "L2", gen="Quantile",
                policy=policy, trees=trees, opts=opts, loop="rmse")
    X, Xc, G, y = K.make_inputs(case)
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case, device=device))
    if device == "cpu":      # host buffers in, NumPy out (compute is on the GPU regardless)
        K.drive(m, case, X, Xc, G, y)
    else:                    # torch device tensors in as 4-tuples, DLPack out
        import torch
        keep = []

        def to_input(a):
            t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
            keep.append(t)
            return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
        K.drive(m, case, X, Xc, G, y, to_input=to_input, to_numpy=lambda c: c if isinstance(c, np.ndarray) else torch.from_dlpack(c).cpu().numpy())
    assert m.get_num_trees() == trees
    return m, case


def _batch(case, n, seed):
    big = dict(case, N=n, seed=seed)
    X, Xc, _, _ = K.make_inputs(big)
    return X, Xc


SHAPES = [   # policy, depth, D, F, Fc, trees, optimizer kind
    ("oblivious", 1, 1, 4, 0, 5, "linear"), ("oblivious", 3, 5, 12, 0, 9, "mixed"), ("oblivious", 4, 8, 16, 2, 14, "mixed"),
    ("oblivious", 6, 8, 32, 0, 15, "mixed2"), ("oblivious", 8, 16, 9, 0, 6, "mixed"), ("oblivious", 5, 40, 8, 0, 7, "mixed2"),
    ("greedy", 1, 5, 4, 0, 6, "mixed"), ("greedy", 2, 1, 7, 1, 8, "linear"), ("greedy", 4, 8, 16, 0, 12, "mixed"),
    ("greedy", 5, 16, 12, 2, 9, "mixed2"), ("greedy", 5, 40, 8, 0, 5, "linear"), ("greedy", 3, 8, 128, 0, 10, "mixed"),
]


@pytest.mark.parametrize("policy,depth,D,F,Fc,trees,kind", SHAPES)
def test_fast_paths_are_bitwise_the_general_kernel(policy, depth, D, F, Fc, trees, kind, monkeypatch):
    m, case = _grown(policy, depth, D, F, Fc, trees, 9000 + 13 * depth + D + F, _opts(D, kind))
    # rows around the tile sizes of the streaming kernel (128 / 256) and the chain path's limit, ragged last tiles
    for n in (1, 63, 129, 1500, 8192, 8193):
        X, Xc = _batch(case, n, 77 + n)
        ranges = [(0, 0), (1, trees - 1), (trees - 1, trees)] if n in (129, 8193) else [(0, 0)]
        for a, b in ranges:
            want = _predict(m, X, Xc, monkeypatch, "general", a, b)
            assert _same(_predict(m, X, Xc, monkeypatch, "stream", a, b), want), ("stream", n, a, b)
            assert _same(_predict(m, X, Xc, monkeypatch, "chain", a, b), want), ("chain", n, a, b)
            assert _same(_predict(m, X, Xc, monkeypatch, "default", a, b), want), ("default", n, a, b)


@pytest.mark.parametrize("policy,depth,D,F,Fc,trees,kind", [SHAPES[2], SHAPES[3], SHAPES[8], SHAPES[11]])
def test_dispatch_boundaries_by_default(policy, depth, D, F, Fc, trees, kind, monkeypatch):
    """Without hooks: 32 767 rows stay with the general kernel, 32 768 go to the streaming kernel; the same bits on both sides, and
    the same bits as with each path forced."""
    m, case = _grown(policy, depth, D, F, Fc, trees, 9100 + depth + D, _opts(D, kind))
    X, Xc = _batch(case, 32768 + 200, 5)
    full = _predict(m, X, Xc, monkeypatch, "general")
    for n in (32767, 32768, 32768 + 200):
        xs, xcs = X[:n], (None if Xc is None else Xc[:n])
        got = _predict(m, xs, xcs, monkeypatch, "default")
        assert _same(got, full[:n]), n
        assert _same(_predict(m, xs, xcs, monkeypatch, "no_fast"), got), n
        assert _same(_predict(m, xs, xcs, monkeypatch, "stream", 2, trees - 1), _predict(m, xs, xcs, monkeypatch, "general", 2, trees - 1)), n


def test_optimizers_that_share_outputs_use_the_general_kernel(monkeypatch):
    """Two optimizers on the same outputs (two updates per tree and output): no fast path takes it, whatever the hooks say."""
    opts = [S._lin(0.2, 0.02, 5, 0, 3), S._const(0.05, 1, 3)]
    m, case = _grown("oblivious", 3, 3, 6, 0, 8, 4242, opts)
    X, Xc = _batch(case, 3000, 9)
    want = _predict(m, X, Xc, monkeypatch, "general")
    e = m.get_ensemble_data()
    # ... and the general kernel is the chain of optimizer.cpp:110-118, restated here in float64 (1e-5: float32 against float64)
    lr0 = [float(np.asarray(gbrl_lr(opts[0], t))) for t in range(8)]
    ref = np.tile(np.asarray(m.get_bias(), np.float64), (3000, 1))
    ti, dep = np.asarray(e["tree_indices"]), np.asarray(e["depths"])
    fi, fv, vals = np.asarray(e["feature_indices"]).reshape(8, -1), np.asarray(e["feature_values"]).reshape(8, -1), np.asarray(e["values"]).reshape(-1, 3)
    for t in range(8):
        leaf = np.zeros(3000, np.int64)
        for d in range(dep[t]):
            leaf |= (X[:, fi[t, d]] > fv[t, d]).astype(np.int64) << (dep[t] - 1 - d)
        v = vals[ti[t] + leaf].astype(np.float64)
        ref[:, 0:3] -= lr0[t] * v[:, 0:3]
        ref[:, 1:3] -= 0.05 * v[:, 1:3]
    assert rel_err(want, ref.astype(np.float32), 1.0) <= TOL
    for mode in ("default", "stream", "chain"):
        assert _same(_predict(m, X, Xc, monkeypatch, mode), want), mode


def gbrl_lr(o, t):
    f = np.float32
    T_, t_ = f(o["T"]), f(t) + f(1)
    lr = f(f(o["init_lr"]) + f(f(f(1) - f((T_ - t_) / T_)) * f(f(o["stop_lr"]) - f(o["init_lr"]))))
    return f(o["stop_lr"]) if lr < f(o["stop_lr"]) else lr


# ---------------------------------------------------------------------------------------------------- degenerate schedule
def _twins(policy, depth, D, F, trees, seed, N):
    """A model with Linear(stop_lr == init_lr) optimizers and a Const twin, stepped on the same batches."""
    import gbrl_amd
    lin = [S._lin(0.1, 0.1, 50, 0, D - 1), S._lin(0.03, 0.03, 7, D - 1, D)]
    con = [S._const(0.1, 0, D - 1), S._const(0.03, D - 1, D)]
    out = []
    for opts in (lin, con):
        case = dict(name="twin", seed=seed, N=N, F=F, Fc=0, D=D, depth=depth, n_bins=64, score="Cosine", gen="Quantile", policy=policy, trees=trees,
                    opts=opts, loop="rmse")
        X, Xc, G, y = K.make_inputs(case)
        m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
        K.drive(m, case, X, Xc, G, y)
        out.append(m)
    return out[0], out[1], case


@pytest.mark.parametrize("policy,depth,trees,rows", [("oblivious", 6, 15, 4096), ("greedy", 5, 10, 4096), ("oblivious", 6, 15, 65536), ("greedy", 5, 10, 65536),
                                                     ("oblivious", 3, 500, 2048), ("greedy", 3, 500, 2048)])
def test_degenerate_schedule_predicts_the_bits_of_a_const_twin(policy, depth, trees, rows, monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    ml, mc, case = _twins(policy, depth, 8, 16, trees, 5150 + depth + trees, 2048)
    el, ec = ml.get_ensemble_data(), mc.get_ensemble_data()
    for k in K.ENSEMBLE_KEYS:      # step never reads the optimizer: the same trees
        assert np.array_equal(np.asarray(el[k]), np.asarray(ec[k])), k
    assert ml.get_optimizers()[0]["scheduler_func"] == "Linear" and mc.get_optimizers()[0]["scheduler_func"] == "Const"
    X, Xc = _batch(case, rows, 31)
    want = np.asarray(mc.predict(X, None, 0, 0)).copy()              # the existing kernels, as dispatched today
    assert _same(np.asarray(ml.predict(X, None, 0, 0)), want)
    a, b = trees // 3, trees - 1
    assert _same(np.asarray(ml.predict(X, None, a, b)), np.asarray(mc.predict(X, None, a, b)))
    if trees < 128:      # (beyond, the Const default for small batches sums partial tree ranges: another association)
        for mode in ("general", "stream"):
            assert _same(_predict(ml, X, None, monkeypatch, mode), want), mode


# ---------------------------------------------------------------------------------------------------- fit
def test_fit_sees_the_predictions_of_a_plain_predict(monkeypatch):
    """fit() predicts trees [0, i) for every batch.  With the chain stage forced for those predictions, with the streaming kernel
    forced and with the general kernel alone the grown model and the returned loss are identical: the gradients were the same bits."""
    import gbrl_amd
    rng = np.random.default_rng(21)
    N, F, D = 700, 5, 2
    X = rng.standard_normal((N, F), dtype=np.float32)
    y = (np.tanh(X[:, :D]) + 0.2 * rng.standard_normal((N, D), dtype=np.float32)).astype(np.float32)
    out = []
    for mode in ("chain", "stream", "general"):
        for h in HOOKS:
            monkeypatch.delenv(h, raising=False)
        for k, v in MODES[mode].items():
            monkeypatch.setenv(k, v)
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=3, min_data_in_leaf=0, n_bins=32, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=256, grow_policy="oblivious",
                          verbose=0, device="cpu", learner_name="fitsched")
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Linear", init_lr=0.3, start_idx=0, stop_idx=D, stop_lr=0.01, T=90)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        loss = m.fit(X, None, y, 120, False, "MultiRMSE")
        out.append((loss, m.get_ensemble_data(), _predict(m, X, None, monkeypatch, "general")))
    for loss, e, p in out[1:]:
        assert loss == out[0][0]
        for k in K.ENSEMBLE_KEYS:
            assert np.array_equal(np.asarray(e[k]), np.asarray(out[0][1][k])), k
        assert _same(p, out[0][2])
    # the loss fit() returns is the MultiRMSE of a plain predict over all trees
    want = np.sqrt(0.5 * float(((out[0][2].reshape(N, -1) - y).astype(np.float64) ** 2).sum()) / N)
    assert abs(out[0][0] - want) <= 1e-5 * max(1.0, want)


# ---------------------------------------------------------------------------------------------------- device tensors
@pytest.mark.parametrize("rows", [700, 40000])
def test_device_tensors_and_dlpack_give_the_bits_of_the_numpy_route(rows, monkeypatch):
    import torch
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    m, case = _grown("greedy", 4, 8, 16, 0, 12, 8888, _opts(8, "mixed"))                       # host buffers in, NumPy out
    md, _ = _grown("greedy", 4, 8, 16, 0, 12, 8888, _opts(8, "mixed"), device="cuda")          # device tensors in, DLPack out
    X, _ = _batch(case, rows, 3)
    t = torch.from_numpy(X).to("cuda:0")
    for a, b in ((0, 0), (3, 11)):
        want = np.asarray(m.predict(X, None, a, b)).copy()
        got = md.predict((t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda"), None, a, b)
        assert not isinstance(got, np.ndarray)
        got = torch.from_dlpack(got).cpu().numpy()
        assert _same(np.asarray(got).reshape(want.shape), want), (a, b)


# ---------------------------------------------------------------------------------------------------- long ensembles
# The relay (k_sched_relay) applies 64 trees per batch, four waves take turns and a wave requests its next batches while the others
# apply theirs: only ensembles of several hundred trees run its later rounds.  And small batches against 128 .. 2048 trees (or very few
# rows against more) do NOT run one chain per row by default: like a Const ensemble they sum partial chains over tree slices
# (kern::predict), which is within 1e-5 of the chain but not its bits.  Both are checked here with schedules that really vary.
_LONG = {}


def _long_model(policy):
    """2500 oblivious / 700 greedy trees grown by the rmse loop; two falling schedules, one of them clamped from 60 % of the trees on."""
    if policy not in _LONG:
        trees = 2500 if policy == "oblivious" else 700
        opts = [S._lin(0.2, 0.01, int(trees * 0.6), 0, 4), S._lin(0.08, 0.01, trees + 50, 4, 5)]
        _LONG[policy] = _grown(policy, 3, 5, 12, 0, trees, 777, opts) + (trees, opts)
    return _LONG[policy]


def _slices(n, trees, D, par_th=10):
    """The tree slices kern::predict gives a batch of n rows over `trees` trees (predict): None = one chain per row."""
    row_tiles = (n + 255) // 256
    if n > 64 * 256 or trees < 128:
        return None
    partial_floats = min(64 * n * D, 16 << 20)
    chain_first = n <= 1024      # (those batches take the exact chain, whatever the tree count from 128 on)
    k = chunk = 0
    if trees <= 2048 and row_tiles <= 64 and not chain_first:
        splits = min(64, trees // 32, max(1, 512 // row_tiles))
        while splits > 1 and splits * n * D > partial_floats:
            splits -= 1
        if splits > 1:
            chunk = (trees + splits - 1) // splits
            k = (trees + chunk - 1) // chunk
    elif trees > 2048:
        thr = max(1, min(64, trees // par_th))
        if n // par_th <= 1 and thr > 1 and thr * n * D <= partial_floats:
            k, chunk = thr, trees // thr
    if k <= 1:
        return None
    return [(i * chunk, trees if i == k - 1 else (i + 1) * chunk) for i in range(k)]


def test_slices_restatement_covers_both_sides_of_every_boundary():
    assert _slices(1024, 500, 5) is None and _slices(1025, 500, 5) is not None
    assert _slices(3000, 127, 5) is None and len(_slices(3000, 128, 5)) == 4
    assert _slices(3000, 2048, 5) is not None and _slices(3000, 2049, 5) is None
    assert len(_slices(15, 2500, 5)) == 64 and _slices(19, 2500, 5) is not None and _slices(20, 2500, 5) is None
    assert _slices(16384, 500, 5) is not None and _slices(16385, 500, 5) is None
    s = _slices(3000, 500, 5)
    assert s[0][0] == 0 and s[-1][1] == 500 and all(a[1] == b[0] for a, b in zip(s, s[1:]))


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_relay_over_many_batches_is_bitwise_the_general_kernel(policy, monkeypatch):
    m, case, trees, _ = _long_model(policy)
    ranges = [(0, 0), (3, 303), (100, trees - 100), (trees // 2 + 17, trees), (trees - 65, trees - 1), (7, 7 + 128), (1, 1 + 129)]
    for n in (700, 1024, 1025, 4000, 8192, 8193):
        X, Xc = _batch(case, n, 1000 + n)
        for a, b in (ranges if n in (1025, 8192) else ranges[:4]):
            want = _predict(m, X, Xc, monkeypatch, "general", a, b)
            assert _same(_predict(m, X, Xc, monkeypatch, "chain", a, b), want), ("chain", n, a, b)
            assert _same(_predict(m, X, Xc, monkeypatch, "stream", a, b), want), ("stream", n, a, b)
            t = (b if b else trees) - a
            got = _predict(m, X, Xc, monkeypatch, "default", a, b)
            if _slices(n, t, 5) is None:      # default dispatch: the relay up to 8192 rows (from 512 trees; 128 up to 1024 rows), else the general kernel
                assert _same(got, want), ("default", n, a, b)
            else:
                assert rel_err(got, want, 1.0) <= TOL, ("default, tree slices", n, a, b)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_tree_slices_of_small_batches_with_a_varying_schedule(policy, monkeypatch):
    """Rows on both sides of 1024 and 16 384, tree counts on both sides of 128 and 2048, ranges that start inside the ensemble.  Where
    kern::predict slices the trees, the result is bias + the slices' chains added in tree order: restated here from the general
    kernel's predictions of each slice with a zero bias (a chain that starts at 0), bit for bit; and within 1e-5 of the one chain."""
    m, case, trees, _ = _long_model(policy)
    bias = np.array([0.37, -1.25, 0.004, 2.5, -0.61], np.float32)
    zero = np.zeros(5, np.float32)
    shapes = [(1024, 500), (1025, 500), (3000, 127), (3000, 128), (3000, 500), (2048, 333), (16384, 600), (16385, 600), (9000, 129), (15, 640)]
    if trees > 2049:
        shapes += [(3000, 2048), (3000, 2049), (15, 2300), (19, 2500), (20, 2500), (1500, 2048)]
    sliced = 0
    for n, t in shapes:
        X, Xc = _batch(case, n, 2000 + n + t)
        for a in sorted({0, 41, trees - t}):
            b = a + t
            if b > trees:
                continue
            m.set_bias(bias)
            want = _predict(m, X, Xc, monkeypatch, "general", a, b)
            got = _predict(m, X, Xc, monkeypatch, "default", a, b)
            assert rel_err(got, want, 1.0) <= TOL, (n, a, b)
            sl = _slices(n, t, 5)
            if sl is None:
                assert _same(got, want), (n, a, b)
                continue
            sliced += 1
            m.set_bias(zero)
            acc = np.broadcast_to(np.float32(0.0) + bias, (n, 5)).astype(np.float32)
            for s0, s1 in sl:
                acc = (acc + _predict(m, X, Xc, monkeypatch, "general", a + s0, a + s1).reshape(n, 5)).astype(np.float32)
            m.set_bias(bias)
            assert _same(got.reshape(n, 5), acc), ("slice sums", n, a, b, len(sl))
    m.set_bias(zero)
    assert sliced >= 8


def test_get_scheduler_lrs_follows_the_recording_tree_by_tree():
    """get_scheduler_lrs() after every step against the reference's values at the same tree counts (tests/golden/sched_recordings.npz)."""
    import gbrl_amd
    rec = np.load(os.path.join(GOLDEN, "sched_recordings.npz"))
    rng = np.random.default_rng(7)
    X = K._normalish(rng, (64, 3))
    G = K._normalish(rng, (64, 2))
    for name, opts in S.LRS_SCHEDULES.items():
        want = rec["lrs_" + name]
        m = gbrl_amd.GBRL(**S.LRS_KW)
        m.set_feature_weights(np.ones(3, np.float32))
        for o in opts:
            m.set_optimizer(**o)
        m.set_feature_mapping(np.arange(3, dtype=np.int32), np.array([True] * 3, dtype=bool))
        for t in range(S.LRS_TREES + 1):
            got = np.asarray(m.get_scheduler_lrs(), np.float32)
            assert m.get_num_trees() == t
            assert np.all(np.abs(got - want[t]) <= 1e-6 * np.abs(want[t])), (name, t, got, want[t])
            if t < S.LRS_TREES:
                m.step(X, None, G.copy())
