"""Permutation importance on a prepared data set, on the GPU (GBRL.permutation_importance_prepared; include/gbrl_hip.h, "Feature importance").

The oracle is built from calls that existed before it.  For a variant (c, r) the shuffled observations are materialised on the host,
    Xp = X.copy(); Xp[:, c] = X[gbrl_cpp.permutation_host(n, seed, c, r), c]; dsp = m.prepare_dataset(Xp, reference=ds)
(binning is per cell, so dsp's codes are ds's with column c permuted), and the expected loss is valid_loss[0] of the zero-iteration call
fit_prepared(ds_train, y_train, 0, valid=dsp, valid_targets=y, objective=, alpha=), which grows nothing and evaluates the model as it stands (the
first test confirms that it leaves the file bytes unchanged).  For rmse that equals staged_loss(Xp, None, y, stops=[T])[0], asserted too.

Every comparison is BIT equality, for all four objectives: the new kernels write the one-partial-per-64-rows reduction the validation launch writes
and the finishing sum is the same kernel, so no objective falls back to the reordering bound n * 2^-53.

Shapes: the rows of the evaluated data set n in {1, 63, 64, 65, 257, 4097} (tile edges, and enough blocks for the finishing sum to matter) on a model
grown on 512 other rows with the same thresholds; F in {1, 16, 17, 40} with the shuffled column at 0, 15, 16 and F - 1 (both sides of the 32-byte
record boundary); D in {1, 3, 8}; oblivious depth 3 and greedy depth 4; T in {1, 7, 40}; rmse, logistic, softmax, quantile with a vector alpha; one
case with more (column, repeat) variants than a launch takes (permutation_geometry()).  The targets lean on the tested columns, so that the trees
use them: at least half of the tested columns must be used (asserted from get_ensemble_data(): a condition on the inputs, not a tolerance).
"""
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp

N_TRAIN, SEED = 512, 11


def _model(F, D, policy, lr=0.1, n_bins=32):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=3 if policy == "oblivious" else 4, n_bins=n_bins,
                      split_score_func="L2" if policy == "oblivious" else "Cosine", generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=N_TRAIN)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=lr, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _tested(F):
    return sorted({c for c in (0, 15, 16, F - 1) if 0 <= c < F})


def _data(rows, F, D, objective, rng, W):
    X = rng.standard_normal((rows, F)).astype(np.float32)
    S = X @ W + 0.2 * rng.standard_normal((rows, D))
    if objective == "logistic":
        Y = (1.0 / (1.0 + np.exp(-S)) > rng.random((rows, D))).astype(np.float32)
    elif objective == "softmax":
        return X, np.argmax(S + 0.3 * rng.standard_normal((rows, D)), axis=1).astype(np.int32)
    else:
        Y = S.astype(np.float32)
    return X, (np.ascontiguousarray(Y[:, 0]) if D == 1 else np.ascontiguousarray(Y))


class Case:
    """A model grown by fit_prepared on N_TRAIN rows, and n other rows under the same thresholds to measure the importance on."""

    def __init__(self, n, F, D, policy, T, objective, flat=False, lr=0.1):
        self.n, self.F, self.D, self.T, self.objective = n, F, D, T, objective
        rng = np.random.default_rng(1000 * n + 10 * F + D + T)
        w = np.full(F, 1.0 if flat else 0.4)
        if not flat:
            for c, s in zip(_tested(F), (3.0, 2.5, 2.0, 1.5)):
                w[c] = s
        W = w[:, None] * rng.choice([-1.0, 1.0], size=(F, D))
        self.alpha = np.linspace(0.15, 0.85, D).astype(np.float32) if objective == "quantile" else None
        self.kw = dict(objective=objective) if self.alpha is None else dict(objective=objective, alpha=self.alpha)
        self.m = _model(F, D, policy, lr)
        self.Xt, self.yt = _data(N_TRAIN, F, D, objective, rng, W)
        self.X, self.y = _data(n, F, D, objective, rng, W)
        self.ds_train = self.m.prepare_dataset(self.Xt)
        self.m.fit_prepared(self.ds_train, self.yt, T, **self.kw)
        assert self.m.get_num_trees() == T
        self.ds = self.m.prepare_dataset(self.X, reference=self.ds_train)
        e = self.m.get_ensemble_data()
        depths, fidx = np.asarray(e["depths"]), np.asarray(e["feature_indices"])
        live = np.arange(fidx.shape[1])[None, :] < depths[:, None]
        self.used = set(int(f) for f in fidx[live])

    def oracle(self, c=None, r=0, seed=SEED):
        Xp = self.X.copy()
        if c is not None:
            Xp[:, c] = self.X[cpp.permutation_host(self.n, seed, c, r), c]
        dsp = self.m.prepare_dataset(Xp, reference=self.ds_train)
        out = self.m.fit_prepared(self.ds_train, self.yt, 0, valid=dsp, valid_targets=self.y, **self.kw)
        assert out["iterations"] == 0 and out["valid_loss"].shape == (1,)
        return np.float64(out["valid_loss"][0]), Xp

    def run(self, **kw):
        args = dict(n_repeats=2, seed=SEED)
        args.update(self.kw)
        args.update(kw)
        return self.m.permutation_importance_prepared(self.ds, self.y, **args)


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


CASES = [
    # n, F, D, policy, T, objective
    (1, 1, 1, "oblivious", 1, "rmse"),
    (63, 16, 3, "greedy", 7, "logistic"),
    (64, 17, 8, "oblivious", 40, "softmax"),
    (65, 40, 3, "greedy", 40, "quantile"),
    (257, 17, 1, "oblivious", 7, "rmse"),
    (4097, 40, 8, "greedy", 7, "rmse"),
    (4097, 16, 3, "oblivious", 40, "logistic"),
    (257, 40, 8, "oblivious", 1, "quantile"),
    (65, 1, 3, "greedy", 1, "softmax"),
    (4097, 17, 1, "greedy", 40, "quantile"),
]


@pytest.mark.parametrize("n,F,D,policy,T,objective", CASES)
def test_losses_equal_the_oracle_bit_for_bit(n, F, D, policy, T, objective, tmp_path):
    k = Case(n, F, D, policy, T, objective)
    m, tested = k.m, _tested(F)
    assert 2 * len([c for c in tested if c in k.used]) >= len(tested), (tested, sorted(k.used))
    file0, codes0 = _file(m, tmp_path), k.ds.codes().tobytes()
    # ---- the zero-iteration fit is an evaluation: it leaves the model as it was
    base, _ = k.oracle()
    assert _file(m, tmp_path) == file0
    # ---- every column, two repeats; then the same call again and through the general kernel
    r = k.run()
    assert sorted(r) == ["baseline", "cols", "importance", "loss", "mean", "std"]
    assert r["loss"].dtype == np.float64 and r["loss"].shape == (F, 2) and r["cols"].tolist() == list(range(F)) and isinstance(r["baseline"], float)
    print("baseline %.17g  oracle %.17g" % (r["baseline"], base))
    assert _same(r["baseline"], base)
    for c in tested:
        for rep in range(2):
            want, Xp = k.oracle(c, rep)
            print("col %d repeat %d  loss %.17g  oracle %.17g" % (c, rep, r["loss"][c, rep], want))
            assert _same(r["loss"][c, rep], want), (c, rep, r["loss"][c, rep], want)
            if objective == "rmse":
                assert _same(want, np.asarray(m.staged_loss(Xp, None, k.y, stops=[T]), np.float64)[0])
    for c in range(F):
        if c not in k.used:
            assert _same(r["loss"][c], [base, base]), c
    assert _same(r["importance"], r["loss"] - r["baseline"]) and _same(r["mean"], r["importance"].mean(axis=1))
    assert np.allclose(r["std"], r["importance"].std(axis=1), rtol=1e-12, atol=0)
    again = k.run()
    with _env("GBRL_HIP_PERM_GENERIC", "1"):
        general = k.run()
    for key in ("baseline", "loss", "importance", "mean", "std"):
        assert _same(again[key], r[key]) and _same(general[key], r[key]), key
    # ---- a column subset is those rows of the full call
    if F >= 10:
        sub = k.run(cols=[3, 9])
        assert sub["cols"].tolist() == [3, 9] and _same(sub["loss"], r["loss"][[3, 9]]) and _same(sub["baseline"], r["baseline"])
    one = k.run(cols=[tested[-1]], n_repeats=1)
    assert _same(one["loss"], r["loss"][tested[-1], :1])
    # ---- n_trees = k: the model truncated there (rmse: staged_loss is the oracle of a prefix)
    if T > 1:
        kt = T // 2
        part = k.run(n_trees=kt, cols=tested)
        assert not _same(part["baseline"], r["baseline"])
        if objective == "rmse":
            assert _same(part["baseline"], np.asarray(m.staged_loss(k.X, None, k.y, stops=[kt]), np.float64)[0])
            for i, c in enumerate(tested):
                Xp = k.X.copy()
                Xp[:, c] = k.X[cpp.permutation_host(n, SEED, c, 1), c]
                assert _same(part["loss"][i, 1], np.asarray(m.staged_loss(Xp, None, k.y, stops=[kt]), np.float64)[0]), c
        assert _same(k.run(n_trees=T, cols=tested)["loss"], r["loss"][tested])
    # ---- nothing was written: the patched tile lives on chip only
    assert _file(m, tmp_path) == file0 and k.ds.codes().tobytes() == codes0


def test_more_variants_than_one_launch_takes(tmp_path):
    """17 columns x 5 repeats on a model that uses at least 13 of them: the launches' variant count (64) is crossed, and the variants behind the
    boundary equal the oracle like the ones in front of it"""
    geo = cpp.permutation_geometry()
    k = Case(257, 17, 3, "oblivious", 40, "rmse", flat=True, lr=0.5)
    used = sorted(k.used)
    assert len(used) * 5 + 1 > geo["launch_variants"], used
    r = k.run(n_repeats=5)
    assert r["loss"].shape == (17, 5)
    base, _ = k.oracle()
    assert _same(r["baseline"], base)
    for c in (used[0], used[len(used) // 2], used[-2], used[-1]):     # the first launch, and the last used column, whose repeats end behind variant 64
        for rep in range(5):
            want, _ = k.oracle(c, rep)
            assert _same(r["loss"][c, rep], want), (c, rep)
    with _env("GBRL_HIP_PERM_GENERIC", "1"):
        assert _same(k.run(n_repeats=5)["loss"], r["loss"])
    other = k.run(n_repeats=5, seed=SEED + 1)
    assert _same(other["baseline"], r["baseline"]) and not _same(other["loss"], r["loss"])


def test_the_column_the_target_is_made_of_ranks_first():
    F, n = 8, 2000
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, F)).astype(np.float32)
    y = (3.0 * X[:, 0] + 0.1 * rng.standard_normal(n)).astype(np.float32)
    m = _model(F, 1, "oblivious")
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, y, 30)
    r = m.permutation_importance_prepared(ds, y)
    assert r["loss"].shape == (F, 5) and int(np.argmax(r["mean"])) == 0 and r["mean"][0] > 0 and (r["importance"][0] > 0).all()
    split = m.feature_importance("split")
    cover = m.feature_importance("cover", m.leaf_counts(X, None))
    assert int(np.argmax(split)) == 0 and int(np.argmax(cover)) == 0
    assert cover.sum() == n * np.asarray(m.get_ensemble_data()["depths"]).sum()      # every row meets every level of every oblivious tree


def test_refusals(tmp_path):
    k = Case(65, 17, 3, "oblivious", 7, "rmse")
    m, ds, y, F = k.m, k.ds, k.y, k.F
    file0 = _file(m, tmp_path)
    P = m.permutation_importance_prepared

    def refused(word, *a, **kw):
        with pytest.raises(RuntimeError, match=word):
            P(*a, **kw)

    refused("n_repeats must be >= 1", ds, y, n_repeats=0)
    refused("cols must name between 1 and 17", ds, y, cols=[])
    refused("strictly ascending", ds, y, cols=[3, 3])
    refused("strictly ascending", ds, y, cols=[9, 3])
    refused(r"outside \[0, 17\)", ds, y, cols=[3, F])
    refused(r"outside \[0, 17\)", ds, y, cols=[-1])
    refused("n_trees 0 is outside", ds, y, n_trees=0)
    refused("n_trees 8 is outside", ds, y, n_trees=8)
    refused("without targets", ds, None)
    refused("Expected targets of shape", ds, y[:-1])
    refused("Expected targets of shape", ds, np.zeros((65, 2), np.float32))
    refused("Expected array of format", ds, np.zeros(65, np.int32))
    refused("Expected array of format", ds, y, objective="softmax")          # softmax takes int32 labels
    refused("int32 class labels", ds, np.zeros(64, np.int32), objective="softmax")
    refused("ranking objectives", ds, np.zeros(65, np.int32), objective="pairwise")
    refused("ranking objectives", ds, np.zeros(65, np.int32), objective="lambdarank")
    refused("Invalid objective", ds, y, objective="mae")
    refused("alpha is the level table", ds, y, alpha=0.5)
    refused("needs alpha", ds, y, objective="quantile")
    refused("null data set", None, y)
    # a model without trees
    fresh = _model(F, 3, "oblivious")
    with pytest.raises(RuntimeError, match="the model has no trees"):
        fresh.permutation_importance_prepared(fresh.prepare_dataset(k.X), y)
    # what predict_continue_prepared refuses: another bin count, thresholds the trees do not compare against (the tree is named)
    with pytest.raises(RuntimeError, match="binned with n_bins"):
        P(_model(F, 3, "oblivious", n_bins=16).prepare_dataset(k.X), y)
    own = m.prepare_dataset(k.X)
    with pytest.raises(RuntimeError, match=r"tree \d+, condition \d+ .* does not compare against one of the data set's thresholds"):
        P(own, y)
    with pytest.raises(RuntimeError, match=r"tree \d+, condition"):
        m.predict_continue_prepared(own, np.zeros((65, 3), np.float32))
    # a softmax label outside the classes is found on the device, and named
    s = Case(65, 1, 3, "greedy", 1, "softmax")
    bad = s.y.copy()
    bad[7] = 3
    with pytest.raises(RuntimeError, match=r"label 3 \(row 7\)"):
        s.m.permutation_importance_prepared(s.ds, bad, objective="softmax")
    assert _file(m, tmp_path) == file0
