"""`predict_staged_prepared` / `staged_loss_prepared` (include/gbrl_hip.h): every ensemble prefix in one walk over a data set's bin codes.
Stage s is `predict_continue_prepared(ds, tiled bias, 0, stops[s])` byte for byte.  Every stage's loss against NumPy float64 on that yardstick's predictions,
relative tolerance 64 m D 2**-53 (a re-ordered float64 sum of m D non-negative terms, with slack for the row loss's own rounding; the device row losses are
float64 from the float32 scores, so the textbook formulas are the reference; rmse is MultiRMSE as tests/test_gpu_staged.py defines it, the difference taken
in float32), and equal to fit_prepared's valid_loss / valid_metric with np.array_equal; both kernel families return equal bytes.  Models: fit_prepared on
300 rows, depth 3, T = 3 kG + 1 trees (kG = the streaming kernel's trees per group at that D), so that stops with gaps kG - 1, kG, kG + 1 fit."""
import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu
TOL = lambda m, D: 64.0 * m * D * 2.0 ** -53
NT, _CACHE = 300, {}


def _model(F, D, policy="oblivious", opts=None):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=3, n_bins=32, split_score_func="L2", generator_type="Quantile",
                      grow_policy=policy, device="cpu", batch_size=5000)
    for o in opts or [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)]:
        m.set_optimizer(**o)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _targets(rng, X, D, obj):
    S = X[:, :1] * np.linspace(1.0, 2.0, D, dtype=np.float32) + 0.5 * rng.standard_normal((X.shape[0], D)).astype(np.float32)
    if obj == "softmax":
        return np.argmax(S, axis=1).astype(np.int32)
    T = (S > 0.2).astype(np.float32) if obj == "logistic" else S.astype(np.float32)
    return np.ascontiguousarray(T[:, 0] if D == 1 else T)


def _stages(m, ds, n, T, rows=None):
    bias = np.asarray(m.get_bias(), np.float32).reshape(-1)
    base = np.ascontiguousarray(np.tile(bias, (n, 1))) if bias.size > 1 else np.full(n, bias[0], np.float32)
    return [base.reshape(n, -1)] + [np.asarray(m.predict_continue_prepared(ds, base, 0, k, rows=rows)).reshape(n, -1) for k in range(1, T + 1)]


def _grown(policy, n, F, D, opts=None):
    key = (policy, n, F, D, repr(opts))
    if key not in _CACHE:
        rng = np.random.default_rng(4100 + 7 * n + D + (policy == "greedy"))
        kG = 8 if D <= 4 else 4 if D <= 8 else 2 if D <= 16 else 1
        X = rng.standard_normal((NT, F)).astype(np.float32)
        m = _model(F, D, policy, opts)
        ds = m.prepare_dataset(X)
        m.fit_prepared(ds, _targets(rng, X, D, "rmse"), 3 * kG + 1)
        dsv = m.prepare_dataset(rng.standard_normal((n, F)).astype(np.float32), reference=ds)
        _CACHE[key] = (m, dsv, _stages(m, dsv, n, 3 * kG + 1), 3 * kG + 1, kG)
    return _CACHE[key]


def _check_stages(env, m, ds, want, stops, n, rows=None):
    got = []
    for flag in ("0", "1"):   # the streaming kernel where it takes the shape, then the general one
        env.setenv("GBRL_HIP_STAGED_GENERIC", flag)
        got.append(np.asarray(m.predict_staged_prepared(ds, stops, rows=rows)))
    ks = range(len(want)) if stops is None else stops
    assert got[0].dtype == np.float32 and got[0].shape[:2] == (len(ks), n) and got[0].tobytes() == got[1].tobytes()
    for s, k in enumerate(ks):
        assert got[0][s].tobytes() == want[k].tobytes(), "stage %d (k = %d)" % (s, k)


# one lane; a tile edge; a second tile with a ragged tail and a second code group; a third group and the widest streaming D; the general kernel's first D
@pytest.mark.parametrize("stops", ["zero", "last", "every", "gaps"])
@pytest.mark.parametrize("n,F,D", [(1, 16, 1), (63, 16, 3), (65, 17, 8), (129, 33, 64), (70, 16, 65)])
@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_stage_bytes(policy, n, F, D, stops, monkeypatch):
    m, ds, want, T, kG = _grown(policy, n, F, D)
    _check_stages(monkeypatch, m, ds, want, {"zero": [0], "last": [T], "every": None, "gaps": [kG - 1, 2 * kG - 1, 3 * kG]}[stops], n)


@pytest.mark.parametrize("opts", [[dict(algo="SGD", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=8, stop_lr=0.01, T=50)],
                                  [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=6),
                                   dict(algo="SGD", scheduler="Const", init_lr=0.03, start_idx=6, stop_idx=8)]], ids=["linear", "two-optimizers"])
def test_stage_bytes_by_optimizer_layout(opts, monkeypatch):
    m, ds, want, T, kG = _grown("oblivious", 65, 17, 8, opts)
    _check_stages(monkeypatch, m, ds, want, None, 65)


def test_rows_with_duplicates_out_of_order(monkeypatch):
    m, ds, _, T, kG = _grown("oblivious", 129, 33, 64)
    rows = np.array([128, 5, 5, 0, 64, 63, 127, 1] * 9 + [2], np.int32)   # 73 positions: two tiles
    _check_stages(monkeypatch, m, ds, _stages(m, ds, rows.size, T, rows=rows), [0, 1, T - 1, T], rows.size, rows=rows)


# ---- the losses: one fit_prepared per case with the evaluated set watched as valid=; its curve is the contract, NumPy the reference
# D = 3: every objective; 8, 64: the streaming kernel's 16-byte target loads, its widest register forms; 65: the general kernel alone, logistic / quantile from the stored row
NV, F3, D3, T3 = 129, 17, 3, 17
ALPHA = lambda D: np.linspace(0.1, 0.9, D, dtype=np.float32)
LOSS_CASES = [(o, w, None, D3) for o in ("rmse", "logistic", "softmax") for w in (False, True)] + [
    ("quantile", False, None, D3), ("logistic", False, "error", D3), ("softmax", False, "error", D3), ("logistic", True, None, 8), ("rmse", False, None, 64),
    ("quantile", False, None, 64), ("logistic", False, "error", 64), ("logistic", False, None, 65), ("quantile", False, None, 65), ("softmax", False, "error", 65)]


def _fitted(obj, weighted, metric, D=D3):
    key = ("fit", obj, weighted, metric, D)
    if key not in _CACHE:
        rng = np.random.default_rng(4200 + len(_CACHE))
        X, Xv = rng.standard_normal((NT, F3)).astype(np.float32), rng.standard_normal((NV, F3)).astype(np.float32)
        Y, Yv = _targets(rng, X, D, obj), _targets(rng, Xv, D, obj)
        wv = (0.25 + rng.random(NV)).astype(np.float32) if weighted else None
        m = _model(F3, D)
        ds = m.prepare_dataset(X); dsv = m.prepare_dataset(Xv, reference=ds)
        kw = dict(objective=obj, alpha=ALPHA(D) if obj == "quantile" else None)
        r = m.fit_prepared(ds, Y, T3, valid=dsv, valid_targets=Yv, valid_weights=wv, eval_metric=metric, **kw)
        _CACHE[key] = (m, dsv, Yv, wv, kw, r)
    return _CACHE[key]


def _numpy_loss(obj, P, Y, w):
    P64 = P.astype(np.float64)
    if obj == "rmse":
        L = ((P - Y).astype(np.float32).astype(np.float64) ** 2).sum(1)
    elif obj == "logistic":
        L = (np.logaddexp(0.0, P64) - Y.astype(np.float64) * P64).sum(1)                     # log1p(exp(p)) - y p
    elif obj == "softmax":
        mx = P64.max(1)
        L = mx + np.log(np.exp(P64 - mx[:, None]).sum(1)) - P64[np.arange(P.shape[0]), Y]   # log-sum-exp - p[label]
    else:
        u = Y.astype(np.float64) - P64
        L = np.where(u >= 0, ALPHA(P.shape[1]).astype(np.float64) * u, (ALPHA(P.shape[1]).astype(np.float64) - 1.0) * u).sum(1)   # pinball
    total, rows = (L.sum(), float(P.shape[0])) if w is None else ((w.astype(np.float64) * L).sum(), w.astype(np.float64).sum())
    return np.sqrt(0.5 * total / rows) if obj == "rmse" else total / rows


@pytest.mark.parametrize("obj,weighted,metric,D", LOSS_CASES)
def test_loss_contract_reference_and_both_kernels(obj, weighted, metric, D, monkeypatch):
    m, dsv, Yv, wv, kw, r = _fitted(obj, weighted, metric, D)
    got = []
    for flag in ("0", "1", "0"):
        monkeypatch.setenv("GBRL_HIP_STAGED_GENERIC", flag)
        got.append(m.staged_loss_prepared(dsv, Yv, None, weights=wv, eval_metric=metric, **kw))
    c = got[0]
    assert sorted(c) == sorted(["loss", "stops"] + (["metric", "counts"] if metric else [])) and c["loss"].dtype == np.float64 and np.array_equal(c["stops"], np.arange(T3 + 1))
    for other in got[1:]:   # the general kernel, and a second identical call
        assert all(c[k].tobytes() == other[k].tobytes() for k in c)
    assert np.array_equal(c["loss"], r["valid_loss"]), (c["loss"], r["valid_loss"])
    if metric:
        assert np.array_equal(c["metric"], r["valid_metric"])
        assert c["counts"].dtype == np.int64 and c["counts"].shape == ((T3 + 1,) if obj == "softmax" else (T3 + 1, D))
        cells = NV * (1 if obj == "softmax" else D)
        assert np.array_equal(c["counts"].reshape(T3 + 1, -1).sum(1) / cells, c["metric"])
    for k, P in enumerate(_stages(m, dsv, NV, T3)):
        ref = _numpy_loss(obj, P, Yv.reshape(NV, -1) if obj != "softmax" else Yv, wv)
        assert abs(c["loss"][k] - ref) <= TOL(NV, D) * abs(ref), (k, c["loss"][k], ref)


W1 = np.ones(NV, np.float32)
REFUSALS = [
    ("loss", dict(stops=[0, 0]), "strictly ascending"), ("loss", dict(stops=[T3 + 1]), "out of bounds"), ("loss", dict(stops=[]), "stops is empty"),
    ("predict", dict(stops=[3, 1]), "strictly ascending"), ("predict", dict(stops=[-1]), "out of bounds"),
    ("loss", dict(targets=None), "without targets"), ("loss", dict(targets=np.zeros((NV, 2), np.float32)), "Expected targets of shape"),
    ("loss", dict(alpha=0.5), "alpha is the level table of the quantile objective"), ("loss", dict(objective="quantile"), "needs alpha"),
    ("loss", dict(objective="quantile", alpha=0.5, weights=W1), "row weights with the quantile objective"), ("loss", dict(weights=-W1), "is not a finite number in"),
    ("loss", dict(weights=0 * W1), "sum to 0"), ("loss", dict(weights=W1[:-1]), "Expected weights"), ("loss", dict(eval_metric="error"), "rmse objective has no metric"), ("loss", dict(objective="quantile", alpha=0.5, eval_metric="error"), "has no metric"),
    ("loss", dict(objective="logistic", eval_metric="error", weights=W1), "weights with eval_metric"), ("loss", dict(objective="logistic", eval_metric="auc"), "auc"),
    ("loss", dict(objective="pairwise", targets=np.zeros(NV, np.int32)), "ranking objectives"), ("loss", dict(objective="softmax", targets=np.full(NV, D3, np.int32)), "is outside"),
    ("predict", dict(rows=40000000, stops=None), "2\\^31"), ("predict", dict(rows=np.array([NV], np.int32)), "outside"),
    ("loss", dict(ds="foreign"), "does not compare against one of the data set's thresholds"), ("predict", dict(ds="foreign"), "tree 0"), ("loss", dict(model="empty", stops=None), "the model has no trees"), ("predict", dict(model="wide", stops=[0]), "output_dim > 128"),
]


@pytest.mark.parametrize("form,kw,msg", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_leave_the_model_alone(form, kw, msg, tmp_path):
    m, dsv, Yv, _, _, _ = _fitted("rmse", False, None)
    kw = dict(kw)
    which, data = kw.pop("model", None), kw.pop("ds", None)
    if which:   # a model without trees; a model of 129 outputs: each with a data set of its own
        m = _model(F3, D3 if which == "empty" else 129)
        dsv = m.prepare_dataset(np.random.default_rng(1).standard_normal((NV, F3)).astype(np.float32))
    if data:    # thresholds the model's trees were not grown on
        dsv = m.prepare_dataset(np.random.default_rng(2).standard_normal((NV, F3)).astype(np.float32) * 3.0)
    _file = lambda path: (m.save(str(path)), path.read_bytes())
    before = _file(tmp_path / "before")
    kw.setdefault("stops", [0, 1])
    if isinstance(kw.get("rows"), int):   # that many positions of row 0, built here and not at import
        kw["rows"] = np.zeros(kw["rows"], np.int32)
    with pytest.raises(RuntimeError, match=msg):
        if form == "predict":
            m.predict_staged_prepared(dsv, **kw)
        else:
            m.staged_loss_prepared(dsv, kw.pop("targets", Yv), **kw)
    assert _file(tmp_path / "after") == before and before[0] == 0
