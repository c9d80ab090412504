"""More distinct categorical cells than Fc * n_bins candidates: the reference keeps the categories with the largest mean squared gradient
norm (split_candidate_generator.cpp:117-163).  The device computes count and float32 total of every distinct (feature, cell) pair
(cat_rank.hip); the totals must equal the reference's row-order loop BIT FOR BIT, step() and fit() must grow the reference's trees
(fixtures catrank_*.npz, made by tests/golden/make_catrank_golden.py), and the host scan of every cell (GBRL_HIP_HOST_CATEGORICAL=1) must
give the same bytes."""
import os

import numpy as np
import pytest

import cases as K
import catrank_cases as C
from helpers import GOLDEN, assert_structure_equal, assert_values_close, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


# ---- 1. the statistics -------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32 fma(a, b, c), exactly: a * b is exact in float64; s = fl64(p + c) with its exact error e (two-sum); rounding s to float32 is
    the correctly rounded result unless s sits exactly between two float32 values while e != 0 -- then the neighbour on e's side is."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    fix_up = (e > 0) & (s > r64) & (s == (r64 + up) * 0.5)
    fix_dn = (e < 0) & (s < r64) & (s == (r64 + dn) * 0.5)
    r = np.where(fix_up, up.astype(np.float32), r)
    return np.where(fix_dn, dn.astype(np.float32), r).astype(np.float32)


def _serial_stats(Xc, G):
    """{(feature, first row): (count, total)}: the loop of split_candidate_generator.cpp:119-129 on the norms of math_ops.cpp:726-749."""
    N, D = G.shape
    norm = np.zeros(N, np.float32)
    for d in range(D):
        norm = _fma32(G[:, d], G[:, d], norm)
    out = {}
    for f in range(Xc.shape[1]):
        _, first, inv, cnt = np.unique(Xc[:, f], return_index=True, return_inverse=True, return_counts=True)
        order = np.argsort(inv, kind="stable")                                  # rows of one category together, ascending
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        for u in range(len(cnt)):
            x = norm[order[start[u]:start[u] + cnt[u]]]
            out[(f, int(first[u]))] = (int(cnt[u]), np.cumsum(x, dtype=np.float32)[-1])   # a float32 cumulative sum IS the serial loop
    return out


def _tok(prefix, ids):
    return np.array([(prefix + "%06d" % i).encode() for i in ids], dtype="S128")


def _stats_inputs(name):
    rng = np.random.default_rng({"small": 1, "ragged": 2, "long": 3, "ties": 4}[name])
    if name == "small":
        N, D = 600, 2
        Xc = np.stack([_tok("a", rng.integers(0, 40, N)), _tok("b", rng.integers(0, 40, N))], axis=1)
    elif name == "ragged":
        N, D = 1531, 3
        Xc = np.stack([_tok("a", rng.integers(0, 3, N)), _tok("b", rng.integers(0, 40 * N, N)), _tok("c", rng.integers(0, 20, N))], axis=1)
    elif name == "long":                                 # one chain of ~63 000 rows (past 65 536 rows in the batch), 300 short ones
        N, D = 70001, 2
        ids = np.where(rng.random(N) < 0.9, 0, 1 + rng.integers(0, 300, N))
        Xc = _tok("a", ids).reshape(N, 1)
    else:                                                # every norm is exactly 4.0: totals are multiples of 4, powers of two among them
        N, D = 4096, 4
        Xc = np.stack([_tok("a", rng.integers(0, 30, N)), _tok("b", rng.integers(0, 30, N))], axis=1)
        G = (rng.integers(0, 2, (N, D)) * 2 - 1).astype(np.float32)
        return np.ascontiguousarray(Xc), G
    G = (rng.standard_normal((N, D)) * np.exp(rng.standard_normal((N, 1)))).astype(np.float32)
    return np.ascontiguousarray(Xc), G


@pytest.mark.parametrize("name", ["small", "ragged", "long", "ties"])
def test_device_ranking_statistics_equal_the_serial_loop_bit_for_bit(name):
    import gbrl_amd
    Xc, G = _stats_inputs(name)
    want = _serial_stats(Xc, G)
    feat, first, count, total = gbrl_amd.gbrl_cpp._cat_rank_stats(Xc, G)
    got = {(int(f), int(r)): (int(c), np.float32(t)) for f, r, c, t in zip(feat, first, count, total)}
    assert len(got) == len(feat) == len(want)
    assert set(got) == set(want)
    bad = [(k, got[k], want[k]) for k in want
           if got[k][0] != want[k][0] or np.float32(got[k][1]).view(np.uint32) != np.float32(want[k][1]).view(np.uint32)]
    assert not bad, bad[:5]
    if name == "long":
        assert max(c for c, _ in want.values()) > 60000
    if name == "ties":
        assert all(t == 4.0 * c for c, t in got.values())


# ---- 2. / 3. step() and fit() against the reference fixtures -----------------------------------------------------------------------------
def _load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = C.BY_NAME[name]
    X, Xc, G, y = C.make_inputs(case)
    assert K.inputs_digest(X, Xc, G, y) == str(g["inputs_sha256"]), "input synthesis drifted from the fixture"
    return case, g, (X, Xc, G, y)


def _setters(m, case):
    F, Fc = case["F"], case["Fc"]
    m.set_feature_weights(np.ones(F + Fc, np.float32))
    for o in K.optimizers(case):
        m.set_optimizer(**o)
    m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))


def _step_run(case, X, Xc, G):
    import gbrl_amd
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
    _setters(m, case)
    m.set_profiling(True)
    phases = []
    for _ in range(case["trees"]):
        m.step(X, Xc, G.copy())
        phases.append(dict(m.last_phase_times()))
    return m, np.asarray(m.predict(X, Xc, 0, 0)), phases


@pytest.mark.parametrize("name", [c["name"] for c in C.STEP_CASES])
def test_step_ranks_on_the_device_and_matches_the_reference(name, monkeypatch):
    case, g, (X, Xc, G, y) = _load(name)
    n_distinct = sum(len(np.unique(Xc[:, f])) for f in range(case["Fc"]))
    assert n_distinct > case["Fc"] * case["n_bins"] and (name != "catrank_ties" or n_distinct >= 40)
    monkeypatch.delenv("GBRL_HIP_HOST_CATEGORICAL", raising=False)
    m, pred, phases = _step_run(case, X, Xc, G)
    e = m.get_ensemble_data()
    assert_structure_equal(e, g)
    scale = float(np.abs(G).mean())
    assert_values_close(e, g, scale, TOL)
    assert rel_err(pred, g["pred"], scale) <= TOL
    assert all("cat_rank" in p for p in phases), phases
    monkeypatch.setenv("GBRL_HIP_HOST_CATEGORICAL", "1")
    mh, pred_h, phases_h = _step_run(case, X, Xc, G)
    eh = mh.get_ensemble_data()
    for k in K.ENSEMBLE_KEYS:
        assert np.asarray(e[k]).tobytes() == np.asarray(eh[k]).tobytes(), k
    assert pred.tobytes() == pred_h.tobytes()
    assert not any("cat_rank" in p for p in phases_h), phases_h


def test_fit_ranks_the_whole_data_set_and_matches_the_reference():
    """fit() on a data set with 60 distinct categories against 8 kept: the norms are those of the reference's full_grads (fitter.cpp:152-160).
    The second fit() asks for 6 iterations of a model that holds 4 trees: predict_cpu then returns the bias alone (predictor.cpp:130-133)."""
    import gbrl_amd
    case, g, (X, Xc, G, y) = _load("catrank_fit")
    assert sum(len(np.unique(Xc[:, f])) for f in range(case["Fc"])) == 60 > case["Fc"] * case["n_bins"]
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
    loss, pred = K.drive_fit(m, case, X, y, Xc)
    e = m.get_ensemble_data()
    assert m.get_num_trees() == int(g["n_trees"]) == case["fit_iterations"]
    assert_structure_equal(e, g)
    scale = float(np.abs(y).mean())
    assert_values_close(e, g, scale, TOL)
    assert rel_err(np.asarray(m.get_bias()), g["bias"], scale) <= TOL
    assert rel_err(pred, g["pred"], scale) <= TOL
    assert abs(loss - float(g["fit_loss"])) <= TOL * max(1.0, abs(float(g["fit_loss"])))
    loss2 = float(m.fit(X, Xc, y, case["fit2_iterations"], False, "MultiRMSE"))
    e2 = m.get_ensemble_data()
    assert m.get_num_trees() == int(g["fit2_n_trees"]) == case["fit_iterations"] + case["fit2_iterations"]
    g2 = {k: g["fit2_" + k] for k in K.ENSEMBLE_KEYS}
    assert_structure_equal(e2, g2, "second fit: ")
    assert_values_close(e2, g2, scale, TOL, "second fit: ")
    assert rel_err(np.asarray(m.predict(X, Xc, 0, 0)), g["fit2_pred"], scale) <= TOL
    assert abs(loss2 - float(g["fit2_loss"])) <= TOL * max(1.0, abs(float(g["fit2_loss"])))
