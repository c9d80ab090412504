"""`tree_gram_prepared` (include/gbrl_hip.h, "The Gram matrix"): the streaming MFMA kernel and the general kernel against gbrl_cpp.tree_gram_host on
the same rows, and against the NumPy float64 evaluation of tests/test_gram_host.py.  Bound, derived there: products are exact, only the additions
round, so |got - want| <= (terms + 8) * 2^-53 * sum |v_t v_u| per entry, terms = rows * D.  Models: T trees grown by step_prepared on 300 rows."""
import numpy as np
import pytest

import gbrl_amd
from test_gpu_leaves import _grow, _model
from test_gram_host import np_gram, within_bound

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp
NT, _CACHE = 300, {}
WRAP = 4 * 64 * cpp.tree_gram_geometry(1 << 30, 1)["row_blocks"] + 1   # rows that make every block's grid-stride loop wrap


def _grown(policy, D, T, F=17, depth=3):
    key = (policy, D, T, F)
    if key not in _CACHE:
        rng = np.random.default_rng(100 * T + 10 * D + (7 if policy == "greedy" else 0))
        m = _model(F, 0, D, depth, policy)
        X = rng.standard_normal((NT, F)).astype(np.float32)
        ds = m.prepare_dataset(X)
        for _ in range(T):
            m.step_prepared(ds, rng.standard_normal((NT, D)).astype(np.float32))
        assert m.get_num_trees() == T
        _CACHE[key] = (m, ds, X, m.get_ensemble_data(), rng)
    return _CACHE[key]


# (T, D, rows, start, stop, targets): T the 16-block tail, one chunk exactly, two and three chunks (off-diagonal pairs); D the K slabs; rows the tile
# edges and the wrap of the grid-stride loop; one sub-range; targets on and off
TABLE = [(1, 1, 1, 0, 0, True), (15, 3, 63, 0, 0, True), (17, 8, 64, 0, 0, False), (17, 1, 65, 0, 0, True), (65, 3, 65, 0, 0, True), (130, 1, 200, 0, 0, True),
         (130, 8, 63, 0, 0, False), (130, 3, 64, 3, 120, True), (17, 3, WRAP, 0, 0, True), (65, 1, 200, 64, 65, False)]


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("T,D,n,a,b,with_y", TABLE)
def test_both_routes_against_the_host_rule(policy, T, D, n, a, b, with_y, monkeypatch):
    m, ds, _, e, rng = _grown(policy, D, T)
    Xv = rng.standard_normal((n, 17)).astype(np.float32)
    Y = rng.standard_normal((n, D) if D > 1 else (n,)).astype(np.float32) if with_y else None
    dv = m.prepare_dataset(Xv, reference=ds)
    host = cpp.tree_gram_host(m, Xv, Y, a, b)
    _, _, cap, capm = np_gram(e, policy, Xv, Y, a, b if b else T)
    for generic, route in (("0", "stream"), ("1", "general")):
        monkeypatch.setenv("GBRL_HIP_GRAM_GENERIC", generic)
        r, again = m.tree_gram_prepared(dv, Y, a, b), m.tree_gram_prepared(dv, Y, a, b)
        assert r["route"] == route and r["rows"] == n and r["gram"].shape == host["gram"].shape and r["gram"].dtype == np.float64
        err = np.abs(r["gram"] - host["gram"])
        print(policy, T, D, n, route, "max err / bound", (err / np.maximum((n * D + 8) * 2.0 ** -53 * cap, 1e-300)).max())
        assert within_bound(r["gram"], host["gram"], cap, n * D), np.argwhere(err > (n * D + 8) * 2.0 ** -53 * cap)[:5].tolist()
        assert np.array_equal(r["gram"], r["gram"].T) and r["gram"].tobytes() == again["gram"].tobytes()
        if with_y:
            assert within_bound(r["moment"], host["moment"], capm, n * D) and r["moment"].tobytes() == again["moment"].tobytes()
        else:
            assert r["moment"] is None


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
def test_rows_with_duplicates_and_the_numpy_reference(policy):
    m, ds, X, e, rng = _grown(policy, 3, 65)
    rows = np.array([299, 5, 5, 0, 64, 63, 127, 1] * 9 + [2], np.int32)   # 73 positions: two tiles
    Y = rng.standard_normal((rows.size, 3)).astype(np.float32)
    r = m.tree_gram_prepared(ds, Y, rows=rows)
    want, wm, cap, capm = np_gram(e, policy, X[rows], Y, 0, 65)
    assert r["route"] == "stream" and r["rows"] == rows.size
    assert within_bound(r["gram"], want, cap, rows.size * 3) and within_bound(r["moment"], wm, capm, rows.size * 3)


def test_the_reweighting_loop_end_to_end():
    m, ds, X, _, rng = _grown("oblivious", 1, 15)
    Y = rng.standard_normal(NT).astype(np.float32)
    r = m.tree_gram_prepared(ds, Y)
    w = np.linalg.solve(r["gram"] + 1e-3 * np.eye(15), r["moment"]).astype(np.float32)
    m.scale_trees(w)
    after, want = m.tree_gram_prepared(ds, Y)["gram"], r["gram"] * np.outer(w, w).astype(np.float64)   # (the device mirror follows the host values)
    assert np.allclose(after, want, rtol=1e-5, atol=1e-6 * np.abs(want).max())   # one float32 rounding per scaled value


@pytest.mark.parametrize("what,msg", [("foreign", "does not compare against one of the data set's thresholds"), ("range", "invalid tree range"),
                                      ("rows", "outside"), ("targets", "targets"), ("nan", "targets hold a NaN"), ("value", "leaf value of the range is not finite"),
                                      ("categorical", "categorical columns")])
def test_refusals(what, msg):
    m, ds, X, e, rng = _grown("oblivious", 3, 17)
    bad, bad_ds, args, kw = m, ds, (), {}
    if what == "foreign":
        bad_ds = m.prepare_dataset(X * 3.0)
    elif what == "range":
        kw = dict(start_tree_idx=5, stop_tree_idx=18)
    elif what == "rows":
        kw = dict(rows=np.array([0, NT], np.int32))
    elif what == "targets":
        args = (np.zeros((NT - 1, 3), np.float32),)
    elif what == "nan":
        args = (np.full((NT, 3), np.nan, np.float32),)
    elif what == "value":
        bad, bad_ds, _, _, _ = _grown("oblivious", 3, 2)
        _CACHE.pop(("oblivious", 3, 2, 17))   # (its tree 0 is spoilt below)
        for _ in range(2):
            bad.scale_trees(np.array([3e38], np.float32))
    elif what == "categorical":
        bad = _model(3, 2, 3, 3)
        _grow(bad, rng, 2, 3, 2, 3)
    with pytest.raises(RuntimeError, match=msg):
        bad.tree_gram_prepared(bad_ds, *args, **kw)


def test_the_cap_of_2048_trees():
    """2049 stumps on 64 rows in one fit_prepared: the whole range is refused before anything is enqueued; 2048 of them are the largest grid the call
    launches (528 chunk pairs), and its first chunk pair is the 64-tree call's, byte for byte (one row block either way)."""
    rng = np.random.default_rng(2049)
    m = _model(4, 0, 1, 1)
    X = rng.standard_normal((64, 4)).astype(np.float32)
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, rng.standard_normal(64).astype(np.float32), 2049)
    assert m.get_num_trees() == 2049
    with pytest.raises(RuntimeError, match="tree_gram_prepared: 2049 trees; at most 2048 per call"):
        m.tree_gram_prepared(ds)
    with pytest.raises(RuntimeError, match="tree_gram_host: 2049 trees; at most 2048 per call"):
        cpp.tree_gram_host(m, X)
    big, small = m.tree_gram_prepared(ds, stop_tree_idx=2048), m.tree_gram_prepared(ds, stop_tree_idx=64)
    assert big["route"] == "stream" and big["gram"].shape == (2048, 2048) and np.array_equal(big["gram"], big["gram"].T)
    assert big["gram"][:64, :64].tobytes() == small["gram"].tobytes()
    last = m.tree_gram_prepared(ds, start_tree_idx=1984, stop_tree_idx=2048)["gram"]
    assert big["gram"][1984:, 1984:].tobytes() == last.tobytes()
