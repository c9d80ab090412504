"""The TreeSHAP launch-geometry fixtures (tests/golden/shap_edge_cases.py: models whose max_depth and output_dim select every block size of
the device kernel, grown and explained by the REFERENCE's CPU build) through the HOST evaluation (csrc/explain.cpp), which is what serves a
machine without a GPU and what tests/test_gpu_shap_edges.py compares k_shap with, byte for byte.

Bars: every value finite; within SHAP_TOL (tests/test_explain.py: 1e-5) of the reference's array, relative to its largest magnitude.  The
fixtures also have to BE what the case table says -- a chain of tied nodes, a depth-0 tree between full ones, trees of depth 8 -- and the
exported launch plan has to be the table derived in shap_edge_cases.py."""
import numpy as np
import pytest

import gbrl_amd
import shap_edge_cases as S
import shap_edges as E
from test_explain import SHAP_TOL


@pytest.fixture(autouse=True)
def _host_evaluation(monkeypatch):
    """These checks are about explain.cpp wherever they run: on a machine with a GPU the device would take the call otherwise."""
    for h in E.HOOKS:
        monkeypatch.delenv(h, raising=False)
    monkeypatch.setenv("GBRL_HIP_SHAP_HOST", "1")


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.isfinite(got).all(), what + ": not finite"
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) / scale
    print("%s: %.3g of the array's scale" % (what, err))
    assert err <= SHAP_TOL, f"{what}: {err:.3g} of the array's scale"


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_host_shap_of_every_geometry_case_matches_the_reference(name, tmp_path):
    case, g, X, Xc, G, poly = E.fixture(name)
    m = E.load_model(name, tmp_path)
    md = m.get_metadata()
    assert (md["max_depth"], md["output_dim"], m.get_num_trees()) == (case["depth"], case["D"], case["trees"])
    n = case["shap_rows"]
    got = E.shap_calls(m, E.cycled(X, n), E.cycled(Xc, n), poly)
    want = E.reference_values(g)
    assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 0
    for a, w, what in zip(got, want, ["ensemble"] + ["tree %d" % t for t in E.tree_picks(case["trees"])]):
        _close(a, w, name + " " + what)


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_host_shap_stays_finite_on_edge_value_rows(name, tmp_path):
    """The rows tests/test_gpu_shap_edges.py compares byte for byte: the host evaluation must be finite on them (so that byte equality
    needs no NaN exemption), and a cell ON a threshold walks like the cell one ulp below it (`x > t` is false for both)."""
    case, g, X, Xc, G, poly = E.fixture(name)
    m = E.load_model(name, tmp_path)
    xs, xcs, triples = E.edge_rows(m, X, Xc)
    assert (len(triples) > 0) == (case["F"] > 0)
    out = E.shap_calls(m, xs, xcs, poly)
    differs = 0
    for a in out:
        assert np.isfinite(a).all()
        for below, on, above in triples:
            assert a[on].tobytes() == a[below].tobytes()
            differs += a[above].tobytes() != a[on].tobytes()
    assert differs > 0 or not triples       # one ulp ABOVE a threshold is the other side of it


def test_the_launch_plan_is_the_derived_table():
    for c in S.CASES:
        assert E.plan(c["depth"], c["D"]) == S.PLAN[c["name"]], c["name"]
    shapes = {(c["depth"], c["D"]) for c in S.CASES}
    wanted = {(7, 3), (7, 5), (4, 7), (4, 128), (4, 129), (4, 200), (4, 256), (4, 257), (8, 3), (11, 5), (8, 64), (8, 65), (8, 128), (8, 129),
              (12, 3), (16, 5), (12, 64), (12, 65), (16, 2), (17, 2)}
    assert shapes == wanted
    assert sorted(S.HOST_CASES) == ["host_d12_D65_grd", "host_d17_D2_obl", "host_d4_D257_obl", "host_d8_D129_grd"]


def _paths(e, policy):
    """per tree: [(depth, [feature per level])] of every leaf"""
    ti, depths, fi = np.asarray(e["tree_indices"]), np.asarray(e["depths"]), np.asarray(e["feature_indices"])
    n_leaves = np.asarray(e["values"]).shape[0]
    out = []
    for t in range(len(ti)):
        first, end = int(ti[t]), (int(ti[t + 1]) if t + 1 < len(ti) else n_leaves)
        rows = [t] * (end - first) if policy == "oblivious" else range(first, end)
        out.append([(int(depths[r]), [int(f) for f in fi[r, :int(depths[r])]]) for r in rows])
    return out


def test_the_fixtures_hold_the_structures_the_case_table_names(tmp_path):
    def paths(name):
        return _paths(E.load_model(name, tmp_path).get_ensemble_data(), S.BY_NAME[name]["policy"])

    # a greedy path of depth >= 5 on which one feature occurs three times: nodes tied to tied parents
    tied = [p for tree in paths("t256_d7_D3_grd_tied") for p in tree]
    assert any(d >= 5 and max(f.count(v) for v in set(f)) >= 3 for d, f in tied)
    # oblivious trees that repeat a feature
    assert all(len(set(f)) < d for tree in paths("t256_d7_D5_obl_repeat") for d, f in tree)
    # trees that really reach depth 8 under the 128-thread plan
    assert all(d == 8 for tree in paths("t128_d8_D3_obl_deep") for d, f in tree)
    # a depth-0 tree (one leaf, no condition) between two full trees
    stump = paths("t64_d12_D3_grd_stump")
    assert [len(t) for t in stump][1] == 1 and stump[1][0][0] == 0 and len(stump[0]) > 1 and len(stump[2]) > 1
    # categorical conditions in use, and a model with nothing else
    for name in ("t256_d4_D7_grd_cat", "t256_d4_D200_obl_cat", "t128_d11_D5_grd_catonly"):
        numeric, categorical = E.used_conditions(E.load_model(name, tmp_path))
        assert categorical and (bool(numeric) == (S.BY_NAME[name]["F"] > 0)), name
    # everywhere else the setting is far above what the trees reach: the kernel's loops over max_depth columns run on unused levels
    assert sum(1 for c in S.CASES if c["depth"] >= 8 and max(d for tree in paths(c["name"]) for d, f in tree) <= 4) >= 8
    assert {c["policy"] for c in S.CASES if S.PLAN[c["name"]][0]} == {"greedy", "oblivious"}


@pytest.mark.parametrize("name", S.HOST_CASES)
def test_device_only_hook_raises_for_a_shape_without_a_plan(name, tmp_path, monkeypatch):
    """GBRL_HIP_SHAP_DEVICE_ONLY=1: no silent host evaluation.  The plan is decided before any device is touched, so this needs no GPU."""
    case, g, X, Xc, G, poly = E.fixture(name)
    m = E.load_model(name, tmp_path)
    xs, xcs = E.cycled(X, 3), E.cycled(Xc, 3)
    monkeypatch.delenv("GBRL_HIP_SHAP_HOST")
    monkeypatch.setenv("GBRL_HIP_SHAP_DEVICE_ONLY", "1")
    msg = "no launch plan for max_depth %d, output_dim %d" % (case["depth"], case["D"])
    with pytest.raises(RuntimeError, match=msg):
        m.ensemble_shap(xs, xcs, *poly)
    with pytest.raises(RuntimeError, match=msg):
        m.tree_shap(0, xs, xcs, *poly)
    monkeypatch.setenv("GBRL_HIP_SHAP_HOST", "1")          # the host asked for by name is not a decline
    assert np.isfinite(m.ensemble_shap(xs, xcs, *poly)).all()


def test_device_only_hook_raises_without_a_device(tmp_path, monkeypatch):
    name = "t128_d8_D3_obl_deep"
    case, g, X, Xc, G, poly = E.fixture(name)
    m = E.load_model(name, tmp_path)
    xs = E.cycled(X, 3)
    host = m.ensemble_shap(xs, None, *poly)
    monkeypatch.delenv("GBRL_HIP_SHAP_HOST")
    monkeypatch.setenv("GBRL_HIP_SHAP_DEVICE_ONLY", "1")
    if gbrl_amd.cuda_available():
        assert m.ensemble_shap(xs, None, *poly).tobytes() == host.tobytes()
    else:
        with pytest.raises(RuntimeError, match="GBRL_HIP_SHAP_DEVICE_ONLY=1: no device"):
            m.ensemble_shap(xs, None, *poly)
        monkeypatch.delenv("GBRL_HIP_SHAP_DEVICE_ONLY")    # unset: a machine without a GPU is served by the host, as before
        assert m.ensemble_shap(xs, None, *poly).tobytes() == host.tobytes()
