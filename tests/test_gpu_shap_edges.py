"""k_shap (csrc/shap.hip) at every launch geometry it has, against the host evaluation (csrc/explain.cpp) byte for byte.

The kernel runs one thread per (sample, output) and sizes its block by the model's (max_depth, output_dim): 256 / 128 / 64 threads, threads /
output_dim samples per block, dead lanes when output_dim does not divide the block, the host evaluation when nothing fits (the table and its
derivation: tests/golden/shap_edge_cases.py; the models are the reference-grown fixtures made from it).  Every device call here runs under
GBRL_HIP_SHAP_DEVICE_ONLY=1, which raises where the engine would otherwise hand the call to the host silently -- so a comparison that passes
compared k_shap with the host evaluation and not the host with itself.  The other side of every comparison is the same call under
GBRL_HIP_SHAP_HOST=1; the assertion is equality of the bytes (the host values are finite on all these rows: tests/test_shap_edges_host.py)."""
import numpy as np
import pytest

import shap_edge_cases as S
import shap_edges as E
from test_explain import SHAP_TOL

pytestmark = pytest.mark.gpu


def _device(monkeypatch):
    monkeypatch.delenv("GBRL_HIP_SHAP_HOST", raising=False)
    monkeypatch.setenv("GBRL_HIP_SHAP_DEVICE_ONLY", "1")


def _host(monkeypatch):
    monkeypatch.delenv("GBRL_HIP_SHAP_DEVICE_ONLY", raising=False)
    monkeypatch.setenv("GBRL_HIP_SHAP_HOST", "1")


def _unhooked(monkeypatch):
    for h in E.HOOKS:
        monkeypatch.delenv(h, raising=False)


def _same_bytes(dev, host, what):
    assert len(dev) == len(host)
    for k, (a, b) in enumerate(zip(dev, host)):
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (what, k)
        assert np.isfinite(b).all(), (what, k)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError("%s, call %d: %d of %d values differ, first at [row, feature, output] %s: device %r host %r" % (
                what, k, len(bad), a.size, bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def test_launch_plan_and_the_three_decline_boundaries(tmp_path, monkeypatch):
    """The exported plan is the derived table; a shape the kernel declines raises under the _ONLY hook and gets the host's bytes without it
    -- max_depth 16 | 17, output_dim 256 | 257 at 256 threads, 128 | 129 at 128 threads, 64 | 65 at 64 threads."""
    for c in S.CASES:
        assert E.plan(c["depth"], c["D"]) == S.PLAN[c["name"]], c["name"]
    for name in S.HOST_CASES:
        case, g, X, Xc, G, poly = E.fixture(name)
        m = E.load_model(name, tmp_path)
        xs, xcs = E.cycled(X, case["shap_rows"]), E.cycled(Xc, case["shap_rows"])
        _device(monkeypatch)
        with pytest.raises(RuntimeError, match="no launch plan for max_depth %d, output_dim %d" % (case["depth"], case["D"])):
            m.ensemble_shap(xs, xcs, *poly)
        with pytest.raises(RuntimeError, match="no launch plan"):
            m.tree_shap(0, xs, xcs, *poly)
        _unhooked(monkeypatch)
        plain = E.shap_calls(m, xs, xcs, poly)
        _host(monkeypatch)
        _same_bytes(plain, E.shap_calls(m, xs, xcs, poly), name)
        for a, w in zip(plain, E.reference_values(g)):
            assert np.abs(a.astype(np.float64) - w).max() <= SHAP_TOL * np.abs(w).max(), name


@pytest.mark.parametrize("name", S.DEVICE_CASES)
def test_every_block_geometry_equals_the_host_evaluation(name, tmp_path, monkeypatch):
    """Row counts around the samples-per-block of the case's plan -- one row, a block short of one sample, exactly full, one sample into the
    second block, one into the third -- and a few hundred rows (several blocks, the last one ragged, dead lanes in each when output_dim does
    not divide the block): ensemble_shap and tree_shap of the first, middle and last tree.  At the fixture's row count the device values are
    also held to the reference's."""
    case, g, X, Xc, G, poly = E.fixture(name)
    nt, per = E.plan(case["depth"], case["D"])
    assert (nt, per) == S.PLAN[name] and per >= 1
    m = E.load_model(name, tmp_path)
    counts = sorted({1, per - 1, per, per + 1, 2 * per + 1, E.MANY_ROWS, case["shap_rows"]} - {0})
    assert -(-E.MANY_ROWS // per) >= 3
    for n in counts:
        xs, xcs = E.cycled(X, n), E.cycled(Xc, n)
        _device(monkeypatch)
        dev = E.shap_calls(m, xs, xcs, poly)
        _host(monkeypatch)
        _same_bytes(dev, E.shap_calls(m, xs, xcs, poly), "%s, %d rows (%d threads, %d samples per block)" % (name, n, nt, per))
        if n == case["shap_rows"]:
            for a, w in zip(dev, E.reference_values(g)):
                err = np.abs(a.astype(np.float64) - w).max() / max(float(np.abs(w).max()), 1e-30)      # (a depth-0 tree's values are zeros)
                print("%s vs the reference: %.3g of the array's scale" % (name, err))
                assert err <= SHAP_TOL, name


@pytest.mark.parametrize("name", S.DEVICE_CASES)
def test_edge_values_in_split_features_equal_the_host_evaluation(name, tmp_path, monkeypatch):
    """Cells exactly on a used threshold and one float32 ulp to either side; NaN, +-inf, +-0.0 and a subnormal in every split feature; for
    categorical columns the trained cells, a never-seen cell, the empty string, a 127-byte cell and a trained cell as the prefix of a longer
    one (a dictionary id 0 must match no condition).  Device == host bytes, and ON a threshold == one ulp BELOW it."""
    case, g, X, Xc, G, poly = E.fixture(name)
    m = E.load_model(name, tmp_path)
    xs, xcs, triples = E.edge_rows(m, X, Xc)
    _device(monkeypatch)
    dev = E.shap_calls(m, xs, xcs, poly)
    _host(monkeypatch)
    _same_bytes(dev, E.shap_calls(m, xs, xcs, poly), name + ", edge rows")
    for a in dev:
        for below, on, above in triples:
            assert a[on].tobytes() == a[below].tobytes(), (name, on)


@pytest.mark.parametrize("name", ["t256_d4_D7_grd_cat", "t128_d8_D3_obl_deep"])
def test_cached_program_follows_the_model(name, tmp_path, monkeypatch):
    """The whole-ensemble program stays on the device until the model changes, and a tree_shap call overwrites it: a fixture model that keeps
    training on the GPU is explained in an order that meets every reuse -- after each call the device has the host's bytes."""
    case, g, X, Xc, G, poly = E.fixture(name)
    m = E.load_model(name, tmp_path)
    m.to_device("cpu")
    T = m.get_num_trees()
    xs, xcs = E.cycled(X, 50), E.cycled(Xc, 50)

    def both(call, what):
        _device(monkeypatch)
        dev = call()
        _host(monkeypatch)
        host = call()
        _same_bytes([dev], [host], "%s: %s" % (name, what))
        _unhooked(monkeypatch)
        return dev

    first = both(lambda: m.ensemble_shap(xs, xcs, *poly), "1 ensemble")
    both(lambda: m.tree_shap(0, xs, xcs, *poly), "2 tree 0 (overwrites the program)")
    again = both(lambda: m.ensemble_shap(xs, xcs, *poly), "3 ensemble (rebuilt)")
    assert again.tobytes() == first.tobytes()
    m.step(None if X is None else X.copy(), None if Xc is None else Xc.copy(), G.copy())
    assert m.get_num_trees() == T + 1
    grown = both(lambda: m.ensemble_shap(xs, xcs, *poly), "5 ensemble after a step")
    last = both(lambda: m.tree_shap(T, xs, xcs, *poly), "6 the new tree")
    assert np.abs(last).max() > 0                                   # the new tree splits ...
    assert grown.tobytes() != first.tobytes()                       # ... and the cached program of step 3 was not reused for it
    n2 = 2 * E.plan(case["depth"], case["D"])[1] + 3
    both(lambda: m.ensemble_shap(E.cycled(X, n2), E.cycled(Xc, n2), *poly), "7 ensemble, another row count (program reused)")
