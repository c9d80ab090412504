"""SHAP interaction values on a prepared data set, on the GPU (GBRL.shap_interactions_prepared / GBRL.shap_interaction_importance_prepared;
include/gbrl_hip.h, "SHAP interaction values on a data set").  Every comparison is equality of the bytes: the matrix against
gbrl_cpp.shap_interactions_host on the observations behind the data set -- which tests/test_shap_interactions_host.py holds to the brute-force reference,
and which is held to it here too, on these thresholds -- through the streaming kernel and the one-thread-per-row kernel (GBRL_HIP_SHAPX_GENERIC=1), and
the importance against gbrl_cpp.shap_sums_host of the flattened matrix.  The models are shapx_cases' hand-written ones with their thresholds drawn from
the data set's; N = 65 rows: a block's 64 and one more, row 0 exactly on a threshold."""
import numpy as np
import pytest

import gbrl_amd
from shapx_cases import CASES, F, N, hand_model, reference, rows_on_thresholds
from test_shap_interactions_host import BOUND

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp


@pytest.fixture(scope="module")
def binned(tmp_path_factory):
    """(a data set of 512 rows whose thresholds the models use, those thresholds)"""
    m = hand_model("obl_d1_D1", tmp_path_factory.mktemp("shapx") / "b.gbrl_model")
    ds = m.prepare_dataset(np.random.default_rng(11).standard_normal((512, F)).astype(np.float32))
    return ds, np.asarray(ds.thresholds())


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a.dtype, b.dtype, a.shape, b.shape, int((a != b).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_both_calls_equal_the_host_rule_through_both_kernels(name, binned, tmp_path, monkeypatch):
    ds_ref, thresholds = binned
    m = hand_model(name, tmp_path / "m.gbrl_model", thresholds)
    X = rows_on_thresholds(m, np.random.default_rng(5).standard_normal((N, F)).astype(np.float32))
    ds = m.prepare_dataset(X, reference=ds_ref)
    host, part = cpp.shap_interactions_host(m, X), cpp.shap_interactions_host(m, X, 2)
    phi = host["values"]
    features, Phi, expected, _ = reference(m, X)
    assert host["features"].tolist() == features.tolist() and np.abs(phi - Phi).max() <= BOUND * np.abs(Phi).max() > 0
    dup = np.array([5, 64, 5, 0, 63, 64, 2], np.int32)                           # duplicates, out of order
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("GBRL_HIP_SHAPX_GENERIC", "1")
        what = name + (": general kernel" if generic else ": streaming kernel")
        got = m.shap_interactions_prepared(ds)
        _same(np.asarray(got["values"]), phi, what)
        assert (got["block_rows"] == 0) == generic, (what, got["block_rows"])
        _same(got["features"], host["features"], what)
        _same(got["expected"], host["expected"], what)
        for n in (1, 63, 64):                                                    # a block of one row, one short of the tile, the tile
            _same(np.asarray(m.shap_interactions_prepared(ds, rows=np.arange(n, dtype=np.int32))["values"]), phi[:n], what + ", %d rows" % n)
        _same(np.asarray(m.shap_interactions_prepared(ds, rows=dup)["values"]), phi[dup], what + ", rows=")
        _same(np.asarray(m.shap_interactions_prepared(ds, n_trees=2)["values"]), part["values"], what + ", n_trees=2")
        s, a = cpp.shap_sums_host(phi.reshape(N, -1))
        for chunk_rows in (None, 64):
            r = m.shap_interaction_importance_prepared(ds, chunk_rows=chunk_rows)
            _same(r["sum"].ravel(), s, what + ": sum, chunk_rows=%s" % chunk_rows)
            _same(r["sum_abs"].ravel(), a, what + ": sum_abs, chunk_rows=%s" % chunk_rows)
            assert r["n_rows"] == N and r["sum"].shape == phi.shape[1:] and r["chunk_rows"] == (chunk_rows or r["chunk_rows"]) and (r["block_rows"] == 0) == generic
        sd, ad = cpp.shap_sums_host(phi[dup].reshape(len(dup), -1))
        _same(m.shap_interaction_importance_prepared(ds, rows=dup)["sum_abs"].ravel(), ad, what + ": sum_abs, rows=")


def test_refusals(binned, tmp_path):
    ds, thresholds = binned
    m = hand_model("obl_d2_D3", tmp_path / "m.gbrl_model", thresholds)
    for call in (m.shap_interactions_prepared, m.shap_interaction_importance_prepared):
        for bad in (0, 5):
            with pytest.raises(RuntimeError, match=r"n_trees %d is outside \[1, 4\]" % bad):
                call(ds, n_trees=bad)
        with pytest.raises(RuntimeError):
            call(ds, rows=np.array([0, 512], np.int32))                          # a row outside the data set
    with pytest.raises(RuntimeError, match="chunk_rows 65 is not a positive multiple of 64"):
        m.shap_interaction_importance_prepared(ds, chunk_rows=65)
    K = len(m.shap_interactions_prepared(ds, rows=np.zeros(1, np.int32))["features"])
    with pytest.raises(RuntimeError, match="2\\^31 elements or more"):
        m.shap_interactions_prepared(ds, rows=np.zeros(2 ** 31 // (K * K * 3) + 1, np.int32))
    off = hand_model("grd_d2_D1", tmp_path / "off.gbrl_model")                    # thresholds that are none of the data set's
    with pytest.raises(RuntimeError, match="the bin codes cannot express it"):
        off.shap_interactions_prepared(ds)
