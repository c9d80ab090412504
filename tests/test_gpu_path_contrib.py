"""Path attribution on a prepared data set, on the GPU (GBRL.path_contrib_prepared / GBRL.path_importance_prepared; include/gbrl_hip.h, "Path attribution
on a data set").  Every comparison is equality of the bytes: the matrix against gbrl_cpp.path_contrib_host on the observations behind the data set, the
importance against gbrl_cpp.shap_sums_host of that matrix, the streaming kernel against the one-thread-per-row kernel (GBRL_HIP_PATH_GENERIC=1); the one
tolerance, additivity against predict, is derived where it is used.  n = 130 rows (two full tiles and a tile of 2), F = 20 (two 16-column groups); models
by fit_prepared on 512 training rows with n_bins = 32, the explained rows bound with reference= (tests/test_gpu_shap_prepared.py's recipe)."""
import numpy as np
import pytest

import gbrl_amd
from test_path_host import EPS, path_reference

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp
N_TRAIN, N, F = 512, 130, 20
LINEAR = [dict(algo="SGD", scheduler="Linear", init_lr=0.1, stop_lr=0.01, T=50, start_idx=0, stop_idx=3)]
TWO = [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=1), dict(algo="SGD", scheduler="Const", init_lr=0.3, start_idx=1, stop_idx=3)]

# id: D, policy, trees, depth, optimizers (None: one Const optimizer over every output)
CASES = {
    "obl_d1_stump": (1, "oblivious", 1, 1, None),
    "obl_d3": (3, "oblivious", 12, 6, None),
    "obl_d8": (8, "oblivious", 12, 6, None),
    "grd_d3": (3, "greedy", 12, 6, None),
    "obl_d64_two_passes": (64, "oblivious", 12, 6, None),
    "grd_d64_two_passes": (64, "greedy", 12, 6, None),
    "obl_d96_general": (96, "oblivious", 12, 6, None),
    "obl_linear": (3, "oblivious", 12, 6, LINEAR),
    "grd_two_optimizers": (3, "greedy", 12, 6, TWO),
}


class Case:
    def __init__(self, D, policy, T, depth, opts):
        rng = np.random.default_rng(100 * D + T + depth)
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=32, split_score_func="L2" if policy == "oblivious" else "Cosine",
                          generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=N_TRAIN)
        for o in opts or [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)]:
            m.set_optimizer(**o)
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        W = np.where(np.arange(F)[:, None] % 2 == 0, 1.5, 0.2) * rng.choice([-1.0, 1.0], size=(F, D))     # every even column matters: both groups of 16 are tested
        Xt = rng.standard_normal((N_TRAIN, F)).astype(np.float32)
        Y = (Xt @ W + 0.2 * rng.standard_normal((N_TRAIN, D))).astype(np.float32)
        ds_train = m.prepare_dataset(Xt)
        m.fit_prepared(ds_train, np.ascontiguousarray(Y[:, 0]) if D == 1 else Y, T)
        assert m.get_num_trees() == T
        self.m, self.D, self.T = m, D, T
        self.X = rng.standard_normal((N, F)).astype(np.float32)
        self.ds = m.prepare_dataset(self.X, reference=ds_train)
        self.phi = cpp.path_contrib_host(m, self.X)          # computed once, shared, never written
        self.phi.setflags(write=False)
        e = m.get_ensemble_data()
        depths, fidx = np.asarray(e["depths"]), np.asarray(e["feature_indices"])
        self.leaf_depths = depths
        self.used = sorted(set(int(f) for f in fidx[np.arange(fidx.shape[1])[None, :] < depths[:, None]]))


@pytest.fixture(scope="module")
def case():
    made = {}
    return lambda name: made.setdefault(name, Case(*CASES[name]))


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a.dtype, b.dtype, a.shape, b.shape, int((a != b).sum()))


def _importance_equals(r, phi, expected, what):
    s, a = cpp.shap_sums_host(np.ascontiguousarray(phi))
    _same(r["sum"], s, what + ": sum")
    _same(r["sum_abs"], a, what + ": sum_abs")
    _same(r["expected"], expected, what + ": expected")


@pytest.mark.parametrize("name", list(CASES))
def test_both_calls_equal_the_host_rule_through_both_kernels(name, case, tmp_path, monkeypatch):
    k = case(name)
    m, ds, phi, plan = k.m, k.ds, k.phi, cpp.path_geometry(len(k.used), F, k.D)
    if k.T > 1:
        assert min(k.used) < 16 <= max(k.used)                              # conditions on both sides of the 16-column boundary
    if "two_passes" in name:
        assert len(k.used) >= 9 and plan["passes"] > 1, (k.used, plan)
    if name == "grd_d3":
        assert len(set(k.leaf_depths.tolist())) > 1                         # leaves at different depths
    path = tmp_path / "m.gbrl_model"
    assert m.save(str(path)) == 0
    file0, codes0 = path.read_bytes(), np.asarray(ds.codes()).copy()
    assert np.abs(phi).max() > 0 and not phi[:, [f for f in range(F) if f not in k.used]].view(np.uint32).any()
    expected = cpp.path_expected_host(m)
    _same(np.asarray(m.path_contrib_prepared(ds)), phi, "matrix")
    r = m.path_importance_prepared(ds)
    assert r["passes"] == (plan["passes"] if k.D <= 64 else 0) and r["n_rows"] == N
    _importance_equals(r, phi, expected, "importance")
    monkeypatch.setenv("GBRL_HIP_PATH_GENERIC", "1")
    _same(np.asarray(m.path_contrib_prepared(ds)), phi, "matrix, general kernel")
    g = m.path_importance_prepared(ds)
    assert g["passes"] == 0 and not _importance_equals(g, phi, expected, "importance, general kernel")
    monkeypatch.delenv("GBRL_HIP_PATH_GENERIC")
    rows = np.array([5, 129, 5, 0, 64, 63, 129, 2], np.int32)                # duplicates, out of order
    _same(np.asarray(m.path_contrib_prepared(ds, rows=rows)), phi[rows], "rows=")
    _importance_equals(m.path_importance_prepared(ds, rows=rows), phi[rows], expected, "importance, rows=")
    _importance_equals(m.path_importance_prepared(ds, rows=np.arange(N, dtype=np.int32)), phi, expected, "importance, rows=arange(n)")
    if k.T > 1:
        part = cpp.path_contrib_host(m, k.X, 5)
        _same(np.asarray(m.path_contrib_prepared(ds, n_trees=5)), part, "n_trees=5")
        _importance_equals(m.path_importance_prepared(ds, n_trees=5), part, cpp.path_expected_host(m, 5), "importance, n_trees=5")
    assert m.save(str(path)) == 0 and path.read_bytes() == file0 and np.asarray(ds.codes()).tobytes() == codes0.tobytes()


@pytest.mark.parametrize("name", ["obl_d3", "grd_two_optimizers", "obl_linear"])
def test_contributions_and_expected_value_add_up_to_predict(name, case):
    """the bound: the contributions' own (c * 2^-23 * S + 2^-23 * |phi|, summed over the features) and predict's chain of T fused multiply-adds, each
    within 2^-24 of a partial sum of at most A = max |bias| + T * max lr * max |value|"""
    k = case(name)
    phi64, S, c, _, _ = path_reference(k.m, k.X)
    e = k.m.get_ensemble_data()
    A = np.abs(np.asarray(e["bias"])).max() + k.T * 0.3 * np.abs(np.asarray(e["values"])).max()
    bound = (c * EPS * S + EPS * np.abs(phi64)).sum(1) + (k.T + 1) * EPS * A
    pred = np.asarray(k.m.predict(k.X, None), np.float64).reshape(N, k.D)
    err = np.abs(k.phi.astype(np.float64).sum(1) + cpp.path_expected_host(k.m) - pred)
    print("%s: max additivity error %.3g, bound there %.3g" % (name, err.max(), bound.flat[err.argmax()]))
    assert (err <= bound).all()
