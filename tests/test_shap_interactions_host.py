"""SHAP interaction values without a device: gbrl_cpp.shap_interactions_host (gbrl_amd/csrc/shapx_core.h has the rule) against the brute-force float64
reference of tests/shapx_cases.py on hand-written models, the identities against the reference's own quantities, the plan and the refusals.  The calls
on a data set run in tests/test_gpu_shap_interactions.py.

Tolerance.  The host rule differs from the reference by the float32 rounding of the stored value and by float64 reassociation; it cannot be derived, so
it was measured: the largest |host - reference| / max |reference| over the cases below is MEASURED = 5.14e-8 (grd_repeat; just under 2^-24, the store
rounding of an element near the array's scale; the float64 part is of the order 1e-16).  The bound is BOUND = 2^-23 = 1.19e-7, 2.3 times that, relative
to each case's max |Phi|."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd
from shapx_cases import CASES, F, N, hand_model, reference, rows_on_thresholds

cpp = gbrl_amd.gbrl_cpp
MEASURED, BOUND = 5.14e-8, 2.0 ** -23


@pytest.mark.parametrize("name", list(CASES))
def test_host_rule_against_the_subset_enumeration(name, tmp_path):
    m = hand_model(name, tmp_path / "m.gbrl_model")
    X = rows_on_thresholds(m, np.random.default_rng(3).standard_normal((N, F)).astype(np.float32))
    for n_trees in (None, 2):                                                  # the ensemble, and a prefix below the tree count
        got = cpp.shap_interactions_host(m, X, n_trees)
        features, Phi, expected, reached = reference(m, X, n_trees)
        v = got["values"]
        assert v.dtype == np.float32 and v.shape == Phi.shape and got["expected"].dtype == np.float64 and got["features"].dtype == np.int32
        assert got["features"].tolist() == features.tolist() and (len(features) == 1) == name.endswith("k1")
        scale = np.abs(Phi).max()
        err = np.abs(v.astype(np.float64) - Phi).max() / scale
        print("%s n_trees=%s: max error / scale %.3g (bound %.3g), scale %.3g" % (name, n_trees, err, BOUND, scale))
        assert scale > 0 and err <= BOUND
        assert np.abs(got["expected"] - expected).max() <= 1e-13 * (1 + np.abs(expected).max())
        assert v.transpose(0, 2, 1, 3).tobytes() == v.tobytes()                # Phi[i, j] == Phi[j, i] bitwise
        K = len(features)                                                      # additivity against the reference's reached leaves: K * K stored roundings
        assert np.abs(v.astype(np.float64).sum((1, 2)) + expected - reached).max() <= K * K * BOUND * scale + 1e-13


def test_the_plan_declines_what_does_not_fit():
    assert cpp.shap_interactions_geometry(6, 6, 6, 16, 3)["block_rows"] == 64
    big = cpp.shap_interactions_geometry(90, 6, 6, 128, 1)
    assert 1 <= big["block_rows"] < 64 and big["lds_bytes"] <= 156 * 1024
    for declined in ((200, 6, 6, 128, 1), (6, 6, 9, 16, 1), (6, 6, 6, 16, 1, 0)):       # K too large for the LDS; a path beyond the table; no table
        assert cpp.shap_interactions_geometry(*declined)["block_rows"] == 0


def test_refusals(tmp_path):
    m = hand_model("obl_d2_D1", tmp_path / "m.gbrl_model")
    for bad in (0, 5, -2):
        with pytest.raises(RuntimeError, match=r"n_trees %d is outside \[1, 4\]" % bad):
            cpp.shap_interactions_host(m, np.zeros((4, F), np.float32), bad)
    with pytest.raises(RuntimeError, match="X must be float32"):
        cpp.shap_interactions_host(m, np.zeros((4, F + 1), np.float32))
    empty = gbrl_amd.GBRL(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    empty.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2)
    with pytest.raises(RuntimeError, match="the model has no trees"):
        cpp.shap_interactions_host(empty, np.zeros((4, 4), np.float32))
    g = np.load(__file__.replace("test_shap_interactions_host.py", "golden/obl_l2_q_cat.npz"))
    (tmp_path / "cat.gbrl_model").write_bytes(g["model_file"].tobytes())
    cat = gbrl_amd.GBRL.load(str(tmp_path / "cat.gbrl_model"))
    with pytest.raises(RuntimeError, match="not available on a model with categorical columns"):
        cpp.shap_interactions_host(cat, np.zeros((4, 1), np.float32))
    # the calls on a data set, without a device: what is refused about the model comes before the missing data set
    reduce_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)

    class Collective(C.Structure):
        _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]

    sharded = hand_model("grd_d1_D1", tmp_path / "s.gbrl_model")
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_set_collective.argtypes = [C.c_void_p, C.c_void_p]
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    assert lib.gbrl_hip_set_collective(sharded._handle(), C.byref(coll)) == 0
    try:
        for model, text in ((m, "null data set"), (cat, "not available on a model with categorical columns"), (empty, "the model has no trees"),
                            (sharded, "collective hooks")):
            for call in (model.shap_interactions_prepared, model.shap_interaction_importance_prepared):
                with pytest.raises(RuntimeError, match=text):
                    call(None)
    finally:
        assert lib.gbrl_hip_set_collective(sharded._handle(), None) == 0
