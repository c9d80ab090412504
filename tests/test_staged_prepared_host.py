"""CPU-side checks of `predict_staged_prepared` / `staged_loss_prepared` (include/gbrl_hip.h): the binding's argument errors that need no device (there is no
data set without one, so `ds` is None and everything checked in front of the handle must already have spoken), and the C ABI's null-argument statuses."""
import ctypes
import os

import numpy as np
import pytest

import gbrl_amd

Y, L = np.zeros((8, 2), np.float32), np.zeros(8, np.int32)


def _model():
    m = gbrl_amd.GBRL(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2)
    return m


@pytest.mark.parametrize("kw,msg", [
    (dict(targets=Y, stops=None), "the model has no trees"), (dict(targets=Y, stops=[]), "stops is empty"), (dict(targets=Y, stops=[0, 0]), "strictly ascending"),
    (dict(targets=Y, stops=[1]), "out of bounds"), (dict(targets=None, stops=[0]), "without targets"),
    (dict(targets=np.zeros((8, 3), np.float32), stops=[0]), "Expected targets of shape"), (dict(targets=np.zeros(8, np.float32), stops=[0]), "Expected targets of shape"),
    (dict(targets=np.zeros((8, 2), np.int32), stops=[0], objective="softmax"), "int32 class labels of shape"),
    (dict(targets=Y, stops=[0], objective="logistic", eval_metric="auc"), "auc.*predict_staged_prepared"),
    (dict(targets=L, stops=[0], objective="pairwise"), "ranking objectives"), (dict(targets=L, stops=[0], objective="lambdarank"), "ranking objectives"),
    (dict(targets=Y, stops=[0]), "null data set"),                       # everything in front of the handle is in order
    (dict(stops=None), "the model has no trees"), (dict(stops=[3, 1]), "out of bounds"), (dict(stops=[0]), "null data set"),
])
def test_binding_argument_errors(kw, msg):
    kw = dict(kw)
    with pytest.raises(RuntimeError, match=msg):   # (a row without targets is the predict form)
        _model().staged_loss_prepared(None, kw.pop("targets"), **kw) if "targets" in kw else _model().predict_staged_prepared(None, **kw)


@pytest.mark.parametrize("golden,msg", [("obl_l2_q_cat", "not available on a model with categorical columns"), ("obl_l2_q", "collective hooks")])
def test_what_is_refused_about_the_model_comes_first(golden, msg, tmp_path):
    # (collective hooks installed as tests/test_shap_prepared_host.py installs them; refused before the data set is looked at, the file bytes stay)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", golden + ".npz"))
    (tmp_path / "m.gbrl_model").write_bytes(g["model_file"].tobytes())
    m = gbrl_amd.GBRL.load(str(tmp_path / "m.gbrl_model"))
    reduce_t = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
    Collective = type("Collective", (ctypes.Structure,), {"_fields_": [("ctx", ctypes.c_void_p), ("world_size", ctypes.c_int), ("rank", ctypes.c_int)] +
                                                                      [(n, reduce_t) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]})
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_set_collective.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    never = reduce_t(lambda ctx, buf, n: 1)
    coll = Collective(None, 2, 0, never, never, never, never)
    saved = lambda name: (m.save(str(tmp_path / name)), (tmp_path / name).read_bytes())
    before = saved("before")
    assert golden == "obl_l2_q_cat" or lib.gbrl_hip_set_collective(m._handle(), ctypes.byref(coll)) == 0
    try:
        D = np.asarray(m.get_bias()).size
        with pytest.raises(RuntimeError, match=msg):
            m.predict_staged_prepared(None, [0])
        with pytest.raises(RuntimeError, match=msg):
            m.staged_loss_prepared(None, np.zeros((8, D) if D > 1 else 8, np.float32), [0])
    finally:
        assert lib.gbrl_hip_set_collective(m._handle(), None) == 0
    assert saved("after") == before and before[0] == 0


def test_c_abi_null_arguments():
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gbrl_hip_predict_staged_prepared.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp, ci]
    lib.gbrl_hip_staged_loss_prepared.argtypes = [vp, vp, vp, ci, ci, vp, ci, ci, vp, vp, ci, ci, vp, ci, vp, vp, vp]
    err = lib.gbrl_hip_last_error
    h = _model()._handle()
    stops, out, loss = np.array([0], np.int32), np.zeros((1, 8, 2), np.float32), np.zeros(1, np.float64)
    predict = lambda handle, op: lib.gbrl_hip_predict_staged_prepared(handle, None, None, 0, 8, stops.ctypes.data, 1, op, 0)
    lossf = lambda handle, yp, lp: lib.gbrl_hip_staged_loss_prepared(handle, None, None, 0, 8, yp, 0, 0, None, None, 0, 0, stops.ctypes.data, 1, lp, None, None)
    assert predict(None, out.ctypes.data) == -1 and b"null model" in err()
    assert predict(h, out.ctypes.data) == -1 and b"null data set" in err()
    assert lossf(None, Y.ctypes.data, loss.ctypes.data) == -1 and b"null model" in err()
    assert lossf(h, Y.ctypes.data, loss.ctypes.data) == -1 and b"null data set" in err()
    assert not out.any() and not loss.any()
