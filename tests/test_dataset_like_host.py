"""CPU-side checks of the data sets that share thresholds and of fit_prepared's validation (include/gbrl_hip.h: gbrl_hip_dataset_create_like,
gbrl_hip_dataset_thresholds_id, gbrl_hip_fit_prepared_valid, gbrl_hip_early_stop_scan).  The stopping rule is host code and is checked in full here
on hand-made curves, against a three-line Python restatement; of the device calls, everything that is refused without a data set in hand,
through the C ABI with the documented status and through the binding.  The calls themselves run in tests/test_gpu_dataset_like.py and
tests/test_gpu_fit_valid.py."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

E_OK, E_INVALID = 0, -1
C_SYMBOLS = ("gbrl_hip_dataset_create_like", "gbrl_hip_dataset_thresholds_id", "gbrl_hip_fit_prepared_valid", "gbrl_hip_early_stop_scan")
NAN = float("nan")


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.gbrl_hip_early_stop_scan.argtypes = [vp, ci, ci, cd, vp, vp]
    lib.gbrl_hip_dataset_create_like.argtypes = [vp, vp, vp, ci, ci]
    lib.gbrl_hip_dataset_create_like.restype = vp
    lib.gbrl_hip_dataset_last_status.restype = ci
    lib.gbrl_hip_dataset_thresholds_id.argtypes = [vp]
    lib.gbrl_hip_dataset_thresholds_id.restype = C.c_uint64
    lib.gbrl_hip_fit_prepared_valid.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, cd, vp, vp, vp, vp]
    return lib


def _scan(curve, rounds, min_delta=0.0):
    lib = _lib()
    c = np.asarray(curve, np.float64)
    stop, best = C.c_int(-7), C.c_int(-7)
    rc = lib.gbrl_hip_early_stop_scan(c.ctypes.data, len(c), rounds, min_delta, C.byref(stop), C.byref(best))
    assert rc == E_OK, lib.gbrl_hip_last_error()
    return stop.value, best.value


def _rule(curve, rounds, min_delta=0.0):
    """the rule as the header states it: (stop_after, best)"""
    best = 0
    for k in range(1, len(curve)):
        best = k if curve[k] < curve[best] - min_delta else best
        if rounds > 0 and k - best >= rounds:
            return k, best
    return len(curve) - 1, best


def _empty(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def test_symbols_and_signatures():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for sym in C_SYMBOLS:
        assert hasattr(lib, sym), sym
    m = _empty()
    assert "reference" in m.prepare_dataset.__doc__ and "valid_targets" in m.fit_prepared.__doc__ and "early_stopping_rounds" in m.fit_prepared.__doc__
    assert hasattr(gbrl_amd.PreparedDataset, "thresholds_id")


@pytest.mark.parametrize("curve,rounds,min_delta,want", [
    ([5.0, 4.0, 3.0, 2.0, 1.0], 1, 0.0, (4, 4)),            # strictly falling: never stops
    ([5.0, 4.0, 3.0, 2.0, 1.0], 3, 0.0, (4, 4)),
    ([1.0, 2.0, 3.0, 4.0], 1, 0.0, (1, 0)),                 # rising from the start
    ([1.0, 2.0, 3.0, 4.0], 3, 0.0, (3, 0)),
    ([1.0, 2.0, 3.0, 4.0], 4, 0.0, (3, 0)),                 # the curve ends before the rule does
    ([2.0, 2.0, 2.0, 2.0], 2, 0.0, (2, 0)),                 # a plateau: equal is no improvement
    ([3.0, 2.0, 2.0, 2.0, 1.0], 2, 0.0, (3, 1)),
    ([3.0, 2.0, 2.0, 2.0, 1.0], 3, 0.0, (4, 4)),            # (k = 4 improves before k - best reaches 3)
    ([3.0, 2.9, 2.8, 2.7, 1.0], 2, 0.5, (2, 0)),            # min_delta turns the small gains into none
    ([3.0, 2.9, 2.8, 2.7, 1.0], 4, 0.5, (4, 4)),
    ([3.0, 2.4, 2.0], 1, 0.5, (2, 1)),                      # 2.4 < 2.5 improves, 2.0 < 1.9 does not
    ([3.0, 2.0, NAN, 1.0, 0.5], 1, 0.0, (2, 1)),            # a NaN never improves
    ([3.0, 2.0, NAN, 1.0, 0.5], 2, 0.0, (4, 4)),
    ([NAN, 1.0, 0.5], 1, 0.0, (1, 0)),                      # nor does anything improve on a NaN
    ([3.0, 4.0, 5.0, 1.0], 0, 0.0, (3, 3)),                 # rounds = 0 never stops
    ([7.0], 1, 0.0, (0, 0)),
])
def test_early_stop_scan_on_hand_made_curves(curve, rounds, min_delta, want):
    assert _scan(curve, rounds, min_delta) == want
    assert _rule(curve, rounds, min_delta) == want


def test_early_stop_scan_is_the_rule_on_random_curves():
    rng = np.random.default_rng(3)
    for _ in range(200):
        c = np.round(rng.standard_normal(int(rng.integers(1, 30))), 1)
        if rng.random() < 0.3:
            c[rng.integers(0, len(c))] = np.nan
        rounds, delta = int(rng.integers(0, 5)), float(rng.choice([0.0, 0.1, 0.5]))
        assert _scan(c, rounds, delta) == _rule(c, rounds, delta), (c.tolist(), rounds, delta)


def test_early_stop_scan_refuses_bad_arguments():
    lib = _lib()
    c = np.array([1.0, 2.0])
    s, b = C.c_int(0), C.c_int(0)
    assert lib.gbrl_hip_early_stop_scan(None, 2, 1, 0.0, C.byref(s), C.byref(b)) == E_INVALID
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, 0, 1, 0.0, C.byref(s), C.byref(b)) == E_INVALID
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, 2, -1, 0.0, C.byref(s), C.byref(b)) == E_INVALID
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, 2, 1, -0.5, C.byref(s), C.byref(b)) == E_INVALID
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, 2, 1, NAN, C.byref(s), C.byref(b)) == E_INVALID
    assert lib.gbrl_hip_early_stop_scan(c.ctypes.data, 2, 1, 0.0, None, C.byref(b)) == E_INVALID


def test_refusals_that_need_no_device(tmp_path):
    lib = _lib()
    err = lib.gbrl_hip_last_error
    m = _empty()
    p = tmp_path / "m.gbrl_model"
    assert m.save(str(p)) == 0
    before = p.read_bytes()
    X = np.zeros((8, 4), np.float32)
    Y = np.zeros((8, 2), np.float32)
    # create_like: a null reference, a handle that never was a data set
    assert lib.gbrl_hip_dataset_create_like(m._handle(), None, X.ctypes.data, 0, 8) is None
    assert lib.gbrl_hip_dataset_last_status() == E_INVALID and b"null data set" in err()
    bogus = C.c_void_p(0x1000)
    assert lib.gbrl_hip_dataset_create_like(m._handle(), bogus, X.ctypes.data, 0, 8) is None
    assert lib.gbrl_hip_dataset_last_status() == E_INVALID and b"destroyed" in err()
    assert lib.gbrl_hip_dataset_create_like(None, None, X.ctypes.data, 0, 8) is None and lib.gbrl_hip_dataset_last_status() == E_INVALID
    assert lib.gbrl_hip_dataset_thresholds_id(None) == 0 and lib.gbrl_hip_dataset_thresholds_id(bogus) == 0
    # fit_prepared_valid
    loss, done, best = C.c_float(0), C.c_int(0), C.c_int(0)
    curve = np.zeros(4, np.float64)
    def call(ds=None, valid=None, vt=Y.ctypes.data, rounds=0, delta=0.0, targets=Y.ctypes.data, iterations=3):
        return lib.gbrl_hip_fit_prepared_valid(m._handle(), ds, targets, 0, iterations, valid, vt, 0, rounds, delta, C.byref(loss), curve.ctypes.data,
                                               C.byref(done), C.byref(best))
    assert call() == E_INVALID and b"null data set" in err()                       # null data sets
    assert call(ds=bogus, valid=bogus) == E_INVALID and b"destroyed" in err()
    assert call(vt=None) == E_INVALID and b"valid_targets" in err()                # null valid targets
    assert call(rounds=-1) == E_INVALID and b"early_stopping_rounds" in err()      # negative rounds
    assert call(delta=NAN) == E_INVALID and b"min_delta" in err()                  # NaN min_delta
    assert call(delta=-1e-9) == E_INVALID and b"min_delta" in err()
    assert call(targets=None) == E_INVALID and b"targets" in err()                 # what fit_prepared refuses
    assert call(iterations=-1) == E_INVALID and b"iterations" in err()
    # the binding: without valid= the other three stay at their defaults
    for kw in (dict(valid_targets=Y), dict(early_stopping_rounds=1), dict(min_delta=0.5)):
        with pytest.raises(RuntimeError, match="need a validation set"):
            m.fit_prepared(None, Y, 3, **kw)
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, Y, 3)
    assert m.save(str(p)) == 0 and p.read_bytes() == before and m.get_num_trees() == 0
