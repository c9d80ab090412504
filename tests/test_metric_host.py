"""CPU-side checks of the classifier metrics (include/gbrl_hip.h, "Classifier metrics"; gbrl_amd/csrc/metric_core.h): gbrl_cpp.eval_metric_host
against a NumPy brute force -- the pair matrix for the AUC, the two error definitions written out -- with the counts compared as integers and
the values as exact doubles, and every refusal that needs no device, through the binding and through the C ABI with the documented status.
tests/test_gpu_metric.py then holds the device to these integers."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

E_INVALID, E_UNSUPPORTED = -1, -5
OBJ = {"rmse": 0, "logistic": 1, "softmax": 2}
METRIC = {"error": 1, "auc": 2}
C_SYMBOLS = ("gbrl_hip_eval_metric", "gbrl_hip_eval_metric_host", "gbrl_hip_fit_prepared_metric")
host = gbrl_amd.gbrl_cpp.eval_metric_host
SHAPES = [(1, 1), (2, 1), (7, 3), (64, 8), (257, 1), (1000, 3), (2000, 8)]


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_eval_metric_host.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    lib.gbrl_hip_eval_metric.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp]
    lib.gbrl_hip_fit_prepared_metric.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, C.c_double, C.c_double, C.c_double, C.c_uint64, ci, ci, vp, vp, vp, vp, vp]
    return lib


def brute_auc(p, y):
    """(value, counts [D, 3]) from the pair matrix of every column; scores compare as floats (-0.0 == +0.0), which is the key's order for
    everything but a NaN"""
    n, D = p.shape
    counts = np.zeros((D, 3), np.int64)
    total = 0.0
    for d in range(D):
        pos = y[:, d] > np.float32(0.5)
        s_pos, s_neg = p[pos, d], p[~pos, d]
        u2 = int((s_pos[:, None] > s_neg).sum()) * 2 + int((s_pos[:, None] == s_neg).sum())
        P, N = int(pos.sum()), int((~pos).sum())
        counts[d] = (u2, P, N)
        total += u2 / (2.0 * float(P) * float(N))
    return total / D, counts


def brute_error_logistic(p, y):
    wrong = ((p > 0) != (y > np.float32(0.5))).sum(axis=0).astype(np.int64)
    return int(wrong.sum()) / (p.shape[0] * p.shape[1]), wrong


def brute_error_softmax(p, labels):
    first_max = np.array([int(np.flatnonzero(row == row.max())[0]) for row in p])
    wrong = int((first_max != labels).sum())
    return wrong / p.shape[0], np.array([wrong], np.int64)


def both_classes(rng, n, D):
    """targets in {0, 1} with a positive and a negative row in every column (n >= 2)"""
    y = (rng.random((n, D)) < 0.4).astype(np.float32)
    y[0], y[1] = 1.0, 0.0
    return y


def score_families(rng, n, D):
    five = np.float32([0.0, -0.0, np.inf, -np.inf, 1.5])
    return {
        "distinct": rng.permutation(n * D).reshape(n, D).astype(np.float32) - np.float32(n * D / 2),
        "five_values": five[rng.integers(0, 5, (n, D))],
        "negative_only": -np.abs(rng.standard_normal((n, D))).astype(np.float32) - np.float32(0.25),
        "mixed_sign": rng.standard_normal((n, D)).astype(np.float32).round(1),
    }


def same(got, want_value, want_counts):
    value, counts = got
    assert counts.dtype == np.int64 and counts.shape == want_counts.shape
    assert counts.tolist() == want_counts.tolist()
    assert isinstance(value, float) and np.float64(value).tobytes() == np.float64(want_value).tobytes(), (value, want_value)


def test_c_symbols_and_python_names():
    lib = _lib()
    for name in C_SYMBOLS:
        assert hasattr(lib, name), name
    assert hasattr(gbrl_amd.GBRL, "eval_metric") and "eval_metric=None" in gbrl_amd.GBRL.fit_prepared.__doc__
    sig = gbrl_amd.GBRL.fit_prepared.__doc__.splitlines()[0]
    assert sig.endswith("-> float")   # the generated line of the three-argument form is kept


@pytest.mark.parametrize("n,D", [s for s in SHAPES if s[0] >= 2])
def test_auc_against_the_pair_matrix(n, D):
    rng = np.random.default_rng(7000 + 31 * n + D)
    y = both_classes(rng, n, D)
    for name, p in score_families(rng, n, D).items():
        same(host(p, y, "logistic", "auc"), *brute_auc(p, y))


@pytest.mark.parametrize("n,D", SHAPES)
def test_error_against_the_definitions(n, D):
    rng = np.random.default_rng(7100 + 31 * n + D)
    y = (rng.random((n, D)) < 0.4).astype(np.float32)
    for name, p in score_families(rng, n, D).items():
        same(host(p, y, "logistic", "error"), *brute_error_logistic(p, y))
    if D >= 2:
        labels = rng.integers(0, D, n).astype(np.int32)
        for name, p in score_families(rng, n, D).items():
            same(host(p, labels, "softmax", "error"), *brute_error_softmax(p, labels))


def test_auc_of_equal_and_of_separated_scores():
    rng = np.random.default_rng(7200)
    n, D = 1500, 3
    y = both_classes(rng, n, D)
    value, counts = host(np.full((n, D), -2.5, np.float32), y, "logistic", "auc")
    assert value == 0.5 and (counts[:, 0] == counts[:, 1] * counts[:, 2]).all()     # 2U == P * N
    up = np.where(y > 0.5, 1.0, -1.0).astype(np.float32) * (1 + rng.random((n, D))).astype(np.float32)
    value, counts = host(up, y, "logistic", "auc")
    assert value == 1.0 and (counts[:, 0] == 2 * counts[:, 1] * counts[:, 2]).all()
    value, counts = host(-up, y, "logistic", "auc")
    assert value == 0.0 and (counts[:, 0] == 0).all()


def test_key_order_of_zeros_infinities_and_nan():
    y = np.float32([[1], [0]])
    for a, b, want in [(0.0, -0.0, 0.5), (-0.0, 0.0, 0.5), (np.inf, 3e38, 1.0), (-np.inf, -3e38, 0.0), (1e-45, 0.0, 1.0), (-1e-45, -0.0, 0.0)]:
        assert host(np.float32([[a], [b]]), y, "logistic", "auc")[0] == want, (a, b)
    # a NaN is ordered by its bits: above +inf with the sign clear, below -inf with it set (defined; meaningless)
    nan_pos = np.uint32([0x7fc00000]).view(np.float32)[0]
    nan_neg = np.uint32([0xffc00000]).view(np.float32)[0]
    assert host(np.float32([[nan_pos], [np.inf]]), y, "logistic", "auc")[0] == 1.0
    assert host(np.float32([[nan_neg], [-np.inf]]), y, "logistic", "auc")[0] == 0.0


def test_edge_cells():
    # p == 0 (either zero) predicts the negative class; a NaN score does too
    p = np.float32([[0.0], [-0.0], [1e-45], [np.nan]])
    assert host(p, np.float32([[1], [1], [1], [1]]), "logistic", "error")[1].tolist() == [3]
    assert host(p, np.float32([[0], [0], [0], [0]]), "logistic", "error")[1].tolist() == [1]
    # soft targets: 0.5 is negative, 0.500001 positive
    soft = np.float32([[0.5], [0.500001]])
    assert host(np.float32([[1.0], [1.0]]), soft, "logistic", "error")[1].tolist() == [1]
    assert host(np.float32([[-1.0], [-1.0]]), soft, "logistic", "error")[1].tolist() == [1]
    value, counts = host(np.float32([[0.0], [2.0]]), soft, "logistic", "auc")
    assert counts.tolist() == [[2, 1, 1]] and value == 1.0
    # soft-max rows with equal maxima take the lowest index; -0.0 == +0.0 among them
    p = np.float32([[1, 3, 3, 0], [2, 2, 2, 2], [-0.0, 0.0, -1, -2], [0.0, -0.0, -1, -2], [-np.inf, -np.inf, -np.inf, -np.inf]])
    for labels, wrong in [([1, 0, 0, 0, 0], 0), ([2, 1, 1, 1, 3], 5), ([1, 3, 0, 1, 0], 2)]:
        value, counts = host(p, np.int32(labels), "softmax", "error")
        assert counts.tolist() == [wrong] and value == wrong / 5


def test_refusals_through_the_binding():
    p, y = np.zeros((4, 2), np.float32), np.float32([[1, 0], [0, 0], [1, 0], [0, 0]])
    with pytest.raises(RuntimeError, match="column 1 of the targets has no positive row"):
        host(p, y, "logistic", "auc")
    with pytest.raises(RuntimeError, match="column 1 of the targets has no negative row"):
        host(p, 1 - y, "logistic", "auc")
    with pytest.raises(RuntimeError, match="column 0 of the targets has no negative row"):
        host(p, np.ones_like(y), "logistic", "auc")                                                 # the first such column is named
    with pytest.raises(RuntimeError, match="column 0 of the targets has no"):
        host(np.zeros((1, 1), np.float32), np.ones((1, 1), np.float32), "logistic", "auc")          # n = 1: a single class
    with pytest.raises(RuntimeError, match="Invalid metric! Options are: error/auc"):
        host(p, y, "logistic", "accuracy")
    for metric in ("error", "auc"):
        with pytest.raises(RuntimeError, match="the rmse objective has no metric"):
            host(p, y, "rmse", metric)
    with pytest.raises(RuntimeError, match="auc with the softmax objective"):
        host(p, np.zeros(4, np.int32), "softmax", "auc")
    with pytest.raises(RuntimeError, match=r"label 2 \(row 3\) is outside \[0, 2\)"):
        host(p, np.int32([0, 1, 0, 2]), "softmax", "error")
    with pytest.raises(RuntimeError, match="Expected array of format 'i'"):
        host(p, y, "softmax", "error")                                                              # float targets where labels are wanted
    with pytest.raises(RuntimeError, match="int32 class labels of shape"):
        host(p, np.zeros(3, np.int32), "softmax", "error")
    with pytest.raises(RuntimeError, match="Expected targets of shape"):
        host(p, y[:3], "logistic", "error")


def test_refusals_through_the_c_abi():
    lib = _lib()
    p, y = np.zeros((4, 2), np.float32), np.float32([[1, 0], [0, 0], [1, 0], [0, 0]])
    labels = np.zeros(4, np.int32)
    value, counts = C.c_double(-3.0), np.full(6, -9, np.int64)

    def call(pred, tar, n, D, objective, metric, v=value, c=counts):
        return lib.gbrl_hip_eval_metric_host(pred.ctypes.data if pred is not None else None, tar.ctypes.data if tar is not None else None, n, D, objective,
                                             metric, C.byref(v) if v is not None else None, c.ctypes.data if c is not None else None)
    assert call(p, y, 4, 2, OBJ["logistic"], METRIC["auc"]) == E_INVALID and b"column 1" in lib.gbrl_hip_last_error()
    assert call(p, y, 4, 2, OBJ["logistic"], 0) == E_INVALID and b"unknown metric 0" in lib.gbrl_hip_last_error()
    assert call(p, y, 4, 2, OBJ["logistic"], 3) == E_INVALID and b"unknown metric 3" in lib.gbrl_hip_last_error()
    assert call(p, y, 4, 2, OBJ["rmse"], METRIC["error"]) == E_INVALID and b"rmse" in lib.gbrl_hip_last_error()
    assert call(p, labels, 4, 2, OBJ["softmax"], METRIC["auc"]) == E_UNSUPPORTED and b"softmax" in lib.gbrl_hip_last_error()
    assert call(p, y, 4, 2, 7, METRIC["error"]) == E_INVALID and b"unknown objective" in lib.gbrl_hip_last_error()
    assert call(p, y, 0, 2, OBJ["logistic"], METRIC["error"]) == E_INVALID and b"no rows" in lib.gbrl_hip_last_error()
    assert call(None, y, 4, 2, OBJ["logistic"], METRIC["error"]) == E_INVALID
    assert call(p, None, 4, 2, OBJ["logistic"], METRIC["error"]) == E_INVALID
    assert call(p, y, 4, 2, OBJ["logistic"], METRIC["error"], v=None, c=None) == E_INVALID
    assert value.value == -3.0 and (counts == -9).all(), "a refused call wrote a result"
    assert call(p, y, 4, 2, OBJ["logistic"], METRIC["error"], c=None) == 0 and value.value == 0.25    # either output alone is enough
    assert call(p, y, 4, 2, OBJ["logistic"], METRIC["error"], v=None) == 0 and counts[:2].tolist() == [2, 0]


def _model(tmp_path, D=2):
    m = gbrl_amd.GBRL(input_dim=4, output_dim=D, policy_dim=D, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious",
                      device="cpu")
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    path = tmp_path / "state.gbrl_model"
    assert m.save(str(path)) == 0
    return m, path


def test_auc_refuses_more_cells_than_the_sort_indexes(tmp_path):
    """n * D >= 2^31 - 2048 is refused (unsupported) before the device or the arrays are touched: 2^24 rows of 128 outputs are 2^31 cells"""
    m, _ = _model(tmp_path, D=128)
    lib = _lib()
    p, value = np.zeros((2, 128), np.float32), C.c_double(-3.0)
    rc = lib.gbrl_hip_eval_metric(m._handle(), p.ctypes.data, 0, p.ctypes.data, 0, 1 << 24, OBJ["logistic"], METRIC["auc"], C.byref(value), None)
    assert rc == E_UNSUPPORTED and b"2^31 - 2048" in lib.gbrl_hip_last_error() and value.value == -3.0


def test_fit_refusals_that_need_no_data_set(tmp_path):
    """A metric without a validation set is refused before a data set handle is looked at (None here), with the model's bytes unchanged; the
    refusals that need a validation set in hand are in tests/test_gpu_fit_metric.py."""
    m, path = _model(tmp_path)
    before = path.read_bytes()
    y = np.zeros((8, 2), np.float32)
    lib = _lib()
    loss, done, best = C.c_float(), C.c_int(), C.c_int()

    def fit(objective, metric):
        rc = lib.gbrl_hip_fit_prepared_metric(m._handle(), None, y.ctypes.data, 0, 3, None, None, 0, 0, 0.0, 1.0, 1.0, 0, objective, metric, C.byref(loss), None,
                                              None, C.byref(done), C.byref(best))
        return rc, lib.gbrl_hip_last_error()
    rc, msg = fit(OBJ["logistic"], METRIC["error"])
    assert rc == E_INVALID and b"eval_metric needs a validation set" in msg
    rc, msg = fit(OBJ["logistic"], 9)
    assert rc == E_INVALID and b"eval_metric needs a validation set" in msg      # (without a validation set that is the first thing wrong)
    rc, msg = fit(OBJ["logistic"], 0)
    assert rc == E_INVALID and b"null data set" in msg                           # no metric: the call goes on to the data set
    assert m.save(str(path)) == 0 and path.read_bytes() == before
    for metric in ("error", "auc"):
        with pytest.raises(RuntimeError, match="eval_metric needs a validation set"):
            m.fit_prepared(None, y, 3, objective="logistic", eval_metric=metric)
    with pytest.raises(RuntimeError, match="Invalid metric! Options are: error/auc"):
        m.fit_prepared(None, y, 3, objective="logistic", eval_metric="logloss")
    assert m.save(str(path)) == 0 and path.read_bytes() == before
