"""The classifier metrics on the GPU (GBRL.eval_metric; include/gbrl_hip.h, "Classifier metrics").  tests/test_metric_host.py holds
gbrl_cpp.eval_metric_host to a NumPy brute force; here the device's integers are the host rule's, integer for integer, and the value the same
double.  The sizes sit around the sort's tile of 2048 elements (one tile, its edge, three tiles) and around the 64 lanes of a wave; the score
families cover both branches of the key, heavy ties (five values with both zeros and both infinities), one value everywhere, a perfect
separation and a run of 5000 equal keys across tile boundaries.  Columns of 32768, 32769 and 70001 rows (and a run of 40000 equal keys) are where
the sort's scan fills one slice of 4096 counts exactly and where it carries its sum into a second and a third."""
import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

host = gbrl_amd.gbrl_cpp.eval_metric_host
SIZES = (2, 63, 64, 65, 2047, 2048, 2049, 4097, 6145)
_MODELS = {}


def _model(D):
    if D not in _MODELS:
        m = gbrl_amd.GBRL(input_dim=3, output_dim=D, policy_dim=D, max_depth=3, n_bins=32, split_score_func="L2", generator_type="Quantile",
                          grow_policy="oblivious", device="cpu", batch_size=64)
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        _MODELS[D] = m
    return _MODELS[D]


def _shape(A, D):
    return np.ascontiguousarray(A[:, 0]) if D == 1 and A.ndim == 2 else np.ascontiguousarray(A)


def _dev(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def _targets(rng, n, D):
    """a positive and a negative row in every column; a few soft targets on either side of 0.5"""
    y = (rng.random((n, D)) < 0.35).astype(np.float32)
    y[0], y[1] = 1.0, 0.0
    if n > 8:
        y[2], y[3], y[4] = 0.5, 0.500001, 0.75
    return y


def _families(rng, n, D, y):
    five = np.float32([0.0, -0.0, np.inf, -np.inf, 1.5])
    separated = np.where(y > 0.5, 1.0, -1.0).astype(np.float32) * (1 + rng.random((n, D))).astype(np.float32)
    return {
        "distinct": rng.permutation(n * D).reshape(n, D).astype(np.float32) - np.float32(n * D // 2),
        "five_values": five[rng.integers(0, 5, (n, D))],
        "all_equal": np.full((n, D), -2.5, np.float32),
        "separated": separated,
        "reversed": -separated,
        "negative_only": -np.abs(rng.standard_normal((n, D))).astype(np.float32) - np.float32(0.25),
        "mixed_sign": rng.standard_normal((n, D)).astype(np.float32).round(2),
    }


def _same(got, want, what):
    (gv, gc), (wv, wc) = got, want
    assert gc.dtype == np.int64 and gc.shape == wc.shape, what
    assert gc.tolist() == wc.tolist(), what
    assert np.float64(gv).tobytes() == np.float64(wv).tobytes(), what


@pytest.mark.parametrize("D", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_device_counts_are_the_host_counts(n, D):
    _counts_are_the_host_counts(n, D)


SORT_TILE, SCAN_SLICE = 2048, 4096   # radix_sort.hip: the elements of a tile, the words of a column's 256 per tile that its scan takes per trip


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("n,slices", [(32768, 1), (32769, 2), (70001, 3)])
def test_device_counts_where_the_scan_takes_another_slice(n, slices, D):
    """16 tiles x 256 digits fill one slice of the sort's scan; from 32769 rows on it carries its running sum from slice to slice"""
    assert -(-256 * -(-n // SORT_TILE) // SCAN_SLICE) == slices and (n > 16 * SORT_TILE) == (slices > 1)
    _counts_are_the_host_counts(n, D)


def _counts_are_the_host_counts(n, D):
    rng = np.random.default_rng(8000 + 31 * n + D)
    m = _model(D)
    y = _targets(rng, n, D)
    for name, p in _families(rng, n, D, y).items():
        for metric in ("auc", "error"):
            _same(m.eval_metric(_shape(p, D), _shape(y, D), "logistic", metric), host(p, y, "logistic", metric), (name, metric))
    value, counts = m.eval_metric(_shape(np.full((n, D), 7.0, np.float32), D), _shape(y, D), "logistic", "auc")
    assert value == 0.5 and (counts[:, 0] == counts[:, 1] * counts[:, 2]).all()
    sep = _families(rng, n, D, y)["separated"]
    assert m.eval_metric(_shape(sep, D), _shape(y, D), "logistic", "auc")[0] == 1.0
    assert m.eval_metric(_shape(-sep, D), _shape(y, D), "logistic", "auc")[0] == 0.0


def test_one_row_is_a_single_class():
    m = _model(1)
    for y in (0.0, 1.0):
        with pytest.raises(RuntimeError, match="column 0 of the targets has no"):
            m.eval_metric(np.float32([0.25]), np.float32([y]), "logistic", "auc")
        assert m.eval_metric(np.float32([0.25]), np.float32([y]), "logistic", "error")[1].tolist() == [1 - int(y)]


def test_the_widest_model():
    rng = np.random.default_rng(8128)
    n, D = 300, 128
    y = _targets(rng, n, D)
    for name, p in _families(rng, n, D, y).items():
        for metric in ("auc", "error"):
            _same(_model(D).eval_metric(p, y, "logistic", metric), host(p, y, "logistic", metric), (name, metric))


def test_a_run_of_equal_keys_across_tiles():
    """one value at 5000 consecutive sorted positions of a column of 6145 rows (the run covers the whole of tile 1 and parts of tiles 0 and 2),
    distinct scores below and above it; the other columns have the run at other offsets"""
    rng = np.random.default_rng(8500)
    n, D = 6145, 3
    y = _targets(rng, n, D)
    p = np.empty((n, D), np.float32)
    for d, below in enumerate((600, 1145, 0)):
        col = np.concatenate([-1.0 - rng.permutation(below), np.full(5000, 0.125), 1.0 + rng.permutation(n - 5000 - below)]).astype(np.float32)
        p[:, d] = rng.permutation(col)
    want = host(p, y, "logistic", "auc")
    _same(_model(D).eval_metric(p, y, "logistic", "auc"), want, "tie run")
    assert 0.0 < want[0] < 1.0


def test_a_run_of_equal_keys_across_scan_slices():
    """one value at 40000 consecutive sorted positions of a column of 70001 rows (35 tiles, three slices of the scan: the run fills one digit's
    counts of some twenty tiles), distinct scores below and above it; the other columns have the run at other offsets"""
    rng = np.random.default_rng(8501)
    n, D, run = 70001, 3, 40000
    assert n > 16 * SORT_TILE and run > 16 * SORT_TILE
    y = _targets(rng, n, D)
    p = np.empty((n, D), np.float32)
    for d, below in enumerate((600, 30001, 0)):
        col = np.concatenate([-1.0 - rng.permutation(below), np.full(run, 0.125), 1.0 + rng.permutation(n - run - below)]).astype(np.float32)
        p[:, d] = rng.permutation(col)
    want = host(p, y, "logistic", "auc")
    _same(_model(D).eval_metric(p, y, "logistic", "auc"), want, "tie run")
    assert 0.0 < want[0] < 1.0


@pytest.mark.parametrize("D", [2, 4, 7])
def test_softmax_error(D):
    m = _model(D)
    for n in SIZES + (1,):
        rng = np.random.default_rng(8600 + 31 * n + D)
        labels = rng.integers(0, D, n).astype(np.int32)
        y = (labels[:, None] == np.arange(D)[None, :]).astype(np.float32)
        for name, p in _families(rng, n, D, y).items():
            if n > 3:
                p[1] = p[1, 0]; p[2, : D // 2 + 1] = p[2].max(); p[3] = -0.0; p[3, D - 1] = 0.0     # rows with equal maxima
            _same(m.eval_metric(p, labels, "softmax", "error"), host(p, labels, "softmax", "error"), (name, n))
    with pytest.raises(RuntimeError, match=r"label 7 \(row 1\) is outside"):
        m.eval_metric(np.zeros((3, D), np.float32), np.int32([0, 7, 1]), "softmax", "error")


def test_device_inputs_and_repeated_calls():
    import torch
    rng = np.random.default_rng(8700)
    n, D = 4097, 3
    m = _model(D)
    y = _targets(rng, n, D)
    p = rng.standard_normal((n, D)).astype(np.float32).round(2)
    labels = rng.integers(0, D, n).astype(np.int32)
    tp, ty, tl = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(labels).cuda()
    for targets, dev_targets, obj, metric in [(y, ty, "logistic", "auc"), (y, ty, "logistic", "error"), (labels, tl, "softmax", "error")]:
        want = host(p, targets, obj, metric)
        for pred_arg, tar_arg in [(p, targets), (_dev(tp), _dev(dev_targets)), (_dev(tp), targets), (p, _dev(dev_targets))]:
            first = m.eval_metric(pred_arg, tar_arg, obj, metric)
            again = m.eval_metric(pred_arg, tar_arg, obj, metric)
            _same(first, want, (obj, metric))
            assert first[1].tobytes() == again[1].tobytes() and np.float64(first[0]).tobytes() == np.float64(again[0]).tobytes()
    assert torch.equal(tp.cpu(), torch.from_numpy(p)) and torch.equal(ty.cpu(), torch.from_numpy(y))      # the inputs are only read


def test_refusals():
    m = _model(3)
    p, y = np.zeros((4, 3), np.float32), np.float32([[1, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 0]])
    with pytest.raises(RuntimeError, match="column 1 of the targets has no positive row"):
        m.eval_metric(p, y, "logistic", "auc")
    with pytest.raises(RuntimeError, match="Invalid metric"):
        m.eval_metric(p, y, "logistic", "f1")
    with pytest.raises(RuntimeError, match="the rmse objective has no metric"):
        m.eval_metric(p, y, "rmse", "error")
    with pytest.raises(RuntimeError, match="auc with the softmax objective"):
        m.eval_metric(p, np.zeros(4, np.int32), "softmax", "auc")
