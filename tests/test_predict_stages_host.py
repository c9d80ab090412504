"""Which error wins when a predict-family call breaks two rules at once, and what a refused call leaves in the model's metadata.

The nine entry points -- predict, predict_encoded, predict_continue, predict_continue_encoded, predict_staged, staged_loss, predict_leaves,
leaf_counts, refit_leaves -- share their batch checks and differ in where their own checks sit: for every call but refit_leaves the batch
checks ("Incompatible dataset", "Cannot call predict without observations!", output_dim > 128) come first; refit_leaves checks trees, range,
targets and decay before it looks at the batch.  Every call below is refused before a device is needed, so the file needs no GPU.

The model without trees has 3 numeric and 2 categorical inputs and 2 outputs; where trees are needed the loaded models are tests/golden's
obl_l2_q_cat (6 numeric + 2 categorical inputs, 2 outputs) and the 257-output model of the SHAP edge fixtures."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd
from helpers import load_golden

E_INVALID, E_UNSUPPORTED = -1, -5
F, FC, D = 3, 2, 2
N = 8


def _empty(**kw):
    base = dict(input_dim=F + FC, output_dim=D, policy_dim=D, max_depth=3, split_score_func="L2", generator_type="Quantile",
                grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def _loaded(tmp_path):
    _, g, (X, Xc, _, _) = load_golden("obl_l2_q_cat")
    p = tmp_path / "obl_l2_q_cat.gbrl_model"
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p)), np.ascontiguousarray(X[:N]), np.ascontiguousarray(Xc[:N])


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, u64, dbl = C.c_void_p, C.c_int, C.c_uint64, C.c_double
    batch, enc = [vp, vp, ci, vp, ci, ci, ci, ci], [vp, vp, ci, vp, ci, u64, ci, ci, ci]
    lib.gbrl_hip_predict.argtypes = batch + [ci, ci, vp, ci]
    lib.gbrl_hip_predict_encoded.argtypes = enc + [ci, ci, vp, ci]
    lib.gbrl_hip_predict_continue.argtypes = batch + [ci, ci, vp, ci, vp, ci]
    lib.gbrl_hip_predict_continue_encoded.argtypes = enc + [ci, ci, vp, ci, vp, ci]
    lib.gbrl_hip_predict_staged.argtypes = batch + [vp, ci, vp, ci]
    lib.gbrl_hip_staged_loss.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, vp, ci, vp]
    lib.gbrl_hip_predict_leaves.argtypes = batch + [ci, ci, vp, ci]
    lib.gbrl_hip_leaf_counts.argtypes = batch + [ci, ci, vp]
    lib.gbrl_hip_refit_leaves.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, dbl, vp]
    lib.gbrl_hip_get_metadata.argtypes = [vp, vp]
    return lib


def _latched(lib, m):
    """(n_num_features, n_cat_features, iteration): words 17..19 of the 80-byte metadata (include/gbrl_hip.h)."""
    md = (C.c_int32 * 20)()
    assert lib.gbrl_hip_get_metadata(m._handle(), md) == 0
    return md[17], md[18], md[19]


class Calls:
    """The nine C entry points on one model and one host batch; every keyword is one argument to get wrong."""

    def __init__(self, lib, m, X, Xc, n_outputs, n_trees):
        self.lib, self.h, self.X, self.Xc = lib, m._handle(), X, Xc
        self.f, self.fc = X.shape[1], (Xc.shape[1] if Xc is not None else 0)
        self.out = np.zeros((max(n_trees, 1) + 1, N, n_outputs), np.float32)     # wide enough for every call's result
        self.Y = np.zeros((N, n_outputs), np.float32)
        self.ids = np.zeros((N, max(self.fc, 1)), np.int32)
        self.loss = np.full(4, -7.0, np.float64)
        self.stops = np.array([0], np.int32)
        self.O, self.YP, self.L = self.out.ctypes.data, self.Y.ctypes.data, self.loss.ctypes.data

    def _batch(self, n, f, fc):
        return (self.h, self.X.ctypes.data, 0, self.Xc.ctypes.data if self.Xc is not None else None, 0, n, self.f if f is None else f, self.fc if fc is None else fc)

    def _enc(self, n, f, fc, ids):
        return (self.h, self.X.ctypes.data, 0, self.ids.ctypes.data if ids == "ids" else ids, 0, 12345, n, self.f if f is None else f, self.fc if fc is None else fc)

    def _stops(self, stops):
        stops = self.stops if stops is None else np.asarray(stops, np.int32)
        return (stops.ctypes.data if stops.size else None), int(stops.size), stops

    def predict(self, n=N, f=None, fc=None, a=0, b=0, out="out"):
        return self.lib.gbrl_hip_predict(*self._batch(n, f, fc), a, b, self.O if out == "out" else out, 0)

    def predict_encoded(self, n=N, f=None, fc=None, a=0, b=0, out="out", ids="ids"):
        return self.lib.gbrl_hip_predict_encoded(*self._enc(n, f, fc, ids), a, b, self.O if out == "out" else out, 0)

    def predict_continue(self, n=N, f=None, fc=None, a=0, b=0, base="out", out="out"):
        return self.lib.gbrl_hip_predict_continue(*self._batch(n, f, fc), a, b, self.O if base == "out" else base, 0, self.O if out == "out" else out, 0)

    def predict_continue_encoded(self, n=N, f=None, fc=None, a=0, b=0, base="out", out="out", ids="ids"):
        return self.lib.gbrl_hip_predict_continue_encoded(*self._enc(n, f, fc, ids), a, b, self.O if base == "out" else base, 0, self.O if out == "out" else out, 0)

    def predict_staged(self, n=N, f=None, fc=None, stops=None, out="out"):
        sp, ns, keep = self._stops(stops)
        return self.lib.gbrl_hip_predict_staged(*self._batch(n, f, fc), sp, ns, self.O if out == "out" else out, 0)

    def staged_loss(self, n=N, f=None, fc=None, stops=None, y="y", loss="loss"):
        sp, ns, keep = self._stops(stops)
        b = self._batch(n, f, fc)
        return self.lib.gbrl_hip_staged_loss(*b[:5], self.YP if y == "y" else y, 0, *b[5:], sp, ns, self.L if loss == "loss" else loss)

    def predict_leaves(self, n=N, f=None, fc=None, a=0, b=0, out="out"):
        return self.lib.gbrl_hip_predict_leaves(*self._batch(n, f, fc), a, b, self.O if out == "out" else out, 0)

    def leaf_counts(self, n=N, f=None, fc=None, a=0, b=0, out="out"):
        return self.lib.gbrl_hip_leaf_counts(*self._batch(n, f, fc), a, b, self.O if out == "out" else out)

    def refit_leaves(self, n=N, f=None, fc=None, a=0, b=0, decay=0.0, y="y", loss="loss"):
        bt = self._batch(n, f, fc)
        return self.lib.gbrl_hip_refit_leaves(*bt[:5], self.YP if y == "y" else y, 0, *bt[5:], a, b, decay, self.L if loss == "loss" else loss)


def _refused(lib, rc, status, text):
    msg = lib.gbrl_hip_last_error()
    assert rc == status and text in msg, (rc, msg)


@pytest.fixture()
def empty_calls():
    lib = _lib()
    m = _empty()
    X = np.zeros((N, F), np.float32)
    Xc = np.full((N, FC), b"a", dtype="S128")
    return lib, m, Calls(lib, m, X, Xc, D, 0)


@pytest.fixture()
def loaded_calls(tmp_path):
    lib = _lib()
    m, X, Xc = _loaded(tmp_path)
    assert m.get_num_trees() >= 2
    return lib, m, Calls(lib, m, X, Xc, D, m.get_num_trees())


def test_a_wrong_feature_count_wins_over_a_missing_result_base_targets_or_stops(empty_calls, loaded_calls):
    for lib, m, c in (empty_calls, loaded_calls):
        bad = dict(f=c.f - 1)                                                 # n_num + n_cat != input_dim
        swapped = dict(f=c.f - 1, fc=c.fc + 1)                                # the sum is right, the split is not (loaded: the file's; fresh: latched by the call itself)
        for kw in (bad,) if m.get_num_trees() == 0 else (bad, swapped):
            _refused(lib, c.predict(out=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_encoded(out=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_continue(base=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_continue(base=None, out=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_continue_encoded(base=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_staged(stops=[], **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_staged(stops=[], out=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.staged_loss(y=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.staged_loss(stops=[], **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.predict_leaves(out=None, **kw), E_INVALID, b"Incompatible dataset")
            _refused(lib, c.leaf_counts(out=None, **kw), E_INVALID, b"Incompatible dataset")
        # the _encoded wrappers ask for their ids before anything else
        _refused(lib, c.predict_encoded(ids=None, **bad), E_INVALID, b"Cannot call predict without observations!")
        _refused(lib, c.predict_continue_encoded(ids=None, base=None, **bad), E_INVALID, b"Cannot call predict without observations!")
        # with the right feature count: a missing result before a missing base, empty stops or missing targets; then the call's own checks in order
        _refused(lib, c.predict_continue(base=None, out=None), E_INVALID, b"Cannot call predict without observations!")
        _refused(lib, c.predict_continue(base=None, a=5, b=1), E_INVALID, b"predict_continue: no base prediction")
        _refused(lib, c.predict_continue(a=5, b=1), E_INVALID, b"predict_continue: invalid tree range")
        _refused(lib, c.predict_continue(a=-1, base=None), E_INVALID, b"invalid tree range")
        assert b"predict_continue" not in lib.gbrl_hip_last_error()          # (the shared sign check, before the call's own)
        _refused(lib, c.predict_staged(stops=[], out=None), E_INVALID, b"Cannot call predict without observations!")
        _refused(lib, c.predict_staged(stops=[]), E_INVALID, b"staged evaluation: stops is empty")
        _refused(lib, c.staged_loss(stops=[], y=None), E_INVALID, b"staged evaluation: stops is empty")
        _refused(lib, c.staged_loss(y=None, loss=None), E_INVALID, b"Cannot call staged_loss without targets!")
        _refused(lib, c.staged_loss(loss=None), E_INVALID, b"staged_loss: no output array")
        _refused(lib, c.staged_loss(n=0, y=None), E_INVALID, b"Cannot call predict without observations!")
        assert np.all(c.loss == -7.0) and not c.out.any()                     # no refused call wrote a result


def test_refit_leaves_checks_its_own_arguments_before_the_batch(loaded_calls):
    lib, m, c = loaded_calls
    T = m.get_num_trees()
    bad = dict(f=c.f - 1)
    _refused(lib, c.refit_leaves(y=None, **bad), E_INVALID, b"Cannot call refit_leaves without targets!")
    _refused(lib, c.refit_leaves(a=T, **bad), E_INVALID, b"refit_leaves: invalid tree range")
    _refused(lib, c.refit_leaves(a=-1, **bad), E_INVALID, b"refit_leaves: invalid tree range")
    _refused(lib, c.refit_leaves(a=T, y=None), E_INVALID, b"refit_leaves: invalid tree range")       # range, then targets
    _refused(lib, c.refit_leaves(y=None, loss=None), E_INVALID, b"Cannot call refit_leaves without targets!")
    _refused(lib, c.refit_leaves(loss=None, decay=2.0, **bad), E_INVALID, b"refit_leaves: no place for the loss")
    _refused(lib, c.refit_leaves(decay=2.0, **bad), E_INVALID, b"refit_leaves: decay_rate must be in [0, 1]")
    _refused(lib, c.refit_leaves(decay=float("nan"), n=0), E_INVALID, b"refit_leaves: decay_rate must be in [0, 1]")
    _refused(lib, c.refit_leaves(**bad), E_INVALID, b"Incompatible dataset")
    _refused(lib, c.refit_leaves(f=c.f - 1, fc=c.fc + 1), E_INVALID, b"Incompatible dataset")
    _refused(lib, c.refit_leaves(n=0), E_INVALID, b"Cannot call predict without observations!")
    assert np.all(c.loss == -7.0)


def test_a_model_without_trees_loses_to_the_feature_count_for_the_leaf_calls_and_wins_for_refit(empty_calls):
    lib, m, c = empty_calls
    bad = dict(f=F - 1)
    for call in (c.predict_leaves, c.leaf_counts):
        _refused(lib, call(**bad), E_INVALID, b"Incompatible dataset")
        _refused(lib, call(out=None), E_INVALID, b"Cannot call predict without observations!")
        _refused(lib, call(a=-1), E_INVALID, b"invalid tree range")           # the shared sign check sits before "no trees"
        assert b"predict_leaves" not in lib.gbrl_hip_last_error()
        _refused(lib, call(a=3, b=1), E_INVALID, b"predict_leaves: the model has no trees")
        _refused(lib, call(), E_INVALID, b"predict_leaves: the model has no trees")
    _refused(lib, c.refit_leaves(**bad), E_INVALID, b"refit_leaves: the model has no trees")
    _refused(lib, c.refit_leaves(n=0, y=None, loss=None, a=-1, decay=7.0, **bad), E_INVALID, b"refit_leaves: the model has no trees")
    # through the binding the shape inference speaks first for both, then each call's own "no trees"
    X, Xc, Y = np.zeros((N, F), np.float32), np.full((N, FC), b"a", dtype="S128"), np.zeros((N, D), np.float32)
    for call in (lambda o: m.predict_leaves(o, Xc), lambda o: m.leaf_counts(o, Xc), lambda o: m.refit_leaves(o, Xc, Y)):
        with pytest.raises(RuntimeError, match="Total number of features 4 != input dim 5"):
            call(X[:, :-1].copy())
    with pytest.raises(RuntimeError, match="^predict_leaves: the model has no trees$"):
        m.predict_leaves(X, Xc, 3, 1)
    with pytest.raises(RuntimeError, match="^leaf_counts: the model has no trees$"):
        m.leaf_counts(X, Xc, 3, 1)
    with pytest.raises(RuntimeError, match="^refit_leaves: the model has no trees$"):
        m.refit_leaves(X, Xc, Y, 3, 1)
    with pytest.raises(RuntimeError, match="^Expected targets of shape \\(8, 2\\), but got \\(8, 3\\)$"):
        m.refit_leaves(X, Xc, np.zeros((N, 3), np.float32), 3, 1)              # (the binding's shape check, before the engine's "no trees")


def test_the_width_limit_wins_over_a_bad_range_for_predict_and_does_not_exist_for_predict_leaves(tmp_path):
    from shap_edges import fixture, load_model
    name = "host_d4_D257_obl"
    m = load_model(name, tmp_path)
    X = np.ascontiguousarray(fixture(name)[2][:N])
    T, wide = m.get_num_trees(), np.asarray(m.get_bias()).size
    assert wide > 128 and T >= 1
    lib = _lib()
    c = Calls(lib, m, X, None, wide, T)
    for kw in (dict(a=-1), dict(b=-1), dict(a=T + 3, b=T + 5), dict()):
        _refused(lib, c.predict(**kw), E_UNSUPPORTED, b"predict: output_dim > 128")
        _refused(lib, c.predict_continue(**kw), E_UNSUPPORTED, b"predict: output_dim > 128")
    _refused(lib, c.predict_staged(stops=[]), E_UNSUPPORTED, b"predict: output_dim > 128")
    _refused(lib, c.staged_loss(stops=[2, 1], y=None), E_UNSUPPORTED, b"predict: output_dim > 128")
    _refused(lib, c.predict(f=X.shape[1] - 1), E_INVALID, b"Incompatible dataset")       # (the batch before the width)
    _refused(lib, c.predict(out=None), E_INVALID, b"Cannot call predict without observations!")
    for call in (c.predict_leaves, c.leaf_counts):
        _refused(lib, call(a=-1), E_INVALID, b"invalid tree range")
        assert b"predict_leaves" not in lib.gbrl_hip_last_error()
        _refused(lib, call(a=T + 3, b=T + 5), E_INVALID, b"predict_leaves: invalid tree range")
        _refused(lib, call(a=T, b=0), E_INVALID, b"predict_leaves: invalid tree range")
    _refused(lib, c.refit_leaves(a=T), E_INVALID, b"refit_leaves: invalid tree range")   # refit: its range before the width ...
    _refused(lib, c.refit_leaves(), E_UNSUPPORTED, b"predict: output_dim > 128")         # ... which it has
    # the binding: predict's own bounds wording first, then the engine's width limit
    with pytest.raises(RuntimeError, match="^start_tree_idx is out of bounds! Got -1, but valid range is \\[0, %d\\]$" % (T - 1)):
        m.predict(X, None, -1, 0)
    with pytest.raises(RuntimeError, match="^stop_tree_idx is out of bounds! Got %d, but valid range is \\[0, %d\\]$" % (T + 1, T)):
        m.predict(None, None, 0, T + 1)                                                    # (before the missing observations)
    with pytest.raises(RuntimeError, match="^predict: output_dim > 128$"):
        m.predict(X, None, 0, 0)
    with pytest.raises(RuntimeError, match="^predict_leaves: invalid tree range \\[%d, 0\\) for %d trees$" % (T, T)):
        m.predict_leaves(X, None, T, 0)


def test_descending_stops_win_over_missing_targets_for_staged_loss(loaded_calls):
    lib, m, c = loaded_calls
    _refused(lib, c.staged_loss(stops=[2, 1], y=None), E_INVALID, b"staged evaluation: stops must be strictly ascending")
    _refused(lib, c.staged_loss(stops=[1, 1], y=None, loss=None), E_INVALID, b"staged evaluation: stops must be strictly ascending")
    _refused(lib, c.staged_loss(stops=[1, 9], y=None), E_INVALID, b"staged evaluation: a stop is out of bounds! Got 9, but valid range is [0, %d]" % m.get_num_trees())
    _refused(lib, c.staged_loss(stops=[9, 1], y=None), E_INVALID, b"a stop is out of bounds")                 # stop by stop: bounds, then order
    _refused(lib, c.staged_loss(stops=[1, 2], y=None), E_INVALID, b"Cannot call staged_loss without targets!")
    # the binding reads the targets before the stops
    X, Xc = c.X, c.Xc
    with pytest.raises(RuntimeError, match="^Cannot call staged_loss without targets!$"):
        m.staged_loss(X, Xc, None, [2, 1])
    with pytest.raises(RuntimeError, match="^Expected targets of shape \\(8, 2\\), but got \\(8\\)$"):
        m.staged_loss(X, Xc, np.zeros(N, np.float32), [2, 1])
    with pytest.raises(RuntimeError, match="^stops must be strictly ascending$"):
        m.staged_loss(X, Xc, c.Y, [2, 1])
    with pytest.raises(RuntimeError, match="^Total number of features 7 != input dim 8$"):
        m.predict_staged(X[:, :-1].copy(), Xc, [])                                                          # the batch before the stops
    with pytest.raises(RuntimeError, match="^stops is empty: nothing to evaluate$"):
        m.predict_staged(X, Xc, [])


def test_binding_reads_observations_then_base_or_targets_then_shapes(loaded_calls):
    lib, m, c = loaded_calls
    X, Xc, Y = c.X, c.Xc, c.Y
    for fn, call in (("predict", lambda o, k: m.predict(o, k)), ("predict_continue", lambda o, k: m.predict_continue(o, k, None)),
                     ("predict_staged", lambda o, k: m.predict_staged(o, k, [])), ("staged_loss", lambda o, k: m.staged_loss(o, k, None, [])),
                     ("predict_leaves", lambda o, k: m.predict_leaves(o, k, 5, 1)), ("leaf_counts", lambda o, k: m.leaf_counts(o, k, 5, 1)),
                     ("refit_leaves", lambda o, k: m.refit_leaves(o, k, None, 5, 1))):
        with pytest.raises(RuntimeError, match="^Cannot call %s without observations!$" % fn):
            call(None, None)
    with pytest.raises(RuntimeError, match="^Cannot call predict_continue without base!$"):
        m.predict_continue(X[:, :-1].copy(), Xc, None)
    with pytest.raises(RuntimeError, match="^Total number of features 7 != input dim 8$"):
        m.predict_continue(X[:, :-1].copy(), Xc, np.zeros((N, 3), np.float32))
    with pytest.raises(RuntimeError, match="^Expected base of shape \\(8, 2\\), but got \\(8, 3\\)$"):
        m.predict_continue(X, Xc, np.zeros((N, 3), np.float32), 5, 1)
    with pytest.raises(RuntimeError, match="^predict_continue: invalid tree range$"):
        m.predict_continue(X, Xc, Y, 5, 1)
    with pytest.raises(RuntimeError, match="^Cannot call refit_leaves without targets!$"):
        m.refit_leaves(X[:, :-1].copy(), Xc, None, 5, 1)
    with pytest.raises(RuntimeError, match="^Total number of features 7 != input dim 8$"):
        m.refit_leaves(X[:, :-1].copy(), Xc, np.zeros((N, 3), np.float32), 5, 1)
    with pytest.raises(RuntimeError, match="^Expected targets of shape \\(8, 2\\), but got \\(8, 3\\)$"):
        m.refit_leaves(X, Xc, np.zeros((N, 3), np.float32), 5, 1)
    with pytest.raises(RuntimeError, match="^refit_leaves: invalid tree range \\[5, 1\\) for 2 trees$"):
        m.refit_leaves(X, Xc, Y, 5, 1)
    # one output: [n] is a shape too, and the message says so
    one = _empty(output_dim=1, policy_dim=1)
    X5, Xc5 = np.zeros((N, F), np.float32), np.full((N, FC), b"a", dtype="S128")
    for call in (lambda y: one.predict_continue(X5, Xc5, y), lambda y: one.staged_loss(X5, Xc5, y, [0]), lambda y: one.refit_leaves(X5, Xc5, y)):
        with pytest.raises(RuntimeError, match="^Expected (base|targets) of shape \\(8, 1\\) or \\(8,\\), but got \\(7\\)$"):
            call(np.zeros(N - 1, np.float32))


def test_a_refused_predict_latches_the_feature_counts_and_a_refused_refit_does_not():
    lib = _lib()
    X, Xc = np.zeros((N, F), np.float32), np.full((N, FC + 1), b"a", dtype="S128")
    for name in ("predict", "predict_encoded", "predict_continue", "predict_continue_encoded", "predict_staged", "staged_loss", "predict_leaves", "leaf_counts"):
        m = _empty()
        c = Calls(lib, m, X, Xc, D, 0)
        assert _latched(lib, m) == (0, 0, 0)
        _refused(lib, getattr(c, name)(f=2, fc=2), E_INVALID, b"Incompatible dataset")       # 2 + 2 != 5: refused, and latched all the same
        assert _latched(lib, m) == (2, 2, 0), name
        _refused(lib, getattr(c, name)(f=1, fc=3, n=0), E_INVALID, b"Incompatible dataset")  # no trees yet: the next call latches again
        assert _latched(lib, m) == (1, 3, 0), name
    m = _empty()
    c = Calls(lib, m, X, Xc, D, 0)
    _refused(lib, c.refit_leaves(f=2, fc=2), E_INVALID, b"refit_leaves: the model has no trees")
    _refused(lib, c.refit_leaves(fc=FC), E_INVALID, b"refit_leaves: the model has no trees")
    assert _latched(lib, m) == (0, 0, 0)
    # a legal batch that fails later in the call is latched as well
    _refused(lib, c.predict(fc=FC, out=None), E_INVALID, b"Cannot call predict without observations!")
    assert _latched(lib, m) == (F, FC, 0)
