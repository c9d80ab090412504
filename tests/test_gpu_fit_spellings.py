"""The five C spellings of fit_prepared and the Python call, on the GPU (include/gbrl_hip.h: gbrl_hip_fit_prepared, _valid, _sampled, _colsampled,
_objective; GBRL.fit_prepared).  The binding reaches the device through one of them only, so the others are run here through ctypes on the
handles of the model and the data sets.  Every comparison is exact (bytes):
  * without a validation set, with one and early_stopping_rounds = 2, and with subsample / colsample / seed: every spelling that can express
    the call leaves the same model file, the same float32 loss, the same validation curve, iterations_done and best_n_trees;
  * which outputs a spelling writes without a validation set (iterations_done = iterations, best_n_trees left alone);
  * gbrl_hip_fit_prepared_valid with a NULL validation set is "null data set", not "no validation".
n = 200 at batch_size 64 is four batches with a last one of 8 rows, and 9 iterations wrap the cursor twice; the 70 validation rows are no
multiple of the 64-row loss partial."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

E_INVALID = -1
N, NV, F, D, BS, DEPTH, T = 200, 70, 5, 3, 64, 3, 9
OBJ_RMSE = 0
SENTINEL = -7
POLICIES = [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform")]


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, d, u64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    head = [vp, vp, vp, ci, ci]                 # model, ds, targets, targets_on_device, iterations
    valid = [vp, vp, ci, ci, d]                 # valid_ds, valid_targets, valid_targets_on_device, early_stopping_rounds, min_delta
    outs = [vp, vp, vp, vp]                     # loss_out, valid_loss_out, iterations_done, best_n_trees
    lib.gbrl_hip_fit_prepared.argtypes = head + [vp]
    lib.gbrl_hip_fit_prepared_valid.argtypes = head + valid + outs
    lib.gbrl_hip_fit_prepared_sampled.argtypes = head + valid + [d, u64] + outs
    lib.gbrl_hip_fit_prepared_colsampled.argtypes = head + valid + [d, d, u64] + outs
    lib.gbrl_hip_fit_prepared_objective.argtypes = head + valid + [d, d, u64, ci] + outs
    return lib


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


class _Fixture:
    def __init__(self, policy, score, gen):
        rng = np.random.default_rng(9100 + len(policy))
        W = rng.standard_normal((F, D)).astype(np.float32)
        def draw(rows):
            X = rng.standard_normal((rows, F)).astype(np.float32)
            return X, np.ascontiguousarray((np.tanh(X @ W) + 0.3 * rng.standard_normal((rows, D))).astype(np.float32))
        self.X, self.Y = draw(N)
        self.Xv, self.Yv = draw(NV)
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=32, split_score_func=score, generator_type=gen,
                          grow_policy=policy, device="cpu", batch_size=BS)
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        self.base = m
        self.ds = m.prepare_dataset(self.X)
        self.dsv = m.prepare_dataset(self.Xv, reference=self.ds)
        self.lib = _lib()

    def run_c(self, spelling, tmp_path, valid, rounds=0, subsample=1.0, colsample=1.0, seed=0, null_valid_ds=False):
        """one C spelling on a fresh clone: (status, file bytes, loss bits, curve bytes over [0, done], iterations_done, best_n_trees)"""
        m = gbrl_amd.GBRL(self.base)
        loss, done, best = C.c_float(np.nan), C.c_int(SENTINEL), C.c_int(SENTINEL)
        curve = np.full(T + 1, -1.0, np.float64)
        head = [m._handle(), self.ds._handle(), self.Y.ctypes.data, 0, T]
        v = [None if null_valid_ds else self.dsv._handle(), self.Yv.ctypes.data, 0, rounds, 0.0] if valid else [None, None, 0, 0, 0.0]
        outs = [C.byref(loss), curve.ctypes.data if valid else None, C.byref(done), C.byref(best)]
        if spelling == "plain":
            assert not valid and subsample == 1.0 and colsample == 1.0
            rc = self.lib.gbrl_hip_fit_prepared(*head, C.byref(loss))
        elif spelling == "valid":
            assert subsample == 1.0 and colsample == 1.0
            rc = self.lib.gbrl_hip_fit_prepared_valid(*head, *v, *outs)
        elif spelling == "sampled":
            assert colsample == 1.0
            rc = self.lib.gbrl_hip_fit_prepared_sampled(*head, *v, subsample, seed, *outs)
        elif spelling == "colsampled":
            rc = self.lib.gbrl_hip_fit_prepared_colsampled(*head, *v, subsample, colsample, seed, *outs)
        else:
            rc = self.lib.gbrl_hip_fit_prepared_objective(*head, *v, subsample, colsample, seed, OBJ_RMSE, *outs)
        k = done.value + 1 if valid and rc == 0 else T + 1
        return rc, _file(m, tmp_path), np.float32(loss.value).tobytes(), curve[:k].tobytes(), done.value, best.value

    def run_py(self, tmp_path, valid, **kw):
        m = gbrl_amd.GBRL(self.base)
        if not valid:
            loss = m.fit_prepared(self.ds, self.Y, T, **kw)
            assert isinstance(loss, float)
            return 0, _file(m, tmp_path), np.float32(loss).tobytes(), None, None, None
        r = m.fit_prepared(self.ds, self.Y, T, valid=self.dsv, valid_targets=self.Yv, **kw)
        return 0, _file(m, tmp_path), np.float32(r["loss"]).tobytes(), np.asarray(r["valid_loss"], np.float64).tobytes(), r["iterations"], r["best_n_trees"]


@pytest.fixture(scope="module", params=POLICIES, ids=[p[0] for p in POLICIES])
def fx(request):
    return _Fixture(*request.param)


def test_the_spellings_agree_without_a_validation_set(fx, tmp_path):
    want = fx.run_c("plain", tmp_path, valid=False)
    assert want[0] == 0 and want[4:] == (SENTINEL, SENTINEL)
    for spelling in ("sampled", "colsampled", "objective"):
        got = fx.run_c(spelling, tmp_path, valid=False)
        assert got[0] == 0, fx.lib.gbrl_hip_last_error()
        assert got[1] == want[1], "%s: the model file differs from gbrl_hip_fit_prepared's" % spelling
        assert got[2] == want[2], "%s: the loss differs" % spelling
        assert got[4] == T, "%s: iterations_done is written without a validation set" % spelling
        assert got[5] == SENTINEL, "%s: best_n_trees is left alone without a validation set" % spelling
    py = fx.run_py(tmp_path, valid=False)
    assert py[1] == want[1] and py[2] == want[2], "GBRL.fit_prepared(ds, y, T) differs from gbrl_hip_fit_prepared"


def test_the_spellings_agree_with_a_validation_set_and_a_stopping_rule(fx, tmp_path):
    want = fx.run_c("valid", tmp_path, valid=True, rounds=2)
    assert want[0] == 0, fx.lib.gbrl_hip_last_error()
    assert 1 <= want[4] <= T and 0 <= want[5] <= want[4], want[4:]
    for spelling in ("sampled", "colsampled", "objective"):
        got = fx.run_c(spelling, tmp_path, valid=True, rounds=2)
        assert got == want, "%s differs from gbrl_hip_fit_prepared_valid in field %d" % (spelling, [a == b for a, b in zip(got, want)].index(False))
    py = fx.run_py(tmp_path, valid=True, early_stopping_rounds=2)
    assert py == want, "GBRL.fit_prepared(valid=) differs in field %d" % [a == b for a, b in zip(py, want)].index(False)


def test_the_spellings_agree_on_row_and_column_samples(fx, tmp_path):
    kw = dict(subsample=0.5, colsample=0.6, seed=7)
    want = fx.run_c("colsampled", tmp_path, valid=True, rounds=2, **kw)
    assert want[0] == 0, fx.lib.gbrl_hip_last_error()
    got = fx.run_c("objective", tmp_path, valid=True, rounds=2, **kw)
    assert got == want, "objective differs from colsampled in field %d" % [a == b for a, b in zip(got, want)].index(False)
    py = fx.run_py(tmp_path, valid=True, early_stopping_rounds=2, **kw)
    assert py == want, "GBRL.fit_prepared differs in field %d" % [a == b for a, b in zip(py, want)].index(False)
    plain = fx.run_c("valid", tmp_path, valid=True, rounds=2)
    assert plain[1] != want[1], "the samples changed nothing: the case does not test them"
    rows = fx.run_c("sampled", tmp_path, valid=True, rounds=2, subsample=0.5, seed=7)
    assert rows == fx.run_c("colsampled", tmp_path, valid=True, rounds=2, subsample=0.5, colsample=1.0, seed=7)
    assert rows[0] == 0 and rows[1] not in (want[1], plain[1])


def test_valid_spelling_with_a_null_validation_set_is_refused(fx, tmp_path):
    untouched = _file(gbrl_amd.GBRL(fx.base), tmp_path)
    rc, after, loss, curve, done, best = fx.run_c("valid", tmp_path, valid=True, rounds=2, null_valid_ds=True)
    assert rc == E_INVALID and b"null data set" in fx.lib.gbrl_hip_last_error()
    assert after == untouched, "a refused call changed the model"
    assert np.isnan(np.frombuffer(loss, np.float32)[0]) and (done, best) == (SENTINEL, SENTINEL)
    assert curve == np.full(T + 1, -1.0, np.float64).tobytes(), "a refused call wrote to valid_loss_out"
