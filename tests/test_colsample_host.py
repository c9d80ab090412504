"""CPU-side checks of the column rule behind fit_prepared(colsample=), PreparedDataset.sample_cols and gbrl_cpp.sample_cols_host (include/gbrl_hip.h,
"Column subsampling"; gbrl_amd/csrc/sample_core.h).  The rule is a definition and runs on the host only, so it is held here to a NumPy
restatement written from the header's text; then what the new calls refuse without a device, and the gather kernel's geometry."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

E_INVALID = -1
C_SYMBOLS = ("gbrl_hip_sample_cols_host", "gbrl_hip_step_prepared_cols", "gbrl_hip_dataset_codes_cols", "gbrl_hip_fit_prepared_colsampled",
             "gbrl_hip_gather_cols_geometry")
U64 = np.uint64
STREAM = 0x636F6C73616D706C


def restate_u(seed, draw, idx):
    """the 24-bit hash of the row sampler (its specification), in wrapping uint64 arithmetic"""
    with np.errstate(over="ignore"):
        x = (U64(draw) << U64(32)) | np.asarray(idx, dtype=np.uint64)
        z = x + U64((int(seed) + 1) % 2**64) * U64(0x9E3779B97F4A7C15)
        z ^= z >> U64(30); z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27); z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        return (z >> U64(40)).astype(np.int64)


def restate_cols(F, colsample, seed=0, draw=0):
    k = max(1, int(np.floor(np.float64(colsample) * F + 0.5)))
    f = np.arange(F, dtype=np.int64)
    u = restate_u(int(seed) ^ STREAM, draw, f)
    order = np.lexsort((f, u))   # by u, ties by f
    return np.sort(f[order[:k]]).astype(np.int32)


def restate_rows(n, subsample, seed=0, draw=0):
    rows = np.arange(n, dtype=np.int64)
    return rows[restate_u(seed, draw, rows) < int(np.floor(np.float64(subsample) * 16777216.0))].astype(np.int32)


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, d, u64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    lib.gbrl_hip_sample_cols_host.argtypes = [ci, d, u64, ci, vp, vp]
    lib.gbrl_hip_gather_cols_geometry.argtypes = [vp, vp]
    lib.gbrl_hip_gather_cols_geometry.restype = None
    lib.gbrl_hip_fit_prepared_colsampled.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, d, d, d, u64, vp, vp, vp, vp]
    lib.gbrl_hip_step_prepared_cols.argtypes = [vp, vp, vp, ci, vp, ci, ci, vp, ci]
    lib.gbrl_hip_dataset_codes_cols.argtypes = [vp, vp, ci, ci, vp, ci, vp]
    return lib


def _both(lib, F, colsample, seed=0, draw=0):
    out = np.full(F, -7, np.int32)
    cnt = C.c_int(-1)
    assert lib.gbrl_hip_sample_cols_host(F, colsample, seed, draw, out.ctypes.data, C.byref(cnt)) == 0, lib.gbrl_hip_last_error()
    assert 1 <= cnt.value <= F and (out[cnt.value:] == -7).all(), "wrote past the count"
    b = gbrl_amd.gbrl_cpp.sample_cols_host(F, colsample, seed=seed, draw=draw)
    assert b.dtype == np.int32 and b.ndim == 1 and np.array_equal(out[:cnt.value], b)
    return b


@pytest.mark.parametrize("F", [1, 2, 16, 17, 128, 1000])
def test_the_column_rule_is_the_restatement(F):
    lib = _lib()
    for p in (1.0 / F, 0.3, 0.5, 0.999, 1.0):
        k = max(1, int(np.floor(np.float64(p) * F + 0.5)))
        for seed in (0, 1, 2**63 + 5, 2**64 - 1):
            for draw in (0, 1, 2**31 - 1):
                got = _both(lib, F, p, seed, draw)
                assert got.size == k, (F, p, seed, draw)
                assert (np.diff(got) > 0).all() and got[0] >= 0 and got[-1] < F, "ascending, distinct, in range"
                assert np.array_equal(got, restate_cols(F, p, seed, draw)), (F, p, seed, draw)
                if p == 1.0:
                    assert got.tolist() == list(range(F))


def test_draws_seeds_and_the_row_stream_differ():
    F = 128
    a = gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5, seed=3, draw=0)
    assert not np.array_equal(a, gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5, seed=3, draw=1))
    assert not np.array_equal(a, gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5, seed=4, draw=0))
    assert np.array_equal(a, gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5, seed=3, draw=0))
    # a stream of its own: not the k rows of [0, F) with the smallest hash of the row sampler, nor its kept set at the same (seed, draw)
    for seed, draw in ((3, 0), (0, 0), (7, 5)):
        cols = gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5, seed=seed, draw=draw)
        rows = gbrl_amd.gbrl_cpp.sample_rows_host(F, 0.5, seed=seed, draw=draw)
        assert np.array_equal(rows, restate_rows(F, 0.5, seed, draw))
        assert not np.array_equal(cols, rows)
        u_rows = restate_u(seed, draw, np.arange(F))
        assert not np.array_equal(cols, np.sort(np.lexsort((np.arange(F), u_rows))[:cols.size]))


def test_symbols_docstrings_and_geometry():
    lib = _lib()
    for sym in C_SYMBOLS:
        assert hasattr(lib, sym), sym
    assert hasattr(gbrl_amd.gbrl_cpp, "sample_cols_host") and hasattr(gbrl_amd.PreparedDataset, "sample_cols")
    assert "colsample=1.0" in gbrl_amd.GBRL.fit_prepared.__doc__ and "cols=None" in gbrl_amd.GBRL.step_prepared.__doc__
    assert "cols: object = None" in gbrl_amd.PreparedDataset.codes.__doc__.splitlines()[0]
    rows, groups = C.c_int(-1), C.c_int(-1)
    lib.gbrl_hip_gather_cols_geometry(C.byref(rows), C.byref(groups))
    assert rows.value > 0 and groups.value > 0
    lib.gbrl_hip_gather_cols_geometry(None, None)   # either may be NULL


BAD_FRACTIONS = (0.0, -0.5, 1.5, float("nan"), float("inf"), -0.0)


def test_the_column_rule_refuses_bad_arguments():
    lib = _lib()
    err = lib.gbrl_hip_last_error
    out = np.full(16, -7, np.int32)
    cnt = C.c_int(-1)
    o, c = out.ctypes.data, C.byref(cnt)
    for p in BAD_FRACTIONS:
        assert lib.gbrl_hip_sample_cols_host(16, p, 0, 0, o, c) == E_INVALID and b"colsample" in err()
        with pytest.raises(RuntimeError, match="colsample"):
            gbrl_amd.gbrl_cpp.sample_cols_host(16, p)
    for F in (0, -3):
        assert lib.gbrl_hip_sample_cols_host(F, 0.5, 0, 0, o, c) == E_INVALID and b"F must be positive" in err()
        with pytest.raises(RuntimeError, match="F must be positive"):
            gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5)
    assert lib.gbrl_hip_sample_cols_host(16, 0.5, 0, -1, o, c) == E_INVALID and b"draw" in err()
    with pytest.raises(RuntimeError, match="draw"):
        gbrl_amd.gbrl_cpp.sample_cols_host(16, 0.5, draw=-1)
    assert lib.gbrl_hip_sample_cols_host(16, 0.5, 0, 0, None, c) == E_INVALID and b"null output" in err()
    assert lib.gbrl_hip_sample_cols_host(16, 0.5, 0, 0, o, None) == E_INVALID and b"null output" in err()
    assert (out == -7).all() and cnt.value == -1
    with pytest.raises(TypeError):
        gbrl_amd.gbrl_cpp.sample_cols_host(4, 0.5, seed=-1)
    # a tiny positive fraction is legal: one column
    assert gbrl_amd.gbrl_cpp.sample_cols_host(16, 1e-300).size == 1


def _empty(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def test_the_model_calls_refuse_before_a_device_is_needed(tmp_path):
    m = _empty()
    y = np.zeros((16, 2), np.float32)
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    before = p.read_bytes()
    lib = _lib()
    err = lib.gbrl_hip_last_error
    loss = C.c_float(-1.0)
    for bad in BAD_FRACTIONS:
        with pytest.raises(RuntimeError, match="colsample must be in"):
            m.fit_prepared(None, y, 3, colsample=bad)
        with pytest.raises(RuntimeError, match="colsample must be in"):
            m.fit_prepared(None, y, 3, valid=None, subsample=0.5, colsample=bad, seed=3)
        rc = lib.gbrl_hip_fit_prepared_colsampled(m._handle(), None, y.ctypes.data, 0, 3, None, None, 0, 0, 0.0, 1.0, bad, 0, C.byref(loss), None, None, None)
        assert rc == E_INVALID and b"colsample must be in" in err()
    # what fit_prepared refuses today comes first, and a good fraction then reaches the data set check
    with pytest.raises(RuntimeError, match="iterations must be >= 0"):
        m.fit_prepared(None, y, -1, colsample=0.0)
    with pytest.raises(RuntimeError, match="subsample must be in"):
        m.fit_prepared(None, y, 3, subsample=0.0, colsample=0.0)
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, y, 3, colsample=0.5, seed=2**64 - 1)
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, y, 3, colsample=1.0, seed=9)
    cols = np.array([0, 2], np.int32)
    g = np.zeros((16, 2), np.float32)
    with pytest.raises(RuntimeError, match="null data set"):
        m.step_prepared(None, g, cols=cols)
    assert lib.gbrl_hip_step_prepared_cols(m._handle(), None, g.ctypes.data, 0, None, 0, 16, None, 2) == E_INVALID and b"null cols" in err()
    assert lib.gbrl_hip_step_prepared_cols(None, None, g.ctypes.data, 0, None, 0, 16, cols.ctypes.data, 2) == E_INVALID and b"null model" in err()
    out = np.zeros(16 * 16, np.uint16)
    assert lib.gbrl_hip_dataset_codes_cols(None, None, 0, 16, cols.ctypes.data, 2, out.ctypes.data) == E_INVALID and b"null data set" in err()
    with pytest.raises(RuntimeError, match="vector of integers"):
        m.step_prepared(None, g, cols=np.array([0.0, 1.0]))
    with pytest.raises(RuntimeError, match="one-dimensional"):
        m.step_prepared(None, g, cols=np.zeros((2, 2), np.int32))
    assert loss.value == -1.0
    assert m.save(str(p)) == 0 and p.read_bytes() == before
