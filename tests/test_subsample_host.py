"""CPU-side checks of the row sampler behind fit_prepared(subsample=) and PreparedDataset.sample_rows (include/gbrl_hip.h, "Row subsampling";
gbrl_amd/csrc/sample_core.h).  The host function is the specification the device kernels are compared with (tests/test_gpu_sample_rows.py), so it
is held here to a NumPy restatement of the rule written from its text, to known answers pinned as literals, and to two sanity conditions on the
samples themselves; then everything the new calls refuse without a device."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

E_INVALID = -1
C_SYMBOLS = ("gbrl_hip_sample_rows_host", "gbrl_hip_dataset_sample_rows", "gbrl_hip_fit_prepared_sampled")
U64 = np.uint64


def restate_u(seed, draw, rows):
    """u of the specification for an array of absolute row indices, in wrapping uint64 arithmetic"""
    with np.errstate(over="ignore"):
        x = (U64(draw) << U64(32)) | np.asarray(rows, dtype=np.uint64)
        z = x + U64((int(seed) + 1) % 2**64) * U64(0x9E3779B97F4A7C15)
        z ^= z >> U64(30); z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27); z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        return (z >> U64(40)).astype(np.int64)


def restate_sample(n, subsample, seed=0, draw=0, row0=0):
    rows = np.arange(row0, row0 + n, dtype=np.int64)
    thr = int(np.floor(np.float64(subsample) * 16777216.0))
    return rows[restate_u(seed, draw, rows) < thr].astype(np.int32)


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, d, u64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    lib.gbrl_hip_sample_rows_host.argtypes = [ci, ci, d, u64, ci, vp, vp]
    lib.gbrl_hip_dataset_sample_rows.argtypes = [vp, ci, ci, d, u64, ci, vp, ci, vp]
    lib.gbrl_hip_fit_prepared_sampled.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, d, d, u64, vp, vp, vp, vp]
    return lib


def _c_sample(lib, n, subsample, seed=0, draw=0, row0=0):
    out = np.full(n, -7, np.int32)
    cnt = C.c_int(-1)
    assert lib.gbrl_hip_sample_rows_host(row0, n, subsample, seed, draw, out.ctypes.data, C.byref(cnt)) == 0, lib.gbrl_hip_last_error()
    assert 0 <= cnt.value <= n and (out[cnt.value:] == -7).all(), "wrote past the count"
    return out[:cnt.value].copy()


def _both(lib, n, subsample, seed=0, draw=0, row0=0):
    a = _c_sample(lib, n, subsample, seed, draw, row0)
    b = gbrl_amd.gbrl_cpp.sample_rows_host(n, subsample, seed=seed, draw=draw, row0=row0)
    assert b.dtype == np.int32 and b.ndim == 1 and np.array_equal(a, b)
    return b


# ---- the tables of the specification, as literals -------------------------------------------------------------------------------------------
U_TABLE = [((7, 3, 0), 4807967), ((7, 3, 1), 12581402), ((7, 3, 2), 1351019), ((7, 3, 3), 7380587), ((0, 0, 0), 0xe220a8), ((1, 0, 0), 0x6e789e)]
SAMPLE_TABLE = [
    # n, subsample, seed, draw, count, first kept, last kept (None: only the last three digits are pinned), sum of kept indices
    (1000, 0.5, 7, 3, 500, [0, 2, 3, 6, 10, 13, 14, 18], [988, 996, 998], 241440),
    (1000, 0.5, 7, 4, 513, [0, 2, 3, 4, 5, 8, 13, 14], [995, 996, 998], 255744),
    (64, 0.25, 0, 0, 12, [3, 10, 18, 20, 21, 33, 40, 41], [49, 57, 62], 402),
    (4096, 0.1, 3, 17, 441, [2, 7, 23, 38, 57, 60, 91, 93], [4072, 4076, 4077], 970443),
    (2**20, 0.5, 1, 0, 524378, [0, 6, 7, 11], None, 275082727169),
    (2**20, 0.8, 2**63 + 5, 2**31 - 1, 838900, [0, 1, 2, 3], None, 439793200043),
    (2**20 + 1, 0.5, 7, 3, 524707, [0, 2, 3, 6], [1048572, 1048573, 1048576], 274795070813),
]


def test_the_restatement_gives_the_pinned_u_values():
    for (seed, draw, row), u in U_TABLE:
        assert int(restate_u(seed, draw, [row])[0]) == u, (seed, draw, row)


def test_single_values_of_u_through_the_threshold():
    """u itself is not exported: row r is kept at threshold t iff u < t, so u is pinned from both sides with subsample = u / 2^24 and (u + 1) / 2^24"""
    lib = _lib()
    for (seed, draw, row), u in U_TABLE:
        assert _both(lib, 1, u / 2**24, seed, draw, row).tolist() == [], (seed, draw, row)
        assert _both(lib, 1, (u + 1) / 2**24, seed, draw, row).tolist() == [row], (seed, draw, row)


@pytest.mark.parametrize("n,p,seed,draw,count,first,last,total", SAMPLE_TABLE)
def test_pinned_samples(n, p, seed, draw, count, first, last, total):
    got = _both(_lib(), n, p, seed, draw)
    assert got.size == count
    assert got[:len(first)].tolist() == first
    if last is None:
        assert [int(v) % 1000 for v in got[-3:]] == [573, 574, 575]
    else:
        assert got[-3:].tolist() == last
    assert int(got.astype(np.int64).sum()) == total
    assert (np.diff(got) > 0).all(), "ascending, without replacement"
    assert np.array_equal(got, restate_sample(n, p, seed, draw))


@pytest.mark.parametrize("row0", [0, 5, 1000])
@pytest.mark.parametrize("p", [2.0**-24, 0.1, 0.5, 1 - 2.0**-24, 1.0])
def test_host_sampler_is_the_restatement(row0, p):
    lib = _lib()
    for seed in (0, 1, 2**63 + 5, 2**64 - 1):
        for draw in (0, 1, 2**31 - 1):
            for n in (1, 64, 777):
                want = restate_sample(n, p, seed, draw, row0)
                assert np.array_equal(_both(lib, n, p, seed, draw, row0), want), (n, p, seed, draw, row0)
                if p == 1.0:
                    assert want.tolist() == list(range(row0, row0 + n))
    # a range is the concatenation of its parts: the rule looks at absolute indices only
    whole = _both(lib, 777, p, 3, 2, row0)
    parts = [_both(lib, 300, p, 3, 2, row0), _both(lib, 477, p, 3, 2, row0 + 300)]
    assert np.array_equal(whole, np.concatenate(parts))


def test_sample_sizes_stay_within_four_standard_deviations():
    """n = 4096 at 0.5: sigma = sqrt(4096 / 4) = 32, so 4 sigma = 128 rows (the rule's own maximum over these 200 draws is 3.03 sigma)"""
    counts = np.array([gbrl_amd.gbrl_cpp.sample_rows_host(4096, 0.5, seed=11, draw=d).size for d in range(200)])
    dev = np.abs(counts - 2048)
    print("largest deviation %d rows = %.2f sigma" % (dev.max(), dev.max() / 32.0))
    assert dev.max() <= 128


def test_two_draws_are_independent_samples():
    n = 2**20
    a = gbrl_amd.gbrl_cpp.sample_rows_host(n, 0.5, seed=1, draw=0)
    b = gbrl_amd.gbrl_cpp.sample_rows_host(n, 0.5, seed=1, draw=1)
    shared = np.intersect1d(a, b, assume_unique=True).size / n
    print("rows in both samples: %.4f of all" % shared)
    assert abs(shared - 0.25) <= 0.005


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_docstrings():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    for sym in C_SYMBOLS:
        assert hasattr(lib, sym), sym
    assert hasattr(gbrl_amd.gbrl_cpp, "sample_rows_host") and hasattr(gbrl_amd.PreparedDataset, "sample_rows")
    for doc in (gbrl_amd.GBRL.fit_prepared.__doc__, gbrl_amd.PreparedDataset.sample_rows.__doc__, gbrl_amd.gbrl_cpp.sample_rows_host.__doc__):
        assert "subsample" in doc and "seed" in doc
    doc = gbrl_amd.GBRL.fit_prepared.__doc__
    sig = doc.splitlines()[0]   # the first overload keeps its generated line
    assert sig.startswith("fit_prepared(self: gbrl_cpp.GBRL, ds: object, targets: object, iterations: ") and sig.endswith("-> float")
    assert "subsample=1.0, seed=0" in doc and "tree count before the step" in doc and "keeps no row" in doc and "subsample == 1.0" in doc


BAD_FRACTIONS = (0.0, -0.5, 1.5, float("nan"), 2.0**-25, float("inf"))


def test_the_sample_calls_refuse_bad_arguments():
    lib = _lib()
    err = lib.gbrl_hip_last_error
    out = np.full(16, -7, np.int32)
    cnt = C.c_int(-1)
    o, c = out.ctypes.data, C.byref(cnt)
    stale = C.create_string_buffer(64)
    for p in BAD_FRACTIONS:
        assert lib.gbrl_hip_sample_rows_host(0, 16, p, 0, 0, o, c) == E_INVALID and b"subsample" in err()
        with pytest.raises(RuntimeError, match="subsample"):
            gbrl_amd.gbrl_cpp.sample_rows_host(16, p)
    for row0, n, draw, what in ((-1, 16, 0, b"row0"), (0, 0, 0, b"n must be positive"), (0, -3, 0, b"n must be positive"), (0, 16, -1, b"draw"),
                                (2**31 - 8, 16, 0, b"2^31")):
        assert lib.gbrl_hip_sample_rows_host(row0, n, 0.5, 0, draw, o, c) == E_INVALID and what in err(), (row0, n, draw)
        # the data set call checks its handle first: a null or stale one is an argument error, never a read through it
        assert lib.gbrl_hip_dataset_sample_rows(None, row0, n, 0.5, 0, draw, o, 0, c) == E_INVALID and b"null data set" in err()
        assert lib.gbrl_hip_dataset_sample_rows(C.addressof(stale), row0, n, 0.5, 0, draw, o, 0, c) == E_INVALID and b"destroyed" in err()
    assert lib.gbrl_hip_sample_rows_host(0, 16, 0.5, 0, 0, None, c) == E_INVALID and b"null output" in err()
    assert lib.gbrl_hip_sample_rows_host(0, 16, 0.5, 0, 0, o, None) == E_INVALID and b"null output" in err()
    assert (out == -7).all() and cnt.value == -1
    with pytest.raises(RuntimeError, match="n must be positive"):
        gbrl_amd.gbrl_cpp.sample_rows_host(0, 0.5)
    with pytest.raises(RuntimeError, match="draw"):
        gbrl_amd.gbrl_cpp.sample_rows_host(4, 0.5, draw=-1)
    with pytest.raises(TypeError):
        gbrl_amd.gbrl_cpp.sample_rows_host(4, 0.5, seed=-1)
    with pytest.raises(TypeError):
        gbrl_amd.gbrl_cpp.sample_rows_host(4, 0.5, seed=2**64)
    # the last row a call may name is 2^31 - 1
    assert _c_sample(lib, 8, 1.0, 0, 0, 2**31 - 8).tolist() == list(range(2**31 - 8, 2**31))


def _empty(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    base.update(kw)
    m = gbrl_amd.GBRL(**base)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=base["output_dim"])
    return m


def test_fit_prepared_refuses_a_bad_subsample_before_a_device_is_needed(tmp_path):
    m = _empty()
    y = np.zeros((16, 2), np.float32)
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    before = p.read_bytes()
    lib = _lib()
    err = lib.gbrl_hip_last_error
    loss = C.c_float(-1.0)
    for bad in BAD_FRACTIONS:
        with pytest.raises(RuntimeError, match="subsample must be in"):
            m.fit_prepared(None, y, 3, subsample=bad)
        with pytest.raises(RuntimeError, match="subsample must be in"):
            m.fit_prepared(None, y, 3, valid=None, subsample=bad, seed=3)
        rc = lib.gbrl_hip_fit_prepared_sampled(m._handle(), None, y.ctypes.data, 0, 3, None, None, 0, 0, 0.0, bad, 0, C.byref(loss), None, None, None)
        assert rc == E_INVALID and b"subsample must be in" in err()
    # what fit_prepared refuses today comes first, and a good fraction then reaches the data set check
    with pytest.raises(RuntimeError, match="iterations must be >= 0"):
        m.fit_prepared(None, y, -1, subsample=0.0)
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, y, 3, subsample=0.5, seed=2**64 - 1)
    with pytest.raises(RuntimeError, match="null data set"):
        m.fit_prepared(None, y, 3, subsample=1.0, seed=9)
    with pytest.raises(TypeError):
        m.fit_prepared(None, y, 3, subsample=0.5, seed=-1)
    # without a validation set the validation arguments must be NULL / 0
    rc = lib.gbrl_hip_fit_prepared_sampled(m._handle(), None, y.ctypes.data, 0, 3, None, y.ctypes.data, 0, 0, 0.0, 0.5, 0, C.byref(loss), None, None, None)
    assert rc == E_INVALID and b"need a validation set" in err()
    rc = lib.gbrl_hip_fit_prepared_sampled(m._handle(), None, y.ctypes.data, 0, 3, None, None, 0, 2, 0.0, 0.5, 0, C.byref(loss), None, None, None)
    assert rc == E_INVALID and b"need a validation set" in err()
    rc = lib.gbrl_hip_fit_prepared_sampled(None, None, y.ctypes.data, 0, 3, None, None, 0, 0, 0.0, 0.5, 0, C.byref(loss), None, None, None)
    assert rc == E_INVALID and b"null model" in err()
    assert loss.value == -1.0
    assert m.save(str(p)) == 0 and p.read_bytes() == before
