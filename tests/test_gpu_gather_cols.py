"""The column gather of a prepared data set on the GPU (gbrl_amd/csrc/gather_cols.hip through PreparedDataset.codes(rows, cols); include/gbrl_hip.h,
"Column subsampling").  Every comparison is exact: codes(rows, cols) against NumPy indexing of codes(), padding slots zero, at the row counts
around a block's tile, with every kind of rows vector, and at a width whose touched groups the kernel walks in more than one chunk.  There is no case for a second,
general kernel: the chunked walk takes every width a data set can hold, so no such kernel exists."""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu


def _geometry():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    rows, groups = C.c_int(-1), C.c_int(-1)
    lib.gbrl_hip_gather_cols_geometry(C.byref(rows), C.byref(groups))
    assert rows.value > 0 and groups.value > 0
    return rows.value, groups.value


ROWS_PER_TILE, MAX_STAGED = _geometry()
ROW_COUNTS = sorted({1, 63, 64, 65, ROWS_PER_TILE + 1})
_CACHE = {}


def _dataset(F, n):
    """one data set per shape with its full codes, shared by the tests and never changed"""
    if (F, n) not in _CACHE:
        m = gbrl_amd.GBRL(input_dim=F, output_dim=1, policy_dim=1, max_depth=2, n_bins=12, split_score_func="L2", generator_type="Uniform",
                          grow_policy="oblivious", device="cpu")
        X = np.random.default_rng(1000 * F + n).standard_normal((n, F)).astype(np.float32)
        ds = m.prepare_dataset(X)
        full = ds.codes()
        assert full.shape == ((F + 15) // 16, n, 16)
        if n > 1:
            assert full.max() > 0, "the premise: the codes are not all zero"
        _CACHE[(F, n)] = (ds, full)
    return _CACHE[(F, n)]


def _want(full, rows, cols):
    cols = np.asarray(cols)
    n = full.shape[1]
    r = np.arange(n) if rows is None else np.asarray(rows)
    out = np.zeros(((cols.size + 15) // 16, r.size, 16), np.uint16)   # padding slots zero
    for s, c in enumerate(cols):
        out[s // 16, :, s % 16] = full[c // 16, r, c % 16]
    return out


def _col_sets(F):
    rng = np.random.default_rng(F)
    sets = {"one column": [F // 2], "the last column": [F - 1], "one column from each group": [min(F - 1, 16 * g + (5 * g + 3) % 16) for g in range((F + 15) // 16)],
            "every column": list(range(F))}
    if F >= 16:
        sets["exactly 16 columns"] = sorted(rng.choice(F, 16, replace=False).tolist())
    if F >= 17:
        sets["17 columns"] = sorted(rng.choice(F, 17, replace=False).tolist())
    return sets


def _row_sets(n):
    rng = np.random.default_rng(n)
    return {"every row": None, "descending": np.arange(n - 1, -1, -1, dtype=np.int32), "with duplicates": rng.integers(0, n, n + 3).astype(np.int32),
            "a short list": rng.integers(0, n, max(1, n // 2)).astype(np.int32)}


def _dev(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("F", [1, 16, 17, 40])
def test_codes_of_a_column_subset_are_numpy_indexing_of_the_codes(F, n):
    import torch
    ds, full = _dataset(F, n)
    for cname, cols in _col_sets(F).items():
        c32 = np.asarray(cols, np.int32)
        for rname, rows in _row_sets(n).items():
            want = _want(full, rows, cols)
            got = ds.codes(rows=rows, cols=c32)
            assert got.dtype == np.uint16 and got.shape == want.shape, (cname, rname)
            assert got.tobytes() == want.tobytes(), (cname, rname)
            if rows is not None:
                got = ds.codes(rows=_dev(torch.from_numpy(rows).cuda()), cols=cols)   # a device rows vector; cols as a plain list
                assert got.tobytes() == want.tobytes(), (cname, rname, "device rows")
    # every column is the call without cols
    assert ds.codes(cols=np.arange(F)).tobytes() == full.tobytes()


def test_a_subset_wider_than_the_staged_groups_is_walked_in_chunks():
    """F = 16 * (max_staged_groups + 1) with every source group touched: the staged groups do not fit one tile, the kernel walks them in chunks"""
    F, n = 16 * (MAX_STAGED + 1), 70
    ds, full = _dataset(F, n)
    rng = np.random.default_rng(7)
    sets = {"one column from each group": [16 * g + (7 * g + 1) % 16 for g in range(MAX_STAGED + 1)],
            "every odd column": list(range(1, F, 2)),
            "all but one": [c for c in range(F) if c != 100],
            "3 of every 4, at random": sorted(rng.choice(F, 3 * F // 4, replace=False).tolist())}
    rows = rng.integers(0, n, 131).astype(np.int32)
    for cname, cols in sets.items():
        assert len({c // 16 for c in cols}) == MAX_STAGED + 1, "the premise: every source group is touched"
        assert ds.codes(cols=cols).tobytes() == _want(full, None, cols).tobytes(), cname
        assert ds.codes(rows=rows, cols=cols).tobytes() == _want(full, rows, cols).tobytes(), (cname, "rows")


def test_sample_cols_of_the_data_set_feeds_codes():
    F, n = 40, 65
    ds, full = _dataset(F, n)
    cols = ds.sample_cols(0.5, seed=9, draw=2)
    assert np.array_equal(cols, gbrl_amd.gbrl_cpp.sample_cols_host(F, 0.5, seed=9, draw=2)) and cols.size == 20
    assert ds.codes(cols=cols).tobytes() == _want(full, None, cols).tobytes()


def test_bad_column_vectors_are_refused():
    F, n = 40, 65
    ds, full = _dataset(F, n)
    for cols, what in (([3, 2], "strictly ascending"), ([2, 2], "strictly ascending"), ([0, 40], "outside"), ([-1, 3], "outside"), ([], "between 1 and"),
                       (list(range(F)) + [F], "between 1 and")):
        with pytest.raises(RuntimeError, match=what):
            ds.codes(cols=np.asarray(cols, np.int32))
        with pytest.raises(RuntimeError, match=what):
            ds.codes(rows=np.array([0, 1], np.int32), cols=np.asarray(cols, np.int32))
    with pytest.raises(RuntimeError, match="outside"):
        ds.codes(rows=np.array([0, n], np.int32), cols=[1, 2])
    assert ds.codes().tobytes() == full.tobytes()
