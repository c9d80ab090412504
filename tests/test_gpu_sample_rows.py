"""The row sampler on the GPU (PreparedDataset.sample_rows, gbrl_hip_dataset_sample_rows, gbrl_hip_sample_gather; include/gbrl_hip.h, "Row
subsampling").  Every comparison is exact:
  * the device sample against gbrl_cpp.sample_rows_host (which tests/test_subsample_host.py holds to the specification) at the sizes where the
    kernels take another path -- a wave, the rows of one block, one slice of the scan of the block counts, each - 1, exact and + 1 -- on
    sub-ranges that begin and end inside a wave, over the fractions, seeds and draws of the host test;
  * the gathered gradient rows of the fused pass, bit for bit, through the 16-byte and the 4-byte accesses, with aligned matrices and with
    matrices offset by 4 bytes; nothing is written behind row m;
  * two calls give the same bytes.
"""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

FRACTIONS = (2.0**-24, 0.1, 0.5, 1 - 2.0**-24, 1.0)
SEEDS = (0, 1, 2**63 + 5, 2**64 - 1)
DRAWS = (0, 1, 2**31 - 1)


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, d, u64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    lib.gbrl_hip_dataset_sample_rows.argtypes = [vp, ci, ci, d, u64, ci, vp, ci, vp]
    lib.gbrl_hip_sample_gather.argtypes = [ci, ci, d, u64, ci, vp, ci, vp, vp, vp]
    lib.gbrl_hip_sample_rows_geometry.argtypes = [vp, vp]
    lib.gbrl_hip_sample_rows_geometry.restype = None
    return lib


def _geometry():
    rpb, width = C.c_int(0), C.c_int(0)
    _lib().gbrl_hip_sample_rows_geometry(C.byref(rpb), C.byref(width))
    assert rpb.value >= 64 and width.value >= 64
    return rpb.value, width.value


def _dataset(n, F=3):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=1, policy_dim=1, max_depth=2, n_bins=8, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cpu")
    X = np.random.default_rng(n).standard_normal((n, F)).astype(np.float32)
    return m.prepare_dataset(X)


_BIG = {}


def _big_dataset(n):
    """one data set for the cases near 2^20 rows (the largest asked for so far is kept)"""
    if _BIG.get("n", 0) < n:
        _BIG["ds"], _BIG["n"] = _dataset(n), n
    return _BIG["ds"]


def _device_sample(ds, p, seed, draw, start=0, stop=None):
    import torch
    t = torch.from_dlpack(ds.sample_rows(p, seed=seed, draw=draw, start=start, stop=stop))
    assert t.dtype == torch.int32 and t.dim() == 1 and t.is_cuda
    return t


def _check(ds, n_rows, p, seed, draw, start=0, stop=None):
    n = (n_rows if stop is None else stop) - start
    want = gbrl_amd.gbrl_cpp.sample_rows_host(n, p, seed=seed, draw=draw, row0=start)
    got = _device_sample(ds, p, seed, draw, start, stop).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), \
        "n %d start %d p %r seed %d draw %d: %d rows against %d, first difference at %s" % (
            n, start, p, seed, draw, got.size, want.size, np.argwhere(got[:min(got.size, want.size)] != want[:min(got.size, want.size)])[:1].tolist())
    return want


def _grid(k):
    """the (fraction, seed, draw) grid, every k-th point of it (k = 1: all 60)"""
    pts = [(p, s, d) for p in FRACTIONS for s in SEEDS for d in DRAWS]
    return pts[::k]


def test_small_ranges_around_a_wave_and_a_sweep():
    for n in (1, 63, 64, 65, 255, 256, 257):
        ds = _dataset(n)
        for p, seed, draw in _grid(1):
            _check(ds, n, p, seed, draw)


def test_ranges_around_the_rows_of_one_block():
    rpb, _ = _geometry()
    for n in (rpb - 1, rpb, rpb + 1, 3 * rpb + 5):
        ds = _dataset(n)
        for p, seed, draw in _grid(4):
            _check(ds, n, p, seed, draw)
        # sub-ranges: start > 0, begin and end inside a wave, one row, across a block edge of the RANGE (blocks count from start)
        for start, stop in ((1, n), (37, n - 3), (70, 71), (5, 6), (n - 1, n), (rpb // 2 + 9, n), (0, 65), (63, 130)):
            if 0 <= start < stop <= n:
                for p, seed, draw in ((0.5, 7, 3), (0.1, 2**64 - 1, 2**31 - 1), (1.0, 0, 0)):
                    _check(ds, n, p, seed, draw, start, stop)


def test_ranges_around_one_slice_of_the_scan():
    rpb, width = _geometry()
    sizes = sorted({2**20 + 1} | ({width * rpb - 1, width * rpb + 1} if width * rpb <= 2**21 else set()))
    ds = _big_dataset(max(sizes))
    for n in sizes:
        for p, seed, draw in ((0.5, 1, 0), (0.1, 2**63 + 5, 2**31 - 1), (1.0, 3, 1)):
            got = _check(ds, max(sizes), p, seed, draw, 0, n)
            if p == 1.0:
                assert got.size == n
    if 2**20 + 1 in sizes:   # a known answer of the specification
        got = _check(ds, max(sizes), 0.5, 7, 3, 0, 2**20 + 1)
        assert got.size == 524707 and got[-3:].tolist() == [1048572, 1048573, 1048576] and int(got.astype(np.int64).sum()) == 274795070813
    # a sub-range that starts inside a block and a wave and ends in the last slice
    _check(ds, max(sizes), 0.5, 11, 5, 12345, max(sizes) - 77)


def test_an_empty_sample_is_a_tensor_of_no_rows():
    ds = _dataset(64)
    want = gbrl_amd.gbrl_cpp.sample_rows_host(64, 2.0**-24, seed=0, draw=0)
    assert want.size == 0, "the premise: this draw keeps no row"
    t = _device_sample(ds, 2.0**-24, 0, 0)
    assert tuple(t.shape) == (0,)
    assert t.cpu().numpy().shape == (0,)


def test_the_sample_is_a_legal_rows_vector_and_the_c_call_writes_host_and_device():
    import torch
    n, F, D = 3000, 3, 2
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, F)).astype(np.float32)
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=3, n_bins=16, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cpu")
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    ds = m.prepare_dataset(X)
    rows = _device_sample(ds, 0.3, 9, 0)
    k = rows.numel()
    assert 0 < k < n
    g = torch.from_numpy(rng.standard_normal((k, D)).astype(np.float32)).cuda()
    dev = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    m.step_prepared(ds, dev(g), rows=dev(rows))
    assert m.get_num_trees() == 1
    base = torch.zeros((k, D), dtype=torch.float32, device="cuda")
    assert m.predict_continue_prepared(ds, dev(base), 0, 1, rows=dev(rows)) is None
    want = np.asarray(m.predict_continue_prepared(ds, np.zeros((k, D), np.float32), 0, 1, rows=rows.cpu().numpy()))
    assert base.cpu().numpy().tobytes() == want.tobytes()
    # the C entry: host and device outputs, the refusals that need a live data set
    lib = _lib()
    host = gbrl_amd.gbrl_cpp.sample_rows_host(n - 10, 0.3, seed=9, draw=2, row0=10)
    out = np.full(n, -7, np.int32)
    cnt = C.c_int(-1)
    assert lib.gbrl_hip_dataset_sample_rows(ds._handle(), 10, n - 10, 0.3, 9, 2, out.ctypes.data, 0, C.byref(cnt)) == 0, lib.gbrl_hip_last_error()
    assert cnt.value == host.size and np.array_equal(out[:cnt.value], host) and (out[cnt.value:] == -7).all()
    dout = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert lib.gbrl_hip_dataset_sample_rows(ds._handle(), 10, n - 10, 0.3, 9, 2, dout.data_ptr(), 1, C.byref(cnt)) == 0, lib.gbrl_hip_last_error()
    assert cnt.value == host.size and np.array_equal(dout.cpu().numpy()[:cnt.value], host) and (dout.cpu().numpy()[cnt.value:] == -7).all()
    for row0, cn in ((0, n + 1), (n, 1), (n - 5, 6), (1, n)):
        assert lib.gbrl_hip_dataset_sample_rows(ds._handle(), row0, cn, 0.3, 9, 2, out.ctypes.data, 0, C.byref(cnt)) == -1
        assert b"outside [0, %d)" % n in lib.gbrl_hip_last_error()
    for start, stop in ((0, n + 1), (5, 5), (-1, 4), (n, None)):
        with pytest.raises(RuntimeError, match="sample_rows: rows"):
            ds.sample_rows(0.5, start=start, stop=stop)
    with pytest.raises(RuntimeError, match="subsample"):
        ds.sample_rows(0.0)
    with pytest.raises(RuntimeError, match="draw"):
        ds.sample_rows(0.5, draw=-1)


# ---- the fused gather -------------------------------------------------------------------------------------------------------------------------
def _offset_matrix(torch, n, D, off, fill=None, bits=None):
    """[n, D] float32 on the device whose first element lies `off` floats behind a 16-byte boundary"""
    flat = torch.empty(n * D + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + n * D].view(n, D)
    if bits is not None:
        view.copy_(torch.from_numpy(bits).cuda().view(torch.float32))
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == 4 * off
    return flat, view


@pytest.mark.parametrize("D", [1, 3, 4, 8, 130])
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_the_gathered_rows_are_the_sampled_rows_bit_for_bit(D, off_in, off_out):
    import torch
    rpb, _ = _geometry()
    lib = _lib()
    n, row0 = 2 * rpb + 77, 1000
    rng = np.random.default_rng(100 * D + 10 * off_in + off_out)
    bits = rng.integers(-2**31, 2**31, size=(n, D), dtype=np.int64).astype(np.int32)   # every bit pattern, NaNs among them
    for p, seed, draw in ((0.5, 7, 3), (0.1, 2**63 + 5, 2**31 - 1), (1.0, 0, 0), (2.0**-24, 1, 1)):
        want_rows = gbrl_amd.gbrl_cpp.sample_rows_host(n, p, seed=seed, draw=draw, row0=row0)
        m = want_rows.size
        runs = []
        for _ in range(2):
            _, G = _offset_matrix(torch, n, D, off_in, bits=bits)
            _, G_out = _offset_matrix(torch, n, D, off_out, fill=-3.0)
            rows = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            cnt = C.c_int(-1)
            torch.cuda.synchronize()
            rc = lib.gbrl_hip_sample_gather(row0, n, p, seed, draw, G.data_ptr(), D, rows.data_ptr(), G_out.data_ptr(), C.byref(cnt))
            assert rc == 0, lib.gbrl_hip_last_error()
            assert cnt.value == m
            h_rows, h_out = rows.cpu().numpy(), G_out.cpu().numpy()
            assert np.array_equal(h_rows[:m], want_rows) and (h_rows[m:] == -7).all()
            assert np.array_equal(h_out[:m].view(np.int32), bits[want_rows - row0]), "D %d: gathered rows differ" % D
            assert (h_out[m:] == -3.0).all(), "written behind row m"
            assert np.array_equal(G.cpu().numpy().view(np.int32), bits), "the source was modified"
            runs.append((h_rows.tobytes(), h_out.tobytes()))
        assert runs[0] == runs[1], "two calls differ"


def test_two_calls_give_identical_bytes():
    ds = _dataset(5000)
    a = _device_sample(ds, 0.5, 7, 3).cpu().numpy().tobytes()
    b = _device_sample(ds, 0.5, 7, 3).cpu().numpy().tobytes()
    assert a == b and len(a) > 0
