"""One-side sampling on the GPU (PreparedDataset.sample_goss; include/gbrl_hip.h, "One-side sampling").  Every comparison is exact: the device
returns the rows, the factors and the gathered gradient rows of the host rule (gbrl_hip_goss_rows_host, which tests/test_goss_host.py holds to
its text) byte for byte
  * at one lane, a wave edge, a block edge either side, several blocks, and 2^20 + 5 rows, where the one-block scan runs a second slice;
  * through the 16-byte and the 4-byte gather (D = 8, 128 against 1, 3);
  * with ties: all keys equal over several blocks with k inside a block and at a block boundary, a tie run that straddles two blocks;
  * on sub-ranges, for NumPy and device inputs, twice with the same bytes, and with top rows that do not depend on the draw.
"""
import ctypes as C

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

RPB = 2048   # the rows one block of the sampler owns (gbrl_hip_sample_rows_geometry; checked below)


def _lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci, d, u64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    lib.gbrl_hip_goss_rows_host.argtypes = [vp, ci, ci, ci, d, d, u64, ci, vp, vp, vp, vp]
    lib.gbrl_hip_sample_rows_geometry.argtypes = [vp, vp]
    lib.gbrl_hip_sample_rows_geometry.restype = None
    return lib


def _host(G, a, b, seed, draw, row0):
    """the host rule with its gathered gradient rows"""
    G = np.ascontiguousarray(G, np.float32)
    n = G.shape[0]
    D = 1 if G.ndim == 1 else G.shape[1]
    rows, factor, out, cnt = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, D), np.float32), C.c_int(0)
    lib = _lib()
    rc = lib.gbrl_hip_goss_rows_host(G.ctypes.data, D, row0, n, a, b, seed, draw, rows.ctypes.data, factor.ctypes.data, out.ctypes.data, C.byref(cnt))
    assert rc == 0, lib.gbrl_hip_last_error()
    m = cnt.value
    return rows[:m], factor[:m], out[:m].reshape((m,) + G.shape[1:])


_DS = {}


def _dataset(n, F=3):
    """a data set of at least n rows (the largest asked for so far is kept)"""
    if _DS.get("n", 0) < n:
        m = gbrl_amd.GBRL(input_dim=F, output_dim=1, policy_dim=1, max_depth=2, n_bins=8, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious",
                          device="cpu")
        _DS["ds"], _DS["n"] = m.prepare_dataset(np.random.default_rng(n).standard_normal((n, F)).astype(np.float32)), n
    return _DS["ds"]


def _dev(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def _device(ds, G, a, b, seed, draw, start, stop, on_device):
    import torch
    if not on_device:
        r = ds.sample_goss(G, a, b, seed=seed, draw=draw, start=start, stop=stop)
        assert all(isinstance(r[k], np.ndarray) for k in ("rows", "factor", "grads"))
        return r["rows"], r["factor"], r["grads"], r["n_top"], r["tau_bits"]
    t = torch.from_numpy(np.ascontiguousarray(G)).cuda()
    r = ds.sample_goss(_dev(t), a, b, seed=seed, draw=draw, start=start, stop=stop)
    rows, factor, grads = (torch.from_dlpack(r[k]) for k in ("rows", "factor", "grads"))
    assert rows.is_cuda and rows.dtype == torch.int32 and factor.dtype == torch.float32 and grads.dtype == torch.float32
    return rows.cpu().numpy(), factor.cpu().numpy(), grads.cpu().numpy(), r["n_top"], r["tau_bits"]


def _check(G, a, b, seed=0, draw=0, start=0, on_device=False, ds_rows=None):
    n = G.shape[0]
    ds = _dataset(max(ds_rows or 0, start + n))
    want = _host(G, a, b, seed, draw, start)
    got = _device(ds, G, a, b, seed, draw, start, start + n, on_device)
    what = "n %d D %s a %r b %r seed %d draw %d start %d device %s" % (n, G.shape[1:], a, b, seed, draw, start, on_device)
    assert got[0].shape == want[0].shape, "%s: %d rows against %d" % (what, got[0].size, want[0].size)
    assert got[0].tobytes() == want[0].tobytes(), what + ": rows"
    assert got[1].tobytes() == want[1].tobytes(), what + ": factor"
    assert got[2].shape == want[2].shape and got[2].tobytes() == want[2].tobytes(), what + ": grads"
    k = int(np.floor(np.float64(a) * n))
    assert got[3] == k
    if k > 0:   # tau is the k-th largest key
        key = np.zeros(n, np.float32)
        G2 = G.reshape(n, -1)
        for d in range(G2.shape[1]):
            key = (key + (G2[:, d] * G2[:, d]).astype(np.float32)).astype(np.float32)
        assert got[4] == int(np.sort(key.view(np.uint32) & np.uint32(0x7FFFFFFF))[n - k]), what + ": tau_bits"
    else:
        assert got[4] == 0x80000000
    return got


def _grads(n, D, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def test_the_geometry_the_sizes_below_are_chosen_for():
    rpb, width = C.c_int(0), C.c_int(0)
    _lib().gbrl_hip_sample_rows_geometry(C.byref(rpb), C.byref(width))
    assert rpb.value == RPB and width.value * rpb.value < 2**20 + 5, "2^20 + 5 rows are more block counts than one slice of the scan"


# ---- 1. sizes and both gather paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4100, 70001])
def test_the_device_sample_is_the_host_rule(n):
    for D in (1, 3, 8, 128):
        G = _grads(n, D, seed=10 * n + D)
        _check(G, 0.2, 0.1, seed=n + D, draw=3)
        _check(G, 0.1, 0.1, seed=2**64 - 1, draw=2**31 - 1, on_device=True)
    G = _grads(n, 8, seed=n)
    _check(G, 0.0, 0.3, seed=5, draw=1)              # no top rows
    _check(G, 0.25, 0.75, seed=5, draw=1)            # every row kept
    _check(G[:, 0].copy(), 0.5, 0.25, seed=6)        # a flat gradient vector: D = 1


def test_a_second_slice_of_the_scan():
    n = 2**20 + 5
    G = _grads(n, 1, seed=77)
    rows, factor, grads, n_top, _ = _check(G, 0.2, 0.1, seed=12, draw=9, on_device=True)
    assert n_top == n // 5 and int((factor == np.float32(1.0)).sum()) == n_top
    assert 0.29 * n < rows.size < 0.31 * n


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 8])
@pytest.mark.parametrize("k", [RPB + 1000, RPB, 2 * RPB, 1, 3 * RPB + 99])
def test_all_keys_equal_over_several_blocks(k, D):
    n = 3 * RPB + 100
    G = np.full((n, D), -0.625, np.float32)
    a = (k + 0.5) / n
    assert int(np.floor(np.float64(a) * n)) == k
    rows, factor, _, n_top, _ = _check(G, a, (1.0 - a) / 2, seed=3, draw=2, on_device=(D == 8))   # (half of the other rows)
    top = rows[factor == np.float32(1.0)]
    assert n_top == k and top.tolist() == list(range(k)), "the first k rows in row order are the top rows"


def test_a_tie_run_that_straddles_two_blocks():
    n = 5000
    rng = np.random.default_rng(21)
    g = (0.001 + 0.9 * rng.random(n)).astype(np.float32)
    g[RPB - 48:RPB + 52] = 2.0                                  # the tie run: 100 rows across the block edge
    above = rng.choice(np.setdiff1d(np.arange(n), np.arange(RPB - 48, RPB + 52)), 50, replace=False)
    g[above] = 3.0
    for take in (1, 48, 49, 60, 100):
        k = 50 + take
        for G in (g.reshape(n, 1), np.repeat(g.reshape(n, 1), 4, axis=1)):
            rows, factor, _, _, tau = _check(G, (k + 0.5) / n, 0.1, seed=8, draw=take)
            top = rows[factor == np.float32(1.0)]
            assert sorted(top.tolist()) == sorted(above.tolist() + list(range(RPB - 48, RPB - 48 + take)))
            assert tau == int(np.float32(4.0 * G.shape[1]).view(np.uint32))


def test_two_norms_with_random_ties():
    n = 3 * RPB + 7
    rng = np.random.default_rng(31)
    G = np.where(rng.random((n, 1)) < 0.4, np.float32(0.5), np.float32(0.125)).astype(np.float32) * np.ones((1, 3), np.float32)
    for a in (0.1, 0.4, 0.7):
        _check(G, a, 0.2, seed=9, draw=5)


# ---- 3. ranges, inputs, repeatability ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_sub_ranges(on_device):
    n_rows = 5000
    for start, stop in ((37, 4500), (1, n_rows), (RPB - 3, RPB + 70), (4999, 5000), (0, 65)):
        G = _grads(stop - start, 8, seed=start)
        _check(G, 0.2, 0.1, seed=4, draw=7, start=start, on_device=on_device, ds_rows=n_rows)
        _check(G[:, :3].copy(), 0.3, 0.3, seed=4, draw=7, start=start, on_device=on_device, ds_rows=n_rows)


def test_two_calls_return_the_same_bytes_and_the_draw_moves_only_the_other_rows():
    n, D = 3 * RPB + 500, 8
    G = _grads(n, D, seed=41)
    G[100:1100] = G[0]            # a tie run among the large rows as well
    one = _check(G, 0.2, 0.1, seed=13, draw=0, on_device=True)
    two = _check(G, 0.2, 0.1, seed=13, draw=0, on_device=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one[:3], two[:3]))
    other = _check(G, 0.2, 0.1, seed=13, draw=1, on_device=True)
    top = lambda r: r[0][r[1] == np.float32(1.0)]
    rest = lambda r: r[0][r[1] != np.float32(1.0)]
    assert top(one).tolist() == top(other).tolist() and top(one).size == n // 5
    assert rest(one).tolist() != rest(other).tolist()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ds = _dataset(5000)
    n = _DS["n"]
    G = _grads(100, 2, seed=1)
    for a, b in ((float("nan"), 0.1), (1.0, 0.1), (0.1, 0.0), (0.6, 0.5), (0.0, 2.0**-25), (-0.1, 0.2), (0.1, 1.1)):
        with pytest.raises(RuntimeError, match="goss"):
            ds.sample_goss(G, a, b, stop=100)
    with pytest.raises(RuntimeError, match="draw"):
        ds.sample_goss(G, 0.2, 0.1, draw=-1, stop=100)
    with pytest.raises(RuntimeError, match="range"):
        ds.sample_goss(G, 0.2, 0.1, start=n - 50, stop=n + 50)
    with pytest.raises(RuntimeError, match="rows"):
        ds.sample_goss(G, 0.2, 0.1, start=0, stop=99)
