"""The one-side sampling rule on the host (gbrl_cpp.goss_rows_host; include/gbrl_hip.h, "One-side sampling"), against a NumPy restatement
written from the header's text: a float32 score loop, a stable argsort for the tie rule, the row sampler's hash.  Every comparison is exact.  No
device is needed."""
import numpy as np
import pytest

import gbrl_amd
from gbrl_amd import gbrl_cpp

U64 = np.uint64
GOSS_STREAM = 0x676F737372657374


# ---- the rule, restated from its text -------------------------------------------------------------------------------------------------------------
def restate_u24(rows, seed, draw):
    with np.errstate(over="ignore"):
        x = (U64(draw) << U64(32)) | np.asarray(rows, np.int64).astype(np.uint64)
        z = x + U64((int(seed) + 1) % 2**64) * U64(0x9E3779B97F4A7C15)
        z ^= z >> U64(30); z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27); z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
        return (z >> U64(40)).astype(np.int64)


def restate_keys(G):
    G = np.asarray(G, np.float32).reshape(G.shape[0], -1)
    s = np.zeros(G.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(G.shape[1]):
            s = (s + (G[:, d] * G[:, d]).astype(np.float32)).astype(np.float32)   # float32 multiply, then float32 add: two roundings
    return s.view(np.uint32) & np.uint32(0x7FFFFFFF)


def restate_amp(a, b):
    return np.float32((1.0 - np.float64(a)) / np.float64(b))


def restate_goss(G, a, b, seed=0, draw=0, row0=0):
    """(rows, factor, gathered grads, n_top, tau_bits) of the rule"""
    G = np.asarray(G, np.float32)
    n = G.shape[0]
    G2 = G.reshape(n, -1)
    key = restate_keys(G2).astype(np.int64)
    k = int(np.floor(np.float64(a) * n))
    top = np.zeros(n, bool)
    order = np.argsort(-key, kind="stable")          # descending keys, equal keys in row order
    top[order[:k]] = True
    tau = int(key[order[k - 1]]) if k > 0 else 0x80000000
    p = np.float64(b) / (1.0 - np.float64(a))
    thr = min(2**24, int(np.floor(p * 16777216.0)))
    rows = np.arange(row0, row0 + n, dtype=np.int64)
    u = restate_u24(rows, int(seed) ^ GOSS_STREAM, draw)
    keep = top | (u < thr)
    amp = restate_amp(a, b)
    factor = np.where(top, np.float32(1.0), amp).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = np.where(top[:, None], G2, (amp * G2).astype(np.float32)).astype(np.float32)
    return rows[keep].astype(np.int32), factor[keep], scaled[keep].reshape((-1,) + G.shape[1:]), k, tau


def _grads(n, D, seed, kind="normal"):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full((n, D), 0.375, np.float32)
    if kind == "zero":
        return np.zeros((n, D), np.float32)
    if kind == "two":      # two distinct norms, about half each, interleaved at random
        return np.where(rng.random((n, 1)) < 0.5, np.float32(0.5), np.float32(0.25)).astype(np.float32) * np.ones((1, D), np.float32)
    return rng.standard_normal((n, D)).astype(np.float32)


def _check(G, a, b, seed=0, draw=0, row0=0):
    rows, factor = gbrl_cpp.goss_rows_host(G, a, b, seed=seed, draw=draw, row0=row0)
    want_rows, want_factor, _, k, _ = restate_goss(G, a, b, seed, draw, row0)
    assert rows.dtype == np.int32 and factor.dtype == np.float32
    assert rows.tobytes() == want_rows.tobytes(), (rows[:8], want_rows[:8])
    assert factor.tobytes() == want_factor.tobytes()
    if restate_amp(a, b) != np.float32(1.0):
        assert int((factor == np.float32(1.0)).sum()) == k == int(np.floor(np.float64(a) * G.shape[0]))
    return rows, factor


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("kind", ["normal", "equal", "two", "zero"])
def test_the_host_rule_is_its_text(n, D, kind):
    G = _grads(n, D, seed=100 * n + D, kind=kind)
    for a, b in ((0.2, 0.1), (0.1, 0.1), (0.5, 0.25), (0.0, 0.3)):
        _check(G, a, b, seed=7 + n, draw=3)
    _check(G, 0.2, 0.1, seed=2**64 - 1, draw=2**31 - 1, row0=12345)
    _check(G[:, 0] if D == 1 else G, 0.3, 0.2, row0=1)


def test_the_kth_key_falls_inside_a_tie_run():
    n, D = 1000, 3
    G = _grads(n, D, seed=5, kind="two")
    key = restate_keys(G)
    hi = int((key == key.max()).sum())
    assert 300 < hi < 700
    for k in (hi - 7, hi, hi + 7):           # inside the upper run, at its end, inside the lower run
        a = (k + 0.5) / n
        rows, factor = _check(G, a, 0.1, seed=11, draw=1)
        top_rows = rows[factor == np.float32(1.0)]
        want = np.argsort(-key.astype(np.int64), kind="stable")[:k]
        assert sorted(top_rows.tolist()) == sorted(want.tolist())


def test_every_row_is_kept_when_the_rates_sum_to_one():
    # binary fractions: 1 - a is exact, so p == 1.0 and the threshold is 2**24 (a + b == 1 in decimal fractions can leave p one ulp below 1)
    n, D = 1000, 3
    G = _grads(n, D, seed=6)
    for a, b in ((0.25, 0.75), (0.5, 0.5), (0.0, 1.0), (0.875, 0.125)):
        rows, factor = _check(G, a, b, seed=9, draw=4, row0=50)
        assert rows.tolist() == list(range(50, 50 + n))
        amp = restate_amp(a, b)
        k = int(np.floor(a * n))
        assert int((factor.view(np.uint32) == amp.view(np.uint32)).sum()) == (n if amp == 1.0 else n - k)


@pytest.mark.parametrize("a,b,bits", [(0.2, 0.1, 0x41000000), (0.1, 0.1, 0x41100000), (0.0, 0.3, 0x40555555), (0.5, 0.5, 0x3F800000), (0.3, 0.0625, 0x41333333)])
def test_the_bits_of_the_amplification(a, b, bits):
    assert int(restate_amp(a, b).view(np.uint32)) == bits, hex(int(restate_amp(a, b).view(np.uint32)))
    G = _grads(64, 2, seed=8)
    G[:, :] = np.abs(G) + 1.0
    G[::2] *= 4.0        # the even rows are the top half
    rows, factor = gbrl_cpp.goss_rows_host(G, a, b, seed=1)
    other = factor[factor != np.float32(1.0)] if bits != 0x3F800000 else factor
    assert other.size > 0 and set(other.view(np.uint32).tolist()) == {bits}


def test_a_zero_top_rate_is_a_hash_draw_of_its_own_stream():
    n = 1000
    G = _grads(n, 2, seed=9)
    rows, factor = _check(G, 0.0, 0.25, seed=4, draw=6, row0=10)
    assert 150 < rows.size < 350 and (factor == np.float32(4.0)).all()
    plain = gbrl_cpp.sample_rows_host(n, 0.25, seed=4, draw=6, row0=10)
    assert rows.tolist() != plain.tolist(), "the other rows are drawn from a stream of their own"
    assert rows.tolist() == gbrl_cpp.sample_rows_host(n, 0.25, seed=4 ^ GOSS_STREAM, draw=6, row0=10).tolist()


def test_an_infinity_and_a_nan_rank_by_their_bits():
    G = np.array([[1.0], [np.inf], [np.nan], [3e38], [0.5], [-np.inf]], np.float32)   # 3e38 squared overflows to +inf
    rows, factor = _check(G, 0.5, 0.25, seed=0)
    key = restate_keys(G)
    assert key[2] > key[1] == key[3] == key[5] > key[0]
    assert rows[factor == np.float32(1.0)].tolist() == [1, 2, 3]      # the NaN, then the first two infinities in row order


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(float("nan"), 0.1), (0.1, float("nan")), (-0.01, 0.1), (1.0, 0.1), (1.5, 0.1), (0.1, 0.0), (0.1, -0.1), (0.1, 1.5), (0.0, 1.0000001),
                                 (0.6, 0.5), (0.9, 0.2), (0.0, 2.0**-25), (0.5, 2.0**-26)])
def test_bad_rates_are_refused(a, b):
    G = _grads(10, 2, seed=1)
    with pytest.raises(RuntimeError, match="goss"):
        gbrl_cpp.goss_rows_host(G, a, b)


def test_the_smallest_other_fraction_is_accepted():
    G = _grads(10, 2, seed=1)
    rows, factor = gbrl_cpp.goss_rows_host(G, 0.0, 2.0**-24)
    assert rows.size <= 1
    rows, factor = gbrl_cpp.goss_rows_host(G, 0.5, 2.0**-25)      # p = 2**-24
    assert rows.size >= 5


def test_bad_ranges_and_draws_are_refused():
    G = _grads(10, 2, seed=1)
    with pytest.raises(RuntimeError, match="row0"):
        gbrl_cpp.goss_rows_host(G, 0.2, 0.1, row0=-1)
    with pytest.raises(RuntimeError, match="draw"):
        gbrl_cpp.goss_rows_host(G, 0.2, 0.1, draw=-1)
    with pytest.raises(RuntimeError, match="2\\^31"):
        gbrl_cpp.goss_rows_host(G, 0.2, 0.1, row0=2**31 - 5)
    with pytest.raises(RuntimeError, match="no rows"):
        gbrl_cpp.goss_rows_host(np.zeros((0, 2), np.float32), 0.2, 0.1)
    with pytest.raises(RuntimeError):
        gbrl_cpp.goss_rows_host(np.zeros((4, 2), np.float64), 0.2, 0.1)
    with pytest.raises(RuntimeError, match="shape"):
        gbrl_cpp.goss_rows_host(np.zeros((4, 2, 2), np.float32), 0.2, 0.1)
