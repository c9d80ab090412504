"""Key families of the quantile-leaf tests (read by tests/test_quantile_host.py, tests/test_gpu_quantile.py and tests/test_gpu_fit_quantile.py):
residual matrices x [m, D] written as exact float32 bit patterns, chosen by what the 8-bit radix passes over quantile_key(x) have to tell apart.
Data and NumPy only.

family(name, m, D, seed) returns (pred, targets) with pred = 0 and targets = -x, so that fl32(pred - targets) is x on the host and on the device
without a rounding (a zero of either sign becomes +0, which the key does anyway).  The one exception is "denormal_by_subtraction": pred and
targets are both normal numbers and their float32 difference is subnormal; its x is residual(pred, targets), NumPy's float32 subtraction, which
does not flush.  Every column has its own draw or permutation.

  distinct                 all-distinct values of both signs, random in every byte
  last_byte                0x3f800000 + r and its negative, r in 0..255: the three upper digits are one value per sign, the last pass decides
  third_byte, second_byte  the same with r << 8 and r << 16
  shared_prefix_ties       40 distinct keys with the same upper 16 bits (half of them with the same upper 24), each many times
  zeros_and_denormals      +-0, +-2^-149, +-(2^-126 - 2^-149), +-2^-126
  huge                     magnitudes from 2^127 to the largest finite float, both signs, the largest itself among them
  negative_only            negative values, random in every byte
  all_equal                one value
  denormal_by_subtraction  pred = 2^-125 (1 + j 2^-23) and targets = 2^-125 (or the two exchanged): x = +-j 2^-148, j < 5000
"""
import numpy as np

f32 = np.float32
FAMILIES = ("distinct", "last_byte", "third_byte", "second_byte", "shared_prefix_ties", "zeros_and_denormals", "huge", "negative_only", "all_equal",
            "denormal_by_subtraction")
TIE_KEYS = 40                          # distinct keys of shared_prefix_ties
SMALLEST_NORMAL = f32(2.0 ** -126)


def _float(bits):
    return np.ascontiguousarray(np.asarray(bits, np.uint32)).view(f32)


def _sign(rng, m):
    return rng.integers(0, 2, m).astype(np.uint32) << np.uint32(31)


def _byte_column(rng, m, shift):
    i = (rng.permutation(m) % 512).astype(np.uint32)      # every (sign, r) pair from 512 rows on, in a random order
    return (np.uint32(0x3f800000) + ((i & np.uint32(255)) << np.uint32(shift))) | ((i >> np.uint32(8)) << np.uint32(31))


def tie_pool(seed):
    """the 40 bit patterns of shared_prefix_ties, ascending: 0x3f80 in the upper 16 bits, 20 of them with 0x3f805a in the upper 24"""
    rng = np.random.default_rng(seed)
    low = np.concatenate([np.uint32(0x5a00) + rng.choice(256, TIE_KEYS // 2, replace=False).astype(np.uint32),
                          np.setdiff1d(rng.choice(0x10000, 4 * TIE_KEYS, replace=False), np.arange(0x5a00, 0x5b00))[: TIE_KEYS - TIE_KEYS // 2].astype(np.uint32)])
    assert len(np.unique(low)) == TIE_KEYS
    return np.sort(np.uint32(0x3f800000) + low)


def _column(name, rng, m, pool):
    if name == "distinct":
        return (np.uint32(0x30000000) + rng.choice(0x20000000, m, replace=False).astype(np.uint32)) | _sign(rng, m)
    if name == "last_byte":
        return _byte_column(rng, m, 0)
    if name == "third_byte":
        return _byte_column(rng, m, 8)
    if name == "second_byte":
        return _byte_column(rng, m, 16)
    if name == "shared_prefix_ties":
        return pool[rng.integers(0, TIE_KEYS, m)]
    if name == "zeros_and_denormals":
        eight = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000], np.uint32)
        return eight[rng.permutation(m) % 8]
    if name == "huge":
        mag = np.uint32(0x7f7fffff) - rng.integers(0, 0x00800000, m).astype(np.uint32)
        mag[0] = np.uint32(0x7f7fffff)
        return mag | _sign(rng, m)
    if name == "negative_only":
        return np.uint32(0x80000000) | (np.uint32(0x30000000) + rng.integers(0, 0x20000000, m).astype(np.uint32))
    if name == "all_equal":
        return np.full(m, 0xc0200000, np.uint32)   # -2.5
    raise KeyError(name)


def values(name, m, D, seed=0):
    """x float32 [m, D] of a family written as bit patterns (every family but denormal_by_subtraction)"""
    rng = np.random.default_rng([seed, FAMILIES.index(name), m, D])
    pool = tie_pool(seed)
    return np.ascontiguousarray(np.stack([_float(_column(name, rng, m, pool)) for _ in range(D)], axis=1))


def family(name, m, D, seed=0):
    """(pred, targets) float32 [m, D]: fl32(pred - targets) is the family's x"""
    if name != "denormal_by_subtraction":
        return np.zeros((m, D), f32), np.ascontiguousarray(-values(name, m, D, seed))
    rng = np.random.default_rng([seed, FAMILIES.index(name), m, D])
    j = rng.integers(0, 5000, (m, D)).astype(np.uint32)
    base = np.full((m, D), 0x01000000, np.uint32)          # 2^-125
    above = _float(base + j)                               # 2^-125 (1 + j 2^-23)
    flip = rng.integers(0, 2, (m, D)).astype(bool)
    return np.where(flip, _float(base), above).astype(f32), np.where(flip, above, _float(base)).astype(f32)


def residual(pred, targets):
    """x = fl32(pred - targets) in NumPy (no flush to zero); finite, or the family is wrong"""
    x = (pred.astype(f32) - targets.astype(f32)).astype(f32)
    assert np.isfinite(x).all()
    return x
