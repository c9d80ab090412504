"""Inputs and entry points shared by tests/test_seqsum_host.py (CPU: the host walk gbrl_hip_seq_sums_model) and tests/test_gpu_seqsum.py (the
kernels, gbrl_hip_seq_sums): the random chains, the plain loop they are compared with, and the CONSTRUCTED chains that put a running sum
exactly where the parity model of seqsum_core.h stops being the float32 add -- on a power of two (below it the spacing is u / 2, not u), on
(2^24 - 1) u, on zero -- which a random float32 sum never does.

A constructed chain of the edge families is: quiet blocks, an edge, quiet blocks (256-element blocks, the kernels' summary unit).  A quiet
block keeps every partial sum between 1.25 * 2^k and 1.75 * 2^k, so ANY correct rule applies it by summary; the block that holds an edge ends
with a step of 0.5 * 2^k that takes the sum back to the middle of the binade.  That is what lets the tests bound the number of blocks added
element by element (`Edge.cap`): a walk that always falls back is exact everywhere and must not pass."""
import ctypes
import functools
import os

import numpy as np

BLOCK = 256                    # kSeqBlock
LENGTHS = [0, 1, 2, 3, 63, 64, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097, 20000]
DUST = [2.0 ** -30, 0.25, 0.26, 0.3, 0.4, 0.5, 0.6, 0.75, 1.0, 1.25, 1.5]     # magnitudes, in units of u, of the elements that follow an edge
K_MIN, K_MAX = 21 - 127, 234 - 127                                          # the exponents the summaries accept (k_seq_summary: biased 21 .. 234)


def lib():
    import gbrl_amd
    so = ctypes.CDLL(os.path.join(os.path.dirname(gbrl_amd.__file__), "libgbrl_hip.so"))
    p = ctypes.c_void_p
    so.gbrl_hip_seq_sums.restype = ctypes.c_int
    so.gbrl_hip_seq_sums.argtypes = [p, p, p, ctypes.c_int, p, p]
    so.gbrl_hip_seq_sums_model.restype = ctypes.c_int
    so.gbrl_hip_seq_sums_model.argtypes = [p, p, p, ctypes.c_int, p, p, p]
    so.gbrl_hip_last_error.restype = ctypes.c_char_p
    return so


def _pack(chains, starts):
    if isinstance(chains, np.ndarray) and chains.ndim == 2:                # equally long chains, one per row
        return np.ascontiguousarray(chains, np.float32).ravel(), np.full(len(chains), chains.shape[1], np.uint32), np.ascontiguousarray(starts, np.float32), np.zeros(len(chains), np.float32)
    x = np.ascontiguousarray(np.concatenate(chains) if len(chains) else np.zeros(0, np.float32), np.float32)
    return x, np.array([len(c) for c in chains], np.uint32), np.ascontiguousarray(starts, np.float32), np.zeros(len(chains), np.float32)


def device(so, chains, starts):
    """-> sums, blocks added element by element (the kernels)"""
    x, lens, st, out = _pack(chains, starts)
    slow = np.zeros(1, np.uint32)
    rc = so.gbrl_hip_seq_sums(x.ctypes.data, lens.ctypes.data, st.ctypes.data, len(chains), out.ctypes.data, slow.ctypes.data)
    assert rc == 0, so.gbrl_hip_last_error()
    return out, int(slow[0])


def model(so, chains, starts):
    """-> sums, blocks added element by element, blocks applied by summary (the host walk)"""
    x, lens, st, out = _pack(chains, starts)
    slow, fast = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    rc = so.gbrl_hip_seq_sums_model(x.ctypes.data, lens.ctypes.data, st.ctypes.data, len(chains), out.ctypes.data, slow.ctypes.data, fast.ctypes.data)
    assert rc == 0, so.gbrl_hip_last_error()
    return out, int(slow[0]), int(fast[0])


def partials(x, start):
    """[start, fl(start + x0), fl(fl(start + x0) + x1), ...]: a cumulative float32 sum IS the plain loop s = float32(s + x)"""
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate((np.array([start], np.float32), np.asarray(x, np.float32))), dtype=np.float32)


def plain(x, start):
    return partials(x, start)[-1]


def same(a, b):
    """the same bytes; NaN equals NaN (sign and payload of a NaN are not the loop's to define)"""
    a, b = np.float32(a), np.float32(b)
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


def mismatches(got, chains, starts, names=None):
    bad = []
    for i, (c, s0) in enumerate(zip(chains, starts)):
        want = plain(c, s0)
        if not same(got[i], want):
            bad.append((names[i] if names else i, len(c), float(want), float(got[i])))
    return bad


def n_blocks(chains):
    return sum((len(c) + BLOCK - 1) // BLOCK for c in chains)


def chain(rng, kind, n):
    if kind == 0: return rng.standard_normal(n).astype(np.float32)
    if kind == 1: return (rng.standard_normal(n) + 0.3).astype(np.float32)
    if kind == 2: return (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3)).astype(np.float32)
    if kind == 3: return (np.round(rng.standard_normal(n) * 8) / 8 + 0.5).astype(np.float32)           # many exact ties
    if kind == 4: return (-np.abs(rng.standard_normal(n))).astype(np.float32)
    if kind == 5: return (rng.integers(-3, 4, n) * 0.25).astype(np.float32)                           # returns to zero again and again
    if kind == 6:
        x = (rng.standard_normal(n) + 1.0).astype(np.float32)
        x[rng.integers(0, n, max(1, n // 200))] = np.float32(1e30)                                   # elements far above the running sum
        x[rng.integers(0, n, max(1, n // 200))] = np.float32(-1e30)
        return x
    if kind == 7:
        x = (rng.standard_normal(n) * 1e-3 + 1.0).astype(np.float32)
        x[rng.integers(0, n, max(1, n // 100))] = np.float32(1e-38)                                  # subnormal-range dust
        x[rng.integers(0, n, max(1, n // 100))] = np.float32(0.0)
        return x
    if kind == 8:
        x = (rng.standard_normal(n) + 0.5).astype(np.float32)
        if n > 3: x[n // 2] = np.float32(np.inf) if rng.integers(0, 2) else np.float32(np.nan)
        return x
    return (np.float32(2.0) ** rng.integers(-30, 30, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)   # pure powers of two


def random_chains():
    """a COPY of the loop that draws the 400 chains in tests/test_gpu_seqsum.py::test_parallel_sequential_sums_equal_the_plain_loop_bit_for_bit
    (that test is kept as it was): the two have to be kept in step by hand"""
    rng = np.random.default_rng(5)
    chains, starts = [], []
    for t in range(400):
        n = LENGTHS[t % len(LENGTHS)] if t < 160 else int(rng.integers(1, 6000))
        chains.append(chain(rng, t % 10, n) if n else np.zeros(0, np.float32))
        starts.append(np.float32(0.0) if t % 3 else np.float32(rng.standard_normal() * 100))
    return chains, starts


# ---- constructed chains ---------------------------------------------------------------------------------------------------------------------

class Edge:
    """One chain under construction around P = sign * 2^k, u = 2^(k - 23).  `edges`: the blocks that hold an edge (the element that puts the
    sum on the edge and the elements that follow it there)."""

    def __init__(self, rng, name, k, sign, start, exact):
        self.rng, self.name, self.k, self.sign, self.exact = rng, name, k, sign, exact
        self.P, self.u = sign * 2.0 ** k, 2.0 ** (k - 23)
        self.start = np.float32(start)
        self.s, self.n, self.parts, self.edges = self.start, 0, [], set()

    def push(self, x, edge=False):
        x = np.atleast_1d(np.asarray(x, np.float64)).astype(np.float32)
        if len(x) == 0: return
        if edge:
            self.edges.update(range(self.n // BLOCK, (self.n + len(x) - 1) // BLOCK + 1))
        self.s = partials(x, self.s)[-1]
        self.n += len(x)
        self.parts.append(x)

    def quiet_to(self, end):
        """multiples of u / 8 (one in eight a tie) -- `exact`: of u, so that no add rounds and the fp64 prefix the kernels predict the exponent
        from IS the running sum -- a random walk of some 500 u a step around 1.5 P: 20 000 steps stay within 0.02 P of it"""
        n = end - self.n
        if n <= 0: return
        m = self.rng.integers(-500, 501, n) * 8 if self.exact else np.rint(self.rng.standard_normal(n) * 4000).astype(np.int64)
        m[self.rng.random(n) < 0.05] = 0
        x = m * 2.0 ** (self.k - 26)
        if self.n == 0 and self.start == 0:
            x[0] = 1.5 * self.P                                            # a chain from zero: its first block cannot be predicted
        self.push(x)

    def land(self, target):
        """one element that puts the running sum exactly on `target`"""
        x = target - np.float64(self.s)
        assert np.float64(np.float32(x)) == x
        self.push(x, edge=True)
        assert np.float64(self.s) == target, (self.name, float(self.s), target)

    def dust(self, cs, toward_zero=True):
        """elements of cs * u.  At the lowest exponents u is a few 2^20 subnormal steps: c * u is quantised to the 2^-149 grid (0.26 u stays
        0.26 u to 1e-6), and 2^-30 u underflows to 0.0f for k < -96 -- there the tiny dust IS a zero, everywhere else it must not be one"""
        x = np.array([(-c if toward_zero else c) * self.sign * self.u for c in cs]).astype(np.float32)
        assert all(v != 0 or (c * self.u <= 2.0 ** -150 and self.k < -96) for v, c in zip(x, cs)), (self.name, cs)
        self.push(x, edge=True)

    def close(self, step):
        """zeros to the block's last element, which is the step back to mid-binade"""
        pad = BLOCK - 1 - self.n % BLOCK
        self.push(np.concatenate((np.zeros(pad), [step * self.P])), edge=True)

    def finish(self, quiet_blocks=2):
        self.quiet_to((self.n // BLOCK + quiet_blocks) * BLOCK - int(self.rng.integers(0, 200)))
        self.x = np.concatenate(self.parts)
        self.in_range = K_MIN <= self.k <= K_MAX
        nb = (self.n + BLOCK - 1) // BLOCK
        # blocks that may be added element by element: those that hold or directly follow an edge, the first block of a chain from zero; every
        # block where the exponent is outside what the summaries accept
        self.cap = len({b for e in self.edges for b in (e, e + 1) if b < nb}) + (1 if self.start == 0 else 0) if self.in_range else nb
        return self

    def check_quiet(self):
        """the premise of `cap`: in every block without an edge the sum it starts from and all its partial sums lie in [1.25, 1.75] |P|, on P's side"""
        ps = partials(self.x, self.start).astype(np.float64) / self.P
        for b in range((self.n + BLOCK - 1) // BLOCK):
            if b in self.edges: continue
            q = ps[b * BLOCK + (1 if b == 0 and self.start == 0 else 0): min(self.n, (b + 1) * BLOCK) + 1]
            assert q.min() >= 1.25 and q.max() <= 1.75, (self.name, b, q.min(), q.max())


def _ks(rng):
    """both ends of the accepted range, one exponent beyond each (only the fallback may run there), fixed ones in between and a few drawn"""
    return [K_MIN - 1, K_MIN, K_MIN + 1, -64, -23, -1, 0, 1, 23, 64, K_MAX - 1, K_MAX, K_MAX + 1] + [int(v) for v in rng.integers(K_MIN + 2, K_MAX - 1, 4)]


PLACES = ("start", "block_first", "block_last", "mid_block", "group_4096", "chunk_16384")


def _lower_edge_chain(rng, k, sign, place, cs, idx):
    """the sum sits on P at `place`, then takes the opposite-sign elements cs * u"""
    name = "lower k=%d sign=%+d %s c=%s" % (k, sign, place, cs)
    if place == "start":
        c = Edge(rng, name, k, sign, sign * 2.0 ** k, idx % 2 == 0)
    else:
        c = Edge(rng, name, k, sign, 0.0 if idx % 4 < 2 else 1.5 * sign * 2.0 ** k, idx % 2 == 0)
        at = {"block_first": BLOCK, "block_last": 2 * BLOCK - 1, "mid_block": BLOCK + 1 + int(rng.integers(0, 200)), "group_4096": 4096 - 1, "chunk_16384": 16384 - 1}[place]
        c.quiet_to(at)
        c.land(c.P)
    c.dust(cs)
    c.close(0.5)
    return c.finish(15 if place in ("group_4096", "chunk_16384") else 2)


def _returning_chain(rng, k, sign, idx):
    """back onto P again and again: dust, j u up, back down onto P; across a block boundary"""
    c = Edge(rng, "returning k=%d sign=%+d" % (k, sign), k, sign, 0.0 if idx % 2 else 1.5 * sign * 2.0 ** k, idx % 4 < 2)
    c.quiet_to(BLOCK + 180)
    c.land(c.P)
    for _ in range(30):
        c.dust([DUST[int(rng.integers(0, len(DUST)))]] * int(rng.integers(1, 4)))
        c.push(int(rng.integers(1, 9)) * sign * c.u, edge=True)
        c.land(c.P)
    c.dust([0.4, 0.3])
    c.close(0.5)
    return c.finish()


def _upper_edge_chain(rng, k, sign, place, cu, idx):
    """the sum reaches (2^24 - 1) u, then takes cu * u of its own sign"""
    c = Edge(rng, "upper k=%d sign=%+d %s c=%s" % (k, sign, place, cu), k, sign, 0.0 if idx % 4 < 2 else 1.5 * sign * 2.0 ** k, idx % 2 == 0)
    c.quiet_to(2 * BLOCK - 1 if place == "block_last" else BLOCK + 1 + int(rng.integers(0, 200)))
    c.land(2 * c.P - sign * c.u)
    c.dust([cu], toward_zero=False)
    c.dust([0.3, 0.5, 0.25][:idx % 4], toward_zero=False)
    c.close(-0.5)
    return c.finish()


@functools.lru_cache(maxsize=None)
def edge_families():
    """families (b) and (c): a list of finished Edge chains.  Every dust size follows every short place at every k; at the two long places
    (elements 4096 and 16384: chains of 8192 and 20 480 elements) every size at k = 0 and k = K_MAX, one size of (0.25, 0.5] u elsewhere."""
    rng = np.random.default_rng(23)
    out, idx = [], 0
    ks = _ks(rng)
    for k in ks:
        for sign in (1, -1):
            for place in PLACES[:4]:
                for c in DUST:
                    out.append(_lower_edge_chain(rng, k, sign, place, [c] * (1 + (idx + 1) % 4), idx)); idx += 1
            for place in PLACES[4:]:                                       # the long ones: every dust size at k = 0 and at the upper end, else one
                for c in (DUST if k in (0, K_MAX) else [DUST[2 + idx % 4]]):  # per (k, sign, place), a size of (0.25, 0.5] u by rotation
                    out.append(_lower_edge_chain(rng, k, sign, place, [c] * (2 + idx % 2), idx)); idx += 1
            out.append(_returning_chain(rng, k, sign, idx)); idx += 1
            for place in ("mid_block", "block_last"):
                for cu in (0.5, 0.4, 0.6, 1.0):
                    out.append(_upper_edge_chain(rng, k, sign, place, cu, idx)); idx += 1
    return out


@functools.lru_cache(maxsize=None)
def zero_family():
    """family (d): names, chains, starts"""
    rng = np.random.default_rng(29)
    f32 = np.float32
    names, chains, starts = [], [], []

    def add(name, x, start):
        names.append(name); chains.append(np.asarray(x, np.float32)); starts.append(f32(start))

    # exact cancellation to +0.0 (round to nearest: x + -x = +0.0), in the middle of a block and on both sides of a block boundary, then on
    for k in (-100, 0, 60):
        for at in (100, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17):
            for start in (0.0, 1.5 * 2.0 ** k, -1.5 * 2.0 ** k):
                head = (np.rint(rng.standard_normal(at) * 4000) * 2.0 ** (k - 26)).astype(np.float32)
                s = plain(head, start)
                tail = (np.rint(rng.standard_normal(300) * 4000) * 2.0 ** (k - 26)).astype(np.float32)
                add("cancel k=%d at=%d start=%g" % (k, at, start), np.concatenate((head, [-s], tail)), start)
                add("cancel, stop k=%d at=%d start=%g" % (k, at, start), np.concatenate((head, [-s])), start)
                add("cancel, -0.0s k=%d at=%d start=%g" % (k, at, start), np.concatenate((head, [-s], np.full(40, -0.0))), start)
    # -0.0 survives only -0.0: a -0.0 start and -0.0 elements, ending inside a block (what stands behind the chain's end must not change it), on
    # a block boundary and beyond; a single +0.0 makes it +0.0 for good; then on
    mz = f32(-0.0)
    for n in (0, 1, 3, BLOCK - 1, BLOCK, BLOCK + 1, 600):
        add("-0.0 start, %d x -0.0" % n, np.full(n, mz), mz)
        add("+0.0 start, %d x -0.0" % n, np.full(n, mz), 0.0)
        if n >= 3:
            x = np.full(n, mz); x[n // 2] = 0.0
            add("-0.0 start, %d x -0.0, one +0.0" % n, x, mz)
            add("-0.0 start, %d x -0.0, then on" % n, np.concatenate((np.full(n, mz), chain(rng, 3, 300))), mz)
            add("-0.0 start, %d x -0.0, then on (negative)" % n, np.concatenate((np.full(n, mz), chain(rng, 4, 300))), mz)
    # subnormal elements (multiples of 2^-149 below 2^-126 = 8 u at the lowest accepted exponent) under the smallest running sums: quiet at both
    # ends of the accepted range's lower end, one exponent below it, a sum that wanders across 2^-106, a sum that stays subnormal
    for k in (K_MIN - 1, K_MIN, K_MIN + 1, K_MIN + 6):
        for sign in (1.0, -1.0):
            for start in (1.5, 1.0, 1.0 + 2.0 ** -20):
                x = (rng.integers(-(1 << 23) + 1, 1 << 23, 1000) * 2.0 ** -149).astype(np.float32)
                add("subnormal elements k=%d start=%g" % (k, sign * start), x, sign * start * 2.0 ** k)
    add("subnormal sum", (rng.integers(-1000, 1001, 700) * 2.0 ** -149).astype(np.float32), 0.0)
    add("subnormal sum from 2^-126", (rng.integers(-1000, 1001, 700) * 2.0 ** -149).astype(np.float32), 2.0 ** -126)
    # inf / nan inside a group of 16 blocks that is summarisable otherwise (quiet around 1.5, no add rounds)
    for what in ("inf", "-inf", "nan", "inf-inf", "overflow"):
        for at in (7 * BLOCK + 100, 16 * BLOCK, 19 * BLOCK + 255):
            x = (rng.integers(-500, 501, 24 * BLOCK) * 2.0 ** -23).astype(np.float32)
            if what == "overflow":
                x[at] = f32(3e38); x[at + 1] = f32(3e38); x[at + 300] = f32(-3e38)
            else:
                x[at] = {"inf": np.inf, "-inf": -np.inf, "nan": np.nan, "inf-inf": np.inf}[what]
                if what == "inf-inf": x[at + 300] = -np.inf
            add("%s at %d" % (what, at), x, 1.5)
    return names, chains, starts


def advice_example():
    """the smallest case: the sum is 1.0f and takes -0.4 * 2^-23; the loop steps down to 1 - 2^-24 = 0.99999994 (the spacing below 1.0 is 2^-24)"""
    names, chains, starts, want = [], [], [], []
    dust = np.float32(0.4 * 2.0 ** -23)
    for sign in (1.0, -1.0):
        z = np.zeros(BLOCK - 1, np.float32)
        for name, x, start in (("start %+g, one element" % sign, [-sign * dust], sign),
                               ("block 1 = [%+g, 0 ...], block 2 = [dust, 0 ...]" % sign, np.concatenate(([sign], z, [-sign * dust], z)), 0.0),
                               ("start %+g, a block of zeros, dust" % sign, np.concatenate((z, [0.0, -sign * dust])), sign)):
            names.append(name); chains.append(np.asarray(x, np.float32)); starts.append(np.float32(start))
            want.append(np.float32(sign * (1.0 - 2.0 ** -24)))
    return names, chains, starts, want
