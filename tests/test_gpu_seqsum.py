"""seqsum.hip: sequential float32 sums evaluated in parallel -- block summaries that depend on the running sum's parity only, the serial loop
where the running sum crosses a power of two -- must equal the plain loop `s = float32(s + x)` BIT FOR BIT (round 6; the near-tie replay's
chains over up to 2^20 rows, node.cpp:336-352).  Random chains with drift, without, heavy-tailed, tie-heavy (multiples of 1/8), sign changes,
cancellations, zeros, huge and tiny elements, inf / nan, lengths around the 256-element block size, non-zero starts."""
import ctypes
import os

import numpy as np
import pytest

import seqsum_cases as S
from seqsum_cases import chain as _chain      # the ten kinds of chains and the lengths: shared with tests/test_seqsum_host.py

pytestmark = pytest.mark.gpu


def _lib():
    import gbrl_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(gbrl_amd.__file__), "libgbrl_hip.so"))
    lib.gbrl_hip_seq_sums.restype = ctypes.c_int
    lib.gbrl_hip_seq_sums.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    return lib


def _plain(x, start):
    s = np.float32(start)
    with np.errstate(all="ignore"):
        for v in x:
            s = np.float32(s + v)
    return s


def _device(lib, chains, starts):
    x = np.ascontiguousarray(np.concatenate(chains) if chains else np.zeros(0, np.float32), np.float32)
    lens = np.array([len(c) for c in chains], np.uint32)
    st = np.ascontiguousarray(starts, np.float32)
    out = np.zeros(len(chains), np.float32)
    slow = np.zeros(1, np.uint32)
    rc = lib.gbrl_hip_seq_sums(x.ctypes.data, lens.ctypes.data, st.ctypes.data, len(chains), out.ctypes.data, slow.ctypes.data)
    assert rc == 0, lib.gbrl_hip_last_error()
    return out, int(slow[0])


def test_parallel_sequential_sums_equal_the_plain_loop_bit_for_bit():
    lib = _lib()
    rng = np.random.default_rng(5)
    lengths = S.LENGTHS
    chains, starts = [], []
    for t in range(400):
        n = lengths[t % len(lengths)] if t < 160 else int(rng.integers(1, 6000))
        chains.append(_chain(rng, t % 10, n) if n else np.zeros(0, np.float32))
        starts.append(np.float32(0.0) if t % 3 else np.float32(rng.standard_normal() * 100))
    got, slow = _device(lib, chains, starts)
    bad = []
    for i, (c, s0) in enumerate(zip(chains, starts)):
        want = _plain(c, s0)
        if np.float32(got[i]).tobytes() != want.tobytes() and not (np.isnan(got[i]) and np.isnan(want)):
            bad.append((i, i % 10, len(c), float(want), float(got[i])))
    assert not bad, bad[:10]
    n_blocks = sum((len(c) + 255) // 256 for c in chains)
    print("400 chains, %d blocks of 256 elements, %d took the serial fallback" % (n_blocks, slow))


def test_long_chains_mostly_take_the_summaries():
    """2^20-element chains of the replay's kinds (a drifting column sum, a zero-mean one, a dot chain of rounded products): exact, and all but a
    few per cent of the blocks are applied in O(1)."""
    lib = _lib()
    rng = np.random.default_rng(6)
    n = 1 << 20
    chains = [(rng.standard_normal(n) * 0.7 + 0.3).astype(np.float32), rng.standard_normal(n).astype(np.float32),
              ((rng.standard_normal(n) + 0.3) * np.float32(0.31)).astype(np.float32)]
    got, slow = _device(lib, chains, [0.0, 0.0, 0.0])
    for i, c in enumerate(chains):
        want = np.float32(0)
        # (the plain loop in NumPy scalars is slow: cumulative float32 sum IS the sequential loop)
        want = np.cumsum(c, dtype=np.float32)[-1]
        assert np.float32(got[i]).tobytes() == np.float32(want).tobytes(), (i, float(want), float(got[i]))
    n_blocks = 3 * (n // 256)
    print("3 chains of 2^20 elements: %d of %d blocks took the serial fallback" % (slow, n_blocks))
    assert slow <= n_blocks // 4


# ---- constructed chains (tests/seqsum_cases.py): running sums exactly on a power of two, on (2^24 - 1) u, on zero -----------------------------
# Each family goes through the kernels and through the host walk of the same arithmetic (gbrl_hip_seq_sums_model): both must give the plain
# loop's bytes, hence each other's (NaN equals NaN: which NaN an add returns is the hardware's choice); the blocks each added element by
# element are printed side by side (the walk makes the kernels' decisions in the kernels' order).

def _device_loop_and_model_agree(names, chains, starts):
    lib = S.lib()
    got, slow = S.device(lib, chains, starts)
    ref, m_slow, m_fast = S.model(lib, chains, starts)
    bad = S.mismatches(got, chains, starts, names)
    print("%d chains, %d blocks: the kernels added %d element by element, the host walk %d; %d sums differ from the plain loop" % (
        len(chains), S.n_blocks(chains), slow, m_slow, len(bad)))
    assert not bad, (len(bad), bad[:10])
    differ = [(n, float(r), float(g)) for n, r, g in zip(names, ref, got) if not S.same(r, g)]
    assert not differ, (len(differ), differ[:10])
    assert m_slow + m_fast == S.n_blocks(chains)
    return slow


def test_edges_of_the_binade_equal_the_plain_loop_and_the_host_walk():
    """The sum exactly on +-2^k (chain start, first / last element of a block, mid-block, elements 4096 and 16384: where a group of 16 blocks
    and a scan of 64 begin) followed by opposite-sign elements of 2^-30 .. 1.5 u, once and again and again; the sum on (2^24 - 1) u followed by
    0.4 .. 1 u of its own sign; k at both ends of the accepted range, one beyond each, and in between.  Below 2^k the spacing is u / 2, which
    the parity model does not know: a run that starts on or touches the power of two has to take the loop.  And not ALL runs may: the blocks
    added element by element are bounded by those that hold or directly follow an edge (the chains' other blocks keep every partial sum in
    [1.25, 1.75] 2^k; tests/test_seqsum_host.py checks that premise on the inputs)."""
    fam = S.edge_families()
    slow = _device_loop_and_model_agree([c.name for c in fam], [c.x for c in fam], [c.start for c in fam])
    cap = sum(c.cap for c in fam)
    assert slow <= cap, (slow, cap)


def test_zero_signed_zero_subnormals_and_non_finite_equal_the_plain_loop_and_the_host_walk():
    """Exact cancellation to +0.0 and on; -0.0 kept by a -0.0 start and -0.0 elements (also behind a chain's last element inside a block: the
    padding must be the identity of EVERY sum) and lost to one +0.0; subnormal elements under the smallest sums; inf / nan / overflow inside a
    group of 16 blocks that is summarisable otherwise."""
    _device_loop_and_model_agree(*S.zero_family())


def test_the_advisors_example():
    """s = 1.0f takes -0.4 * 2^-23: the loop steps down to 0.99999994 (the spacing below 1.0 is 2^-24); a summary that accepts a sum sitting ON
    the power of two keeps 1.0.  As the chain's start, as the sum a block ends on, and mirrored."""
    names, chains, starts, want = S.advice_example()
    got, _ = S.device(S.lib(), chains, starts)
    for n, w, g in zip(names, want, got):
        assert np.float32(g).tobytes() == w.tobytes(), (n, float(w), float(g))
    assert want[0] == np.float32(0.99999994) and want[0] < 1
