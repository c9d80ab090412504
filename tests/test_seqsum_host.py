"""The arithmetic of the parallel sequential float32 sum (gbrl_amd/csrc/seqsum_core.h: the functions the kernels of seqsum.hip are compiled
from) on the CPU, through the host walk gbrl_hip_seq_sums_model, which makes the kernels' decisions in the kernels' order: every sum must be
the plain loop's `s = float32(s + x)` BYTE FOR BYTE (NaN equals NaN).  Random chains cannot put a running sum exactly on a power of two, on
(2^24 - 1) u or on zero, so those are constructed (tests/seqsum_cases.py) -- and because a walk that always fell back to the loop would pass
every comparison, the number of 256-element blocks it may add element by element is bounded as well."""
import numpy as np

import seqsum_cases as S


def test_random_chains_equal_the_plain_loop():
    """(a) the ten kinds and the lengths of tests/test_gpu_seqsum.py, the same 400 chains"""
    chains, starts = S.random_chains()
    got, slow, fast = S.model(S.lib(), chains, starts)
    bad = S.mismatches(got, chains, starts)
    assert not bad, bad[:10]
    assert slow + fast == S.n_blocks(chains)
    print("400 chains, %d blocks: %d applied by summary, %d added element by element" % (S.n_blocks(chains), fast, slow))


def test_edges_of_the_binade_equal_the_plain_loop():
    """(b), (c): the sum exactly on +-2^k -- at the chain's start, on a block's first and last element, inside a block, where a group of 16
    blocks and a scan of 64 begin -- followed by opposite-sign elements of 2^-30 .. 1.5 u, again and again in one variant; the sum on
    (2^24 - 1) u followed by 0.4 .. 1 u of its own sign.  k: both ends of the accepted range, one beyond each, some in between."""
    fam = S.edge_families()
    got, slow, fast = S.model(S.lib(), [c.x for c in fam], [c.start for c in fam])
    bad = [(c.name, float(S.plain(c.x, c.start)), float(g)) for c, g in zip(fam, got) if not S.same(g, S.plain(c.x, c.start))]
    print("%d constructed chains, %d elements, %d blocks: %d by summary, %d element by element; %d wrong" % (
        len(fam), sum(c.n for c in fam), S.n_blocks([c.x for c in fam]), fast, slow, len(bad)))
    assert not bad, (len(bad), bad[:10])


def test_edge_chains_mostly_take_the_summaries():
    """(f) not a vacuous pass: per chain, the blocks added element by element are at most those that hold or directly follow an edge, plus the
    first block of a chain that starts from zero; beyond the accepted exponents nothing but the fallback runs.  The premise -- every other
    block keeps all its partial sums in [1.25, 1.75] 2^k, so any correct rule applies it -- is checked on the inputs first."""
    fam = S.edge_families()
    so = S.lib()
    assert {c.k for c in fam} >= {S.K_MIN - 1, S.K_MIN, S.K_MAX, S.K_MAX + 1} and {c.sign for c in fam} == {1, -1}
    over = []
    for c in fam:
        c.check_quiet()
        nb = (c.n + S.BLOCK - 1) // S.BLOCK
        _, slow, fast = S.model(so, [c.x], [c.start])
        assert slow + fast == nb, c.name
        if not c.in_range:
            assert fast == 0, c.name
        elif slow > c.cap:
            over.append((c.name, slow, c.cap, nb))
        assert c.in_range is False or c.cap < nb, c.name                   # (the bound binds: every chain has blocks that must be applied)
    assert not over, (len(over), over[:10])


def test_zero_signed_zero_subnormals_and_non_finite():
    """(d) exact cancellation to +0.0 and on; -0.0 kept by a -0.0 start and -0.0 elements -- also behind the chain's last element, inside a
    block -- and lost to one +0.0; subnormal elements under the smallest sums; inf and nan inside a group that is summarisable otherwise"""
    names, chains, starts = S.zero_family()
    got, slow, fast = S.model(S.lib(), chains, starts)
    bad = S.mismatches(got, chains, starts, names)
    assert not bad, (len(bad), bad[:10])
    assert slow + fast == S.n_blocks(chains)


def test_the_advisors_example():
    names, chains, starts, want = S.advice_example()
    got, _, _ = S.model(S.lib(), chains, starts)
    for n, c, s0, w, g in zip(names, chains, starts, want, got):
        assert S.plain(c, s0).tobytes() == w.tobytes(), n
        assert np.float32(g).tobytes() == w.tobytes(), (n, float(w), float(g))
    assert want[0] == np.float32(0.99999994) and want[0] < 1


def test_core_exhaustively_around_both_ends_of_the_binade():
    """(e) u = 1 (exponent 23): every start A0 in +-{2^23, 2^23 + 1, 2^23 + 2, 2^24 - 2, 2^24 - 1}, every run of one, two and three elements
    m / 8, |m| <= 24 (one block each, so the composed summary of the run is what is tried).  The summary must be applied exactly when A0 and
    every partial sum of the plain loop lie strictly between 2^23 and 2^24 on A0's side -- declined when a partial sum leaves that interval
    or touches its lower end -- and the sum is the loop's either way."""
    so = S.lib()
    lo, hi = float(1 << 23), float(1 << 24)
    elems = (np.arange(-24, 25) / 8.0).astype(np.float32)
    n_apply = n_decline = 0
    for a0 in (1 << 23, (1 << 23) + 1, (1 << 23) + 2, (1 << 24) - 2, (1 << 24) - 1):
        for sign in (1.0, -1.0):
            for run in (1, 2, 3):
                x = np.stack(np.meshgrid(*[elems] * run, indexing="ij"), -1).reshape(-1, run)   # [n][run]: every run
                s = np.full(len(x), sign * a0, np.float32)
                inside = np.full(len(x), lo < a0 < hi)
                for j in range(run):
                    s = s + x[:, j]                                                             # float32 arrays: the loop, all runs at once
                    inside &= (s * np.float32(sign) > lo) & (s * np.float32(sign) < hi)
                assert s.dtype == np.float32
                for sel, applied in ((inside, True), (~inside, False)):
                    n = int(sel.sum())
                    if n == 0: continue
                    got, slow, fast = S.model(so, x[sel], np.full(n, sign * a0, np.float32))
                    assert got.tobytes() == s[sel].tobytes(), (a0, sign, run, applied, int((got != s[sel]).sum()))
                    assert (slow, fast) == ((0, n) if applied else (n, 0)), (a0, sign, run, applied, slow, fast, n)
                    n_apply += n if applied else 0; n_decline += 0 if applied else n
    print("%d runs applied by summary, %d declined" % (n_apply, n_decline))
    assert n_apply > 0 and n_decline > 0
