"""Split scoring and selection cell by cell: k_score, k_argmax_stage1 and k_resolve_splits of step_score.hip through gbrl_hip_score_probe.

Group 1 holds every score to the exact integer reference of tests/score_cases.py (the expected float32 is the exact value rounded once; a cell
may differ from it only within ulp32 / 2 + exact * (D + 5) * 2^-53, the fp64 evaluation's own error; rejected candidates are exactly -inf, cells no
block stores keep the sentinel, row counts and histograms are compared exactly).  The later groups compare the fused greedy outputs and the
selection outputs bit for bit with the reduction rule (score_cases.select) applied on the host to the scores the probe returned in scores mode
for the same inputs.  Every test asserts on its own inputs that the edge it is meant to reach is reached.

The greedy branch of k_argmax_stage1 (oblivious = 0) has no case: no step reaches it -- greedy levels reduce inside k_score and the engine
launches argmax for oblivious levels only."""
import numpy as np
import pytest

import score_cases as S

pytestmark = pytest.mark.gpu

FIVE = (("acc",), ("der", 0), ("der", -1), ("zero",), ("der", 3))        # accumulated; derived with a sibling, without one, with an empty one


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(S.bits(got) != S.bits(want)) if got.dtype == np.float32 else np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d cells differ; first (index: got, expected): %s" % (
        what, len(bad), want.size, [(tuple(int(x) for x in i), got[tuple(i)], want[tuple(i)]) for i in bad[:6]])


def _check_scores(L):
    """scores mode against the exact reference -> (reference, probe output)"""
    R = S.reference_scores(L)
    o = S.probe(L, with_nr=True)
    assert o.rc == 0, o.error
    bad = S.score_failures(L, o.scores, R)
    off = int((S.bits(o.scores) != S.bits(R.scores)).sum())
    print("%d candidates, %d not bit-equal to the once-rounded value, %d outside the bound" % (o.scores.size, off, len(bad)))
    assert not bad, "%d scores miss the reference; first (node, candidate, got, expected): %s" % (len(bad), [(k, j, o.scores[k, j], R.scores[k, j]) for k, j in bad[:6]])
    assert not S.parent_failures(L, o.parent, R), (o.parent, R.parent)
    _same_bits(o.cand_nr, R.cand_nr, "cand_nr")
    _same_bits(o.hist, R.hist, "hist")
    return R, o


def _check_greedy(L, s, with_sn, **resolve):
    """the fused greedy form, and resolve_splits behind it when asked, against the rule applied to the scores `s` of the same inputs"""
    g = S.probe(L, do_score=2, with_s=with_sn, with_n=with_sn, do_resolve=int(bool(resolve)), **resolve)
    assert g.rc == 0, g.error
    pv, pi, ps, pn = S.expected_greedy_parts(L, s.scores, s.parent, s.cand_nr, with_sn)
    _same_bits(g.part_v, pv, "part_v")
    _same_bits(g.part_i, pi, "part_i")
    if with_sn:
        _same_bits(g.part_s, ps, "part_s")
        _same_bits(g.part_n, pn, "part_n")
    _same_bits(g.parent, s.parent, "parent")
    _same_bits(g.hist, s.hist, "hist")
    assert np.all(S.bits(g.scores) == S.SENT32)                                   # the fused form writes no scores
    if resolve:
        R = S.expected_resolve(L, pv, pi, ps if with_sn else None, pn if with_sn else None, oblivious=0, parent=s.parent,
                               **{k: v for k, v in resolve.items() if k != "do_resolve"})
        _check_resolve(g, R)
    return g, (pv, pi, ps, pn)


def _check_resolve(o, R):
    _same_bits(o.best_idx, R.best_idx, "best_idx")
    _same_bits(o.best_score, R.best_score, "best_score")
    _same_bits(o.counts4, R.counts4, "counts4")
    _same_bits(o.splits, R.splits, "splits")
    _same_bits(o.cursors, R.cursors, "cursors")


def _crossings(L, node, f):
    """how many steps of the running suffix sum of (node, slot f), over all fields, change the high word"""
    sfx = S.suffix_sums(S.obj(L.eff[node][f]))[1:, :L.D]
    hi = np.array([[int(x) >> 32 for x in row] for row in sfx])
    assert max(abs(int(x)) for x in sfx.ravel()) < 1 << 34
    return int((hi[1:] != hi[:-1]).sum()), hi[1:].size


# ------------------------------------------------------------------------------------------------------------ group 1: the scores

@pytest.mark.parametrize("NBe", [2, 3, 5, 64, 65, 255, 256, 257, 260, 261, 512, 513, 516, 517, 1030])
def test_class_count_edges_on_carry_data(NBe):
    """the block scan's tile edges: a last tile of 1..4 classes is added serially (257, 260, 513, 516), 261 and 517 take another full tile.  Numeric
    and categorical slots side by side, a categorical slot of 33 classes (or fewer) next to them, a slot without candidates; accumulated and
    derived nodes; the data carry or borrow across 2^32 in almost every add.  keep_derived = 1: derived slices are written for NBe classes only."""
    nc = NBe - 1
    slots = [(0, nc), (1, min(32, nc)), (0, 0), (1, nc), (0, min(nc, 7))]
    L = S.make_level(NBe, 3, slots, nodes=FIVE, data="carry", min_data=1)
    L.is_root[0] = 1
    assert L.NB == NBe and np.all(L.hist[4] == S.SENT64) and int(L.eff[0][0][:, 3].sum()) > 0 and int(L.eff[3][0][:, 3].sum()) == 0
    if nc >= 8:
        n, of = _crossings(L, 0, 0)
        assert n >= 0.9 * of, (n, of)
    R, s = _check_scores(L)
    assert np.all(R.hist[1, 0, :NBe] == L.eff[1][0]) and np.all(R.hist[0] == L.hist[0])                      # derived: written; accumulated: untouched
    assert np.all(R.hist[1, 1, min(32, nc) + 1:] == S.SENT64) and np.all(R.hist[1, 2, 1:] == S.SENT64) and np.all(R.hist[:, 5] == S.SENT64)
    assert np.all(R.scores[3] == -np.inf)                                                                  # the node without rows: every side is below min_data
    _check_greedy(L, s, with_sn=NBe % 2 == 1)


@pytest.mark.parametrize("D", [1, 8, 9, 17, 18, 35])
def test_field_count_edges(D):
    """the scan runs in passes of nine fields: D + 1 = 2, 9, 10, 18, 19 and 36 fields are one, one, two, two, three and four passes; 261 classes
    (two tiles), 257 (the serial remainder) and a categorical slot; L2 and Cosine alternate"""
    L = S.make_level(100 + D, D, [(0, 260), (1, 32), (0, 256)], nodes=(("acc",), ("der", 0)), data="carry", cosine=D % 2)
    assert -(-(D + 1) // 9) == {1: 1, 8: 1, 9: 2, 17: 2, 18: 3, 35: 4}[D]
    n, of = _crossings(L, 0, 0)
    assert n >= 0.9 * of
    _, s = _check_scores(L)
    _check_greedy(L, s, with_sn=True)


@pytest.mark.parametrize("data,cosine", [("big", 0), ("big", 1), ("negative", 0), ("negative", 1), ("zero", 0), ("random", 1)])
def test_magnitudes(data, cosine):
    """sums at +-(2^52 - 1) with sbits = 40 and nodes of up to 2^26 rows; all-negative fields; all-zero classes; a level of zeros only (min_data = 0)"""
    big = data == "big"
    L = S.make_level(13, 9, [(0, 516), (1, 40), (0, 64)], nodes=(("acc",), ("der", 0), ("zero",)), data=data, cosine=cosine, sbits=40 if big else 20,
                     count_max=(1 << 26) // 300 if big else 50, min_data=0 if data == "zero" else 1)
    sfx = S.suffix_sums(S.obj(L.eff[0][0]))
    top = max(abs(int(x)) for x in sfx[1:, :9].ravel())
    if big:
        assert (1 << 52) - (1 << 32) < top < (1 << 52) + (1 << 32) and 1 << 25 < max(int(x) for x in sfx[:, 9]) <= 1 << 26
    if data == "negative":
        assert all(int(x) <= 0 for x in sfx[1:, :9].ravel())
    if data != "zero":
        assert any(not L.eff[0][0][c].any() for c in range(1, 517))                                       # an all-zero class
    R, s = _check_scores(L)
    if data == "zero":
        # class 0 holds every row: each candidate sends nothing right and scores what the parent scores; the node without rows scores 0, and nothing is rejected
        assert int(L.eff[0][0][0, 9]) > 0 and np.all(R.scores[0] == R.parent[0]) and R.parent[0] > 0 and np.all(R.scores[2] == 0) and R.parent[2] == 0
    _check_greedy(L, s, with_sn=True)


@pytest.mark.parametrize("NBe", [33, 257, 1030])
def test_the_last_level_keeps_every_sentinel(NBe):
    """keep_derived = 0: the derived nodes are scored from parent - sibling and nothing is written back; k_resolve_splits then derives the child
    sizes from the same two slices itself"""
    nc = NBe - 1
    L = S.make_level(NBe + 1, 4, [(0, nc), (1, 32), (0, 0), (1, nc)], nodes=FIVE, data="random")
    L.keep_derived = 0
    assert int(L.eff[0][0][:, 4].sum()) > 0                                                                # the sibling of node 1 has rows
    R, s = _check_scores(L)
    assert np.array_equal(R.hist, L.hist) and np.all(L.hist[[1, 2, 4]] == S.SENT64)
    _check_greedy(L, s, with_sn=True, near=1, near_rel=2.0 ** -20, seg_start=[0, 100, 300, 600, 600], thr_keys=True)


@pytest.mark.parametrize("min_data", [0, 1, 3])
def test_min_data(min_data):
    L = S.make_level(20 + min_data, 2, [(0, 70), (1, 20)], nodes=(("acc",), ("der", 0), ("zero",)), min_data=min_data, count_max=1)
    R, s = _check_scores(L)
    one_side = 0
    for f, (base, nc) in enumerate(((0, 70), (70, 20))):
        E = L.eff[0][f]
        for c in range(nc):
            n_r = int(E[c + 1, 2] if f else E[c + 1:, 2].sum())
            n_l = int(E[:, 2].sum()) - n_r
            assert (R.scores[0, base + c] == -np.inf) == (n_l < min_data or n_r < min_data)
            one_side += (n_l < min_data) != (n_r < min_data)
    assert one_side > 0 or min_data < 3                                                                   # min_data = 3 rejects candidates for ONE side only
    assert np.all(np.isfinite(R.scores[2])) == (min_data == 0)                                             # the node without rows
    _check_greedy(L, s, with_sn=False)


def test_path_rejection():
    """the node's path: lengths 0, 1 and 32; all 32 entries on one slot; entries of other slots; entries behind path_len that would match; a numeric
    match is by threshold VALUE (a repeated threshold falls twice), a categorical one by bin == k + 1.  min_data = 0: only the path rejects."""
    L = S.make_level(31, 2, [(0, 40), (1, 12), (0, 40)], nodes=(("acc",),) * 4, min_data=0)
    L.thr[0, 8] = L.thr[0, 7]                                                                              # candidates 7 and 8 of slot 0 share a threshold
    L.thr[2, :40] = L.thr[0, :40]                                                                          # slot 2 has slot 0's values: a match must look at the slot
    S.set_path(L, 0, [(0, L.thr[0, 3], 0), (1, 0.0, 5)], length=0)                                         # path_len 0: entries that would match
    S.set_path(L, 1, [(1, 0.0, 12)] + [(0, L.thr[0, 5], 0)] * 31, length=1)                                # path_len 1: the last categorical class
    S.set_path(L, 2, [(0, L.thr[0, i], 0) for i in range(32)])                                             # 32 entries, all on slot 0, thresholds 0..31
    mixed = [(0, L.thr[0, 7], 0), (1, 0.0, 1), (3, L.thr[0, 0], 1), (2, L.thr[2, 39], 0), (1, 0.0, 7), (0, 123.5, 0), (1, 0.0, 0), (1, 0.0, 13)]
    S.set_path(L, 3, mixed * 4, length=20)                                                                 # 20 of 32; positions 20.. repeat matches
    L.path_slot[3, 20:], L.path_val[3, 20:], L.path_bin[3, 20:] = [0, 1, 2] * 4, L.thr[0, 20], 3            # behind path_len: would reject slot 0's 20, class 3, slot 2's 20
    R, s = _check_scores(L)
    want = {0: set(), 1: {40 + 11}, 2: set(range(32)), 3: {7, 8, 40 + 0, 40 + 6, 52 + 39}}
    for k in range(4):
        assert set(np.flatnonzero(R.scores[k] == -np.inf).tolist()) == want[k], k
    _check_greedy(L, s, with_sn=True)


def test_launch_window():
    """slot0 > 0 with fewer slots launched than the table holds: the other slots' candidates keep the sentinel, the parent comes from the first
    LAUNCHED slot, and part_* are indexed by block"""
    L = S.make_level(41, 5, [(0, 30), (1, 9), (0, 300), (0, 12)], nodes=FIVE)
    L.slot0, L.n_slots = 1, 2
    R, s = _check_scores(L)
    assert np.all(S.bits(R.scores[:, :30]) == S.SENT32) and np.all(S.bits(R.scores[:, 339:]) == S.SENT32) and np.all(R.hist[1, [0, 3]] == S.SENT64)
    g, (pv, pi, ps, pn) = _check_greedy(L, s, with_sn=True)
    assert g.part_v.shape == (5, 2) and set(L.cand_slot[L.ref_to_internal[pi[0]]].tolist()) == {1, 2}


# ------------------------------------------------------------------------------------------------------------ group 2: near ties

def _tie_level(rows, placed, n_slots=2, nc=300):
    """one node of `rows` rows, D = 1, weights 1, parent 0: every candidate sends half the rows right with a zero sum (gain 0) except `placed`,
    (slot, candidate, right sum, right rows): with total sum 0 the gain is s^2 (1 / n_r + 1 / (rows - n_r)), the same bits for n_r and its mirror"""
    L = S.make_level(0, 1, [(0, nc)] * n_slots, data="zero", sbits=0, min_data=1)
    L.cand_w[:] = 1
    L.cand_ref[:] = np.arange(L.n_cand)
    L.ref_to_internal[:] = np.arange(L.n_cand)
    for f in range(n_slots):
        sfx = np.zeros((nc + 1, 2), np.int64)
        sfx[:, 1] = rows // 2
        sfx[0] = (0, rows)
        for (ff, c, s, n_r) in placed:
            if ff == f:
                sfx[c + 1] = (s, n_r)
        S.set_suffix(L, 0, f, sfx)
    return L


@pytest.mark.parametrize("rows", [1000, 1024, 1025, 6000])
@pytest.mark.parametrize("where", ["same-wave", "other-wave", "same-thread", "other-slot", "same-sizes"])
def test_near_tie_classes(rows, where):
    """equal gains with different right counts are a runner-up at distance 0 in nodes of more than 1024 rows, and one class (by the gain alone) in
    smaller ones; equal gains with EQUAL right counts never are.  The winner and its mirror sit in one wave, in two waves, in one thread's own loop
    (candidates 256 apart) and in two slots: the per-thread loop, the wave shuffles, the four-wave merge and k_resolve_splits each meet the tie."""
    a, b = rows // 4, rows - rows // 4
    spot = {"same-wave": (0, 40), "other-wave": (0, 130), "same-thread": (0, 3 + 256), "other-slot": (1, 77), "same-sizes": (0, 40)}[where]
    placed = [(0, 3, 64, a), (spot[0], spot[1], -64, a if where == "same-sizes" else b), (0, 200, 32, a), (1, 10, 16, b)]
    L = _tie_level(rows, placed)
    R, s = _check_scores(L)
    j1, j2 = 3, spot[0] * 300 + spot[1]
    assert R.scores[0, j1] == R.scores[0, j2] > R.scores[0, 200] > R.scores[0, 310] > 0 == R.scores[0, 5] and R.parent[0] == 0           # the tie is a tie
    assert (R.cand_nr[0, j1] != R.cand_nr[0, j2]) == (rows > 1024 and where != "same-sizes")
    g, (pv, pi, ps, pn) = _check_greedy(L, s, with_sn=True, near=1, near_rel=2.0 ** -20, seg_start=[0])
    tie = rows > 1024 and where != "same-sizes"
    if where != "other-slot":
        assert (ps[0, 0] == pv[0, 0]) == tie and pi[0, 0] == j1 and (tie or ps[0, 0] == R.scores[0, 200])
    assert g.best_idx[0] == j1 and g.counts4[2, 0] == int(tie)                                             # flagged at distance 0, and only then
    assert np.array([g.counts4[3, 0]], np.int64).astype(np.int32).view(np.float32)[0] == (pv[0].max() if tie else R.scores[0, 200])
    # part_s / part_n absent: classes by the gain alone, and no near words
    g2, _ = _check_greedy(L, s, with_sn=False, seg_start=[0])
    assert g2.counts4[2, 0] == 0 and g2.best_idx[0] == j1


# ------------------------------------------------------------------------------------------------------------ group 3: k_argmax_stage1, the oblivious form

@pytest.mark.parametrize("n_nodes", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("n_cand", [1, 255, 256, 257, 600])
def test_argmax_oblivious(n_nodes, n_cand):
    """the sum over the nodes is float32, eight loads wide, in node order (data whose float32 sum depends on the order); 256 candidates per block;
    ties across blocks go to the lowest reference index; resolve_splits behind it, one winner for every node"""
    L = S.make_level(n_nodes * 1000 + n_cand, 1, [(0, n_cand)], nodes=(("acc",),) * n_nodes, count_max=400)
    rng = np.random.default_rng(n_nodes + n_cand)
    scores = (rng.standard_normal((n_nodes, n_cand)) * 10.0 ** rng.integers(-3, 4, size=(n_nodes, n_cand))).astype(np.float32)
    small = rng.random(n_cand) < 0.5
    scores[:, small] = rng.integers(0, 2, size=(n_nodes, int(small.sum())))                                 # sums that tie
    scores[rng.integers(0, n_nodes), rng.random(n_cand) < 0.2] = -np.inf
    L.cand_w[small] = 1
    if n_cand > 256:
        scores[:, 256], L.cand_w[256] = 1e6, 1
        scores[:, 40], L.cand_w[40] = 1e6, 1                                                                # the same best in two blocks
    pv, pi, ps, sc = S.expected_argmax(L, scores)
    if n_nodes > 2 and n_cand > 200:
        reverse = np.zeros(n_cand, np.float32)
        for k in reversed(range(n_nodes)):
            reverse = (reverse + scores[k]).astype(np.float32)
        assert np.any((reverse * L.cand_w).astype(np.float32)[np.isfinite(sc)] != sc[np.isfinite(sc)])     # the order of the sum shows
    if n_cand > 256:
        assert pv[0] == pv[1] and len(np.unique(sc[np.isfinite(sc) & small])) < small.sum()
    seg = np.arange(n_nodes) * 7
    o = S.probe(L, do_score=0, do_argmax=1, do_resolve=1, oblivious=1, scores=scores, with_s=True, near=1, near_rel=2.0 ** -12, near_rows=16384, seg_start=seg)
    assert o.rc == 0, o.error
    _same_bits(o.part_v[0], pv, "part_v")
    _same_bits(o.part_i[0], pi, "part_i")
    _same_bits(o.part_s[0], ps, "part_s")
    assert np.all(S.bits(o.part_v[1:]) == S.SENT32)                                                        # one result for the level
    R = S.expected_resolve(L, pv[None], pi[None], ps[None], None, oblivious=1, near=1, near_rel=2.0 ** -12, near_rows=16384, seg_start=seg)
    _check_resolve(o, R)
    i, v, _ = S.merge_parts(pv, pi, None, None)
    assert o.best_idx[0] == (0 if i == S.NO_CAND else i) and np.all(o.splits[:, 1:4] == o.splits[0, 1:4])


# ------------------------------------------------------------------------------------------------------------ group 4: k_resolve_splits on given parts

RESOLVE_SLOTS = [(0, 1), (0, 63), (1, 64), (0, 64), (0, 511), (1, 5), (0, 512), (0, 1029)]          # 2, 64, 65, 65, 512, 6, 513 and 1030 classes


def _resolve_level(seed):
    L = S.make_level(seed, 2, RESOLVE_SLOTS, nodes=(("acc",),) * 3, count_max=30)
    L.is_root[1] = 1
    return L


def _random_parts(L, rng, n_parts, winner=None):
    shape = (L.n_nodes, n_parts)
    pv = rng.choice(np.array([-np.inf, -1.5, 0.25, 0.25, 1.0, 3.0, 3.0], np.float32), size=shape)
    pi = rng.integers(0, L.n_cand, size=shape).astype(np.int32)
    pi[pv == -np.inf] = S.NO_CAND
    ps = np.where(rng.random(shape) < 0.5, pv, np.float32(-np.inf)).astype(np.float32)
    ps = np.minimum(ps, pv - np.float32(0.5) * (rng.random(shape) < 0.7)).astype(np.float32)
    pn = rng.integers(0, 3, size=shape).astype(np.int32)
    if winner is not None:
        q = int(rng.integers(0, n_parts))
        pv[:, q], pi[:, q] = 7.0, winner
    return pv, pi, ps, pn


@pytest.mark.parametrize("n_parts", [1, 63, 64, 65, 200])
def test_resolve_part_counts(n_parts):
    """the strided loop of one wave over 1, 63, 64, 65 and 200 per-block results, then the shuffles; with and without the near-tie words"""
    L = _resolve_level(n_parts)
    rng = np.random.default_rng(n_parts)
    parts = _random_parts(L, rng, n_parts)
    parts[0][2, 0], parts[1][2, 0], parts[2][2, 0] = 9.0, 5, -np.inf                                       # node 2: one best far above the rest
    parent = rng.random(L.n_nodes).astype(np.float32)
    seg = [5, 50, 500]
    flags = set()
    for near, rel in ((1, 2.0 ** -20), (1, 0.6), (0, 0.0)):
        o = S.probe(L, do_score=0, do_resolve=1, parts=parts, near=near, near_rel=rel, parent=parent, seg_start=seg)
        assert o.rc == 0, o.error
        R = S.expected_resolve(L, *parts, oblivious=0, near=near, near_rel=rel, parent=parent, seg_start=seg)
        _check_resolve(o, R)
        _same_bits(o.hist, L.hist, "hist")
        flags |= set(R.counts4[2, :3].tolist()) if near else set()
        assert near or R.counts4[2, :3].tolist() == [0, 0, 0]
    assert flags == {0, 1} or n_parts == 1                                                                 # both answers of the near-tie flag
    # oblivious: row 0 serves every node, one flag, the other nodes' near words cleared
    o = S.probe(L, do_score=0, do_resolve=1, oblivious=1, parts=parts[:3] + (None,), near=1, near_rel=0.6, near_rows=10000, seg_start=seg)
    assert o.rc == 0, o.error
    R = S.expected_resolve(L, parts[0], parts[1], parts[2], None, oblivious=1, near=1, near_rel=0.6, near_rows=10000, seg_start=seg)
    _check_resolve(o, R)
    assert R.counts4[2, 1] == 0 and R.counts4[3, 1] == S.SENT64 and np.all(S.bits(R.best_score[1:]) == S.SENT32)


@pytest.mark.parametrize("slot", range(len(RESOLVE_SLOTS)))
@pytest.mark.parametrize("last", [0, 1], ids=["first-bin", "last-bin"])
def test_resolve_winner_slots(slot, last):
    """winners in slots of 2, 64, 65, 512, 513 and 1030 classes, numeric and categorical, first and last bin: the class counts right of the bin;
    seg_start given (do_split, n_left, cursors zeroed) and absent; hist_global given (a second pair of counts, no near words) and null"""
    L = _resolve_level(50 + slot)
    is_cat, nc, base = (int(x) for x in L.slots[slot, :3])
    j = base + (nc - 1 if last else 0)
    parts = _random_parts(L, np.random.default_rng(slot), 65, winner=int(L.cand_ref[j]))
    glob = np.where(L.hist == S.SENT64, S.SENT64, L.hist * 3 + 1)
    for seg, hg, keys in (([9, 99, 999], None, True), (None, glob, True), ([1, 2, 3], glob, False)):
        o = S.probe(L, do_score=0, do_resolve=1, parts=parts, seg_start=seg, hist_global=hg, thr_keys=keys, max_front=5)
        assert o.rc == 0, o.error
        R = S.expected_resolve(L, *parts, oblivious=0, near=0, seg_start=seg, hist_global=hg, thr_keys=keys, max_front=5)
        _check_resolve(o, R)
        assert R.splits[0, 1] == slot and R.splits[0, 2] == (j - base + is_cat) and R.splits[0, 3] == is_cat
        assert (R.splits[0, 0], R.splits[0, 4]) == ((1, seg[0]) if seg else (0, 0)) and np.all(R.cursors == (0 if seg else S.SENT32))
        assert R.counts4[3, 0] == (int(np.array([-np.inf], np.float32).view(np.int32)[0]) if hg is None else R.counts4[1, 0] * 3 + (1 if is_cat else nc - (j - base)))
        assert np.all(R.counts4[:, 3:] == S.SENT64)                                                        # max_front 5, three nodes
    assert R.splits[0, 6] == 0 and (is_cat or o.splits[0, 6] == 0)


def test_resolve_no_winner_and_negative_zero():
    """all -inf: index 0 and no split.  A best gain of -0.0f splits (greedy: >= 0), -inf and negative gains do not; oblivious: any finite best"""
    L = _resolve_level(77)
    pv = np.full((3, 64), -np.inf, np.float32)
    pi = np.full((3, 64), S.NO_CAND, np.int32)
    pv[1, 9], pi[1, 9] = -0.0, 11
    pv[2, 63], pi[2, 63] = -2.0, 12
    for oblivious in (0, 1):
        if oblivious:
            pv[0, 5], pi[0, 5] = -3.0, 700
        o = S.probe(L, do_score=0, do_resolve=1, oblivious=oblivious, parts=(pv, pi, None, None), seg_start=[0, 10, 20])
        assert o.rc == 0, o.error
        R = S.expected_resolve(L, pv, pi, None, None, oblivious=oblivious, near=0, seg_start=[0, 10, 20])
        _check_resolve(o, R)
        if oblivious:
            assert o.splits[:, 0].tolist() == [1, 1, 1] and o.best_idx[0] == 700
        else:
            assert o.best_idx.tolist() == [0, 11, 12] and o.splits[:, 0].tolist() == [0, 1, 0] and S.bits(o.best_score)[1] == S.bits(np.array([-0.0], np.float32))[0]
            j0 = int(L.ref_to_internal[0])                                                                 # no winner: reference index 0, described but not split
            cat0, _, base0 = (int(x) for x in L.slots[L.cand_slot[j0], :3])
            assert o.best_score[0] == -np.inf and o.splits[0, 1:4].tolist() == [int(L.cand_slot[j0]), j0 - base0 + cat0, cat0]
