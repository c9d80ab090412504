"""The split-score histograms cell by cell: every kernel instantiation the route of step_hist_build.hip can choose (tests/hist_cases.py), and
the reduce of step_hist_reduce.hip in both variants and all three output layouts, against np.add.at in int64.  The sums are integers: every
comparison is exact, and a cell that no kernel stored must still hold the caller's sentinel.

One gbrl_hip_hist_probe call per case.  Its nodes carry the chunk lengths at which the kernels' loops can go wrong, derived from the
S = 1024 / FG row slots of a block and the U rows a slot keeps in flight (step = S * U rows per main-loop iteration):
1, S - 1, S, S + 1, step - 1, step, step + 1, 2 step - 1, 2 step + 1 and 3 step + S + 1 (three pipeline stages, the unrolled remainder and a
tail), a node without rows, a node of three equal chunks, a node that is one row many times, and len = 0 entries behind the table.  The row
list is drawn with replacement (rows repeat) and every third feature slot uses three classes only (the others stay empty).  At FG = 1 the
longest length needs a row list of 13 313 entries; every other case keeps it at 8192."""
import numpy as np
import pytest

import hist_cases as H

pytestmark = pytest.mark.gpu


def _edge_nodes(case):
    S = H.THREADS // case.FG
    step = S * H.unroll(case.kind, case.param)
    lens = [1, S - 1, S, S + 1, step - 1, step, step + 1, 2 * step - 1, 2 * step + 1, 3 * step + S + 1]
    nodes = [[n] for n in lens if n > 0]
    nodes.insert(4, [])                       # no rows, no chunk: the reduce writes zeros
    nodes.append([S + 3] * 3)                 # three equal chunks
    nodes.append([2 * S + 5])                 # ONE row, 2 S + 5 times (below)
    nodes.append([])
    return nodes


def _check(c, case, *, direct=0):
    ref = H.reference(c)
    rc, got, ran, wrote = H.probe(c)
    assert rc == 0, H.lib().gbrl_hip_last_error()
    meant = (case.kind, case.param, int(case.pipe), int(bool(c.count_rows)))          # kind, parameter, PIPE form, COUNT form
    assert (ran, wrote) == (meant, direct), "launched %s%s direct=%d, meant %s%s direct=%d" % (H.KIND_NAMES.get(ran[0]), ran[1:], wrote, H.KIND_NAMES[meant[0]], meant[1:], direct)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError("%s: %d of %d cells differ; first (index: got, expected): %s" % (
            case.name, len(bad), ref.size, [(tuple(int(x) for x in i), int(got[tuple(i)]), int(ref[tuple(i)])) for i in bad[:8]]))
    return ref


@pytest.mark.parametrize("case", H.CASES, ids=[c.name for c in H.CASES])
def test_every_instantiation_cell_by_cell(case):
    nodes = _edge_nodes(case)
    c = H.make_call(case, nodes, seed=len(case.name) * 131 + case.D, trailing=3)
    k = len(nodes) - 2
    s, n = int(c.chunks[c.chunks[:, 0] == k][0, 1]), 2 * (H.THREADS // case.FG) + 5
    c.rows[s:s + n] = c.rows[s]
    assert c.n_rows <= 10000 and (c.m == 8192 or case.FG == 1)
    ref = _check(c, case)
    assert np.all(ref[4] == 0) and np.all(ref[-1] == 0)                          # the nodes without rows
    assert not case.count_rows or np.any(ref[10, ..., case.D] == 0)               # classes that stay empty in the longest node


# ------------------------------------------------------------------------------------------------------------ HistDirect

def _direct_cap(D):
    return min(8192, max(1024, 9216 // (D + 1)))       # the engine's bound on the rows one block walks alone (engine_grow_levels.hip)


@pytest.mark.parametrize("name", ["fixed-D1-pipe", "fixed-D3-pipe", "fixed-D8-pipe", "fixed-D8-nopipe", "fixed-D16-pipe", "generic-FG16-D5", "generic-FG16-D16",
                                  "generic-FG2-D3", "generic-FG2-D2-odd", "generic-FG1-D4-odd"])
def test_direct_store(name):
    """every node ONE chunk, the block stores the node's int64 histogram: nodes of 0 rows (zeros must be written), 1 row, the engine's direct_cap
    and a length in between; a slot_map that permutes and leaves holes, which keep the sentinel"""
    case = H.BY_NAME[name]
    cap = _direct_cap(case.D)
    c = H.make_call(case, [[0], [1], [cap], [cap // 2 + 3], [0]], seed=7 + case.D, mode=1, n_hist_slots=7, slot_map=[5, 0, 3, 6, 2])
    ref = _check(c, case, direct=1)
    assert np.all(ref[[1, 4]] == H.SENTINEL) and np.all(ref[[5, 2]] == 0) and ref[3, ..., case.D].sum() == cap * c.padded()


# ------------------------------------------------------------------------------------------------------------ count-less build + root_le

def _root_call(case, B, chunks_per_slot, count_rows, n=8000, root_F=13):
    """The root of a numeric tree: every row once, in 8 chunks.  Features below root_F are binned from columns with repeating thresholds
    (constant, two-valued, five-valued, hundred-valued, continuous): code = first threshold >= value, le[c] = #{values <= threshold c}."""
    rng = np.random.default_rng(B * 7 + case.D)
    c = H.make_call(case, [[n // 8] * 8], seed=B + case.D, n_rows=n, m=n, chunks_per_slot=chunks_per_slot, count_rows=count_rows)
    c.rows[:] = rng.permutation(n)
    c.chunks[:, 1] = np.arange(8) * (n // 8)
    le = np.zeros((root_F, B), np.uint32)
    for f in range(root_F):
        x = [np.full(n, 3.5), rng.integers(0, 2, n) * 2.0, rng.integers(0, 5, n) * 1.0, rng.integers(0, 100, n) * 0.5, rng.normal(size=n)][f % 5]
        thr = np.quantile(x, (np.arange(B) + 1.0) / (B + 1), method="lower")
        c.codes[f >> 4, :, f & 15] = np.searchsorted(thr, x, side="left")
        le[f] = np.searchsorted(np.sort(x), thr, side="right")
    c.root_le, c.root_F, c.root_B, c.root_n = le, root_F, B, n
    return c


@pytest.mark.parametrize("chunks_per_slot", [8, 48])
@pytest.mark.parametrize("name", ["fixed-D1-countless", "fixed-D8-countless", "fixed-D16-countless"])
def test_countless_build_and_root_counts(name, chunks_per_slot):
    """k_hist_build<COUNT = false> accumulates no count; hist_reduce writes le[c] - le[c-1] (class B: n - le[B-1]) for the features below root_F.
    Features from root_F on have no ranks: their count field is what was accumulated -- nothing."""
    case = H.BY_NAME[name]
    c = _root_call(case, case.NB - 1, chunks_per_slot, False)
    ref = _check(c, case)
    c.root_le, c.count_rows = None, True                     # the construction itself: the ranks give the counts that accumulation gives
    acc = H.reference(c)
    assert np.array_equal(ref[:, :13], acc[:, :13]) and np.all(ref[:, 13:, :, case.D] == 0) and np.array_equal(ref[..., :case.D], acc[..., :case.D])
    assert np.any(acc[0, :13, :, case.D] == 0) and acc[0, 0, :, case.D].max() == 8000


@pytest.mark.parametrize("B", [31, 29])
def test_root_counts_replace_accumulated_counts(B):
    """root_le given to a build that DID count: below root_F the ranks win (they are halved here, so the two differ), from root_F on the accumulated
    counts stay.  B = n_classes - 3: the classes past B hold no numeric rows, their count is 0."""
    case = H.BY_NAME["fixed-D8-pipe"]
    c = _root_call(case, B, 8, True)
    c.codes[:] = np.minimum(c.codes, B)
    c.root_le = c.root_le // 2
    ref = _check(c, case)
    c.root_le = None
    acc = H.reference(c)
    assert not np.array_equal(ref[:, :13, :, 8], acc[:, :13, :, 8]) and np.array_equal(ref[:, 13:], acc[:, 13:]) and np.all(ref[:, :13, B + 1:, 8] == 0)


# ------------------------------------------------------------------------------------------------------------ hist_reduce

@pytest.mark.parametrize("layout", ["nodes", "slot_map", "scatter-divides", "scatter-remainder"])
@pytest.mark.parametrize("chunks_per_slot", [1, 48])
@pytest.mark.parametrize("name", ["fixed-D3-pipe", "wide-H10-D18"])
def test_reduce_variants_and_layouts(name, chunks_per_slot, layout):
    """k_hist_reduce<1> and <4> (one and four threads per element) over nodes of 1, 3, 4, 5, 31, 32, 33 and 67 chunks -- the 8-way, 4-way and
    single steps of both -- and none; FG = 16 (stores through the LDS tile) and FG = 8 (plain stores); node slots, a slot_map with holes, and the
    reduce-scatter send layout with a slice width that divides the padded feature count and one that does not"""
    case = H.BY_NAME[name]
    rng = np.random.default_rng(chunks_per_slot + len(layout))
    counts = [1, 3, 4, 5, 0, 31, 32, 33, 67]
    nodes = [[int(x) for x in rng.integers(1, 24, size=k)] for k in counts]
    Fp = -(-case.n_fslots // case.FG) * case.FG
    kw = {"nodes": {}, "slot_map": dict(n_hist_slots=12, slot_map=[7, 0, 11, 3, 4, 9, 1, 5, 10]),
          "scatter-divides": dict(scatter_fs=8), "scatter-remainder": dict(scatter_fs=5 if Fp == 32 else 12)}[layout]
    fs = kw.get("scatter_fs", 0)
    assert (layout != "scatter-divides" or Fp % fs == 0) and (layout != "scatter-remainder" or Fp % fs != 0)
    c = H.make_call(case, nodes, seed=chunks_per_slot, chunks_per_slot=chunks_per_slot, trailing=5, **kw)
    ref = _check(c, case)
    if layout == "slot_map":
        assert np.all(ref[[2, 6, 8]] == H.SENTINEL) and np.all(ref[4] == 0)
    if layout == "scatter-remainder":
        assert np.all(ref[-1, :, Fp % c.scatter_fs:] == H.SENTINEL) and np.all(ref[-1, :, : Fp % c.scatter_fs] != H.SENTINEL)


# ------------------------------------------------------------------------------------------------------------ the wrap claim

@pytest.mark.parametrize("name", ["fixed-D2-pipe", "fixed-D2-nopipe", "fixed-D2-countless", "wide-H10-D18", "quad-R9-D35", "generic-FG16-D5", "generic-FG4-D64"])
def test_wrapped_int32_sums_are_exact(name):
    """'Integer adds wrap mod 2^32 ... the wrapped result exact' (k_hist_build): one class of one chunk receives 1024 rows of +3 * 2^20 and then
    1024 of -3 * 2^20 in output 0, and the opposite signs in output 1.  A row slot walks its positions in ascending order, so every slot adds all
    rows of the first sign before any of the second: the running sums pass 3 * 2^30 and -3 * 2^30 unless the waves of a block drift apart by
    whole passes over the chunk, and come back to 0.  Then chunks whose sums are exactly 2^31 - 1 and -2^31, and 64 such chunks in one node,
    whose sum needs int64."""
    case = H.BY_NAME[name]
    c = H.make_call(case, [[2048], [1024], [1] * 64], seed=3, n_rows=3072, m=3072, qmax=1000)
    c.rows[:] = np.arange(3072)
    c.chunks[:, 1] = [0, 2048] + [2048] * 64               # the 64 chunks of node 2 are 64 times the rows of node 1
    c.chunks[:, 2] = [2048, 1024] + [1024] * 64
    c.codes[:, :2048] = 1
    c.codes[:, 2048:] = 2
    big = np.repeat(np.array([3 << 20, -(3 << 20)], np.int32), 1024)          # positions 0..1023 all +, 1024..2047 all -: no shuffle
    c.qg[:2048, 0] = big
    c.qg[:2048, 1] = -big
    run = np.cumsum(c.qg[c.rows[:2048], :2].astype(np.int64), axis=0)           # the sums in list order: past +-2^31, back to 0
    assert run[:, 0].max() == 3 << 30 > (1 << 31) and run[:, 1].min() == -(3 << 30) < -(1 << 31) and not run[-1].any()
    S = H.THREADS // case.FG
    for s in (0, 1, S - 1):                                                      # and slot by slot: first sign first (1024 is a multiple of S)
        assert np.all(np.diff(np.sign(c.qg[c.rows[s:2048:S], 0])) <= 0)
    c.qg[2048:, 0] = 1 << 21
    c.qg[3071, 0] = (1 << 21) - 1
    c.qg[2048:, 1] = -(1 << 21)
    ref = _check(c, case)
    n = 1 if case.count_rows else 0
    assert ref[0, 0, 1, 0] == 0 and ref[0, 0, 1, 1] == 0 and ref[0, 0, 1, case.D] == 2048 * n
    assert ref[1, 0, 2, 0] == (1 << 31) - 1 and ref[1, 0, 2, 1] == -(1 << 31)
    assert ref[2, 0, 2, 0] == 64 * ((1 << 31) - 1) and ref[2, 0, 2, 1] == -(1 << 37) and ref[2, 0, 2, case.D] == 65536 * n
