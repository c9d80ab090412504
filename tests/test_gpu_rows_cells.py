"""The row kernels of step_partition.hip cell by cell through gbrl_hip_rows_probe: k_partition (destination slots by ballot, an LDS scan and one
atomic per side), k_count_right and k_leaf_sums (atomics into caller-owned words).  All comparisons are exact; a cell no kernel stored must still
hold the caller's sentinel.  The references and the inputs are in tests/rows_cases.py."""
import numpy as np
import pytest

import rows_cases as R

pytestmark = pytest.mark.gpu

EDGE_LENS = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096]


def _check_partition(c):
    want, cur_want = R.reference_partition(c)
    out, cur = np.full(len(c.rows), R.SENT32, np.int32), R.start_cursors(c)
    rc, err = R.probe(c, R.PARTITION, rows_out=out, cursors=cur)
    assert rc == 0, err
    untouched = np.ones(len(out), bool)
    for k, w in enumerate(want):
        if w is None:
            continue
        s, nl, n = int(c.splits[k, 4]), len(w[0]), len(w[0]) + len(w[1])
        assert np.array_equal(np.sort(out[s:s + nl]), w[0]), "node %d: the left range does not hold the node's left rows" % k
        assert np.array_equal(np.sort(out[s + nl:s + n]), w[1]), "node %d: the right range does not hold the node's right rows" % k
        untouched[s:s + n] = False
    assert np.all(out[untouched] == R.SENT32), "a position outside every splitting node's segment was written"
    assert np.array_equal(cur, cur_want), (cur.tolist(), cur_want.tolist())
    return want


@pytest.mark.parametrize("kind,kt", [("num", True), ("num", False), ("cat", True), ("cat", False)], ids=["numeric-keys", "numeric-codes", "categorical-keys-given", "categorical"])
def test_partition_chunk_lengths(kind, kt):
    """one node per chunk length 1 .. 4096, a node of three full chunks plus one row, a node that stays a leaf and len = 0 entries; feature slots
    in both code groups; the threshold is a row's own key (or code): keys equal to thr_key and codes equal to bin are met.  With kt given the keys
    disagree with the codes on purpose, so that the source a numeric split reads is visible; a categorical one reads the codes either way."""
    c = R.make_table(17)
    c.use_kt = kt
    nodes = [([n], kind, 17 if i % 2 else 3) for i, n in enumerate(EDGE_LENS)]
    nodes.insert(4, ([700], "leaf", 2))
    nodes.append(([R.PART_ROWS] * 3 + [1], kind, 18))
    R.add_splits(c, np.random.default_rng(5), nodes)
    for k in (3, 9, 10):                                               # the inputs reach what they are meant to reach
        sp, seg = c.splits[k], c.rows[c.splits[k, 4]:c.splits[k, 4] + sum(nodes[k][0])]
        if kind == "num" and kt:
            keys, codes = c.kt[sp[1], seg], c.codes[sp[1] >> 4, seg, sp[1] & 15]
            assert np.any(keys == np.uint32(int(sp[6]) & 0xffffffff)) and np.any((keys > np.uint32(int(sp[6]) & 0xffffffff)) != (codes > sp[2]))
        else:
            assert np.any(c.codes[sp[1] >> 4, seg, sp[1] & 15] == sp[2])
    want = _check_partition(c)
    assert want[4] is None and all(len(w[0]) and len(w[1]) for w in want[6:] if w is not None) and len(want[-1][0]) + len(want[-1][1]) == 3 * R.PART_ROWS + 1


def test_partition_one_sided_splits():
    """all rows left and all rows right, numeric by keys and categorical; and the same numeric splits by codes"""
    for kt in (True, False):
        c = R.make_table(23)
        c.use_kt = kt
        nodes = [([1025], "num-left", 3), ([R.PART_ROWS, 65], "num-right", 17), ([64], "cat-left", 5), ([1023, 1], "cat-right", 19), ([0], "num", 1), ([100], "num", 16)]
        R.add_splits(c, np.random.default_rng(7), nodes)
        want = _check_partition(c)
        assert [len(w[1]) if i % 2 == 0 else len(w[0]) for i, w in enumerate(want[:4])] == [0, 0, 0, 0] and want[4] is None


def test_count_right():
    """the same predicates; chunk lengths 0, 1, 1023, 1024, 1025 and 5000 and several chunks per slot; on top of non-zero caller values"""
    for kt in (True, False):
        c = R.make_table(29)
        c.use_kt = kt
        nodes = [([0], "num", 3), ([1], "num", 3), ([1023], "cat", 17), ([1024], "num", 18), ([1025], "cat", 4), ([5000], "num", 17), ([5000, 0, 1, 1024], "num", 2),
                 ([300], "num-left", 3), ([300], "cat-left", 7), ([77], "leaf", 6)]
        R.add_splits(c, np.random.default_rng(11), nodes)
        acc0 = np.array([5, -3, 1 << 40, 0, 7, -(1 << 33), 11, 123456789, -1, 9], np.int64)
        acc = acc0.copy()
        rc, err = R.probe(c, R.COUNT_RIGHT, acc=acc)
        assert rc == 0, err
        want = R.reference_count_right(c, acc0)
        assert np.array_equal(acc, want), (acc.tolist(), want.tolist())
        assert want[7] == acc0[7] and want[8] == acc0[8] and want[0] == acc0[0] and want[5] - acc0[5] > 100 and want[9] != acc0[9]     # (a leaf's slot is counted too)


@pytest.mark.parametrize("D", [1, 3, 7, 64, 100, 128, 200, 256, 257, 320, 512])
def test_leaf_sums(D):
    """a block keeps per = 256 / D rows in flight, eight deep: lengths 1, per - 1, per, 8 per - 1, 8 per, 8 per + 1 and 16 per + 3, an empty chunk and
    a slot of several chunks; on top of caller values of both signs; gradients of both signs, some of them exact ties of the rounding.  From 257
    outputs on a thread owns several fields: the kernel is bounded at 256 threads."""
    per = max(1, 256 // D)
    lens = sorted({n for n in (1, per - 1, per, 8 * per - 1, 8 * per, 8 * per + 1, 16 * per + 3) if n > 0})
    rng = np.random.default_rng(D)
    c = R.Call()
    c.n_rows, c.D, c.lbits = 700, D, 20
    c.grads = (rng.standard_normal((c.n_rows, D)) * 10.0 ** rng.integers(-3, 3, size=(c.n_rows, 1))).astype(np.float32)
    ties = rng.random((c.n_rows, D)) < 0.05
    c.grads[ties] = ((2 * rng.integers(-5000, 5000, size=int(ties.sum())) + 1) * 2.0 ** -21).astype(np.float32)           # x.5 after the scale
    chunk_lens = [[n] for n in lens] + [[0], [per + 1, 8 * per, 3]]
    c.n_slots = len(chunk_lens) + 1                                    # the last slot has no chunk
    c.rows = rng.integers(0, c.n_rows, size=sum(sum(n) for n in chunk_lens)).astype(np.int32)
    chunks, start = [], 0
    for k, ns in enumerate(chunk_lens):
        for n in ns:
            chunks.append((k, start, n))
            start += n
    c.chunks = np.array(chunks, np.int32)
    q = np.rint(c.grads.astype(np.float64) * 2.0 ** 20)
    assert np.any(np.abs(c.grads.astype(np.float64) * 2.0 ** 20 % 1) == 0.5) and q.min() < 0 < q.max()
    acc0 = rng.integers(-(1 << 40), 1 << 40, size=(c.n_slots, D + 1))
    acc = acc0.copy()
    rc, err = R.probe(c, R.LEAF_SUMS, acc=acc)
    assert rc == 0, err
    want = R.reference_leaf_sums(c, acc0)
    bad = np.argwhere(acc != want)
    assert len(bad) == 0, "%d of %d cells differ; first (slot, field: got, expected): %s" % (len(bad), want.size, [(tuple(i), acc[tuple(i)], want[tuple(i)]) for i in bad[:6]])
    assert np.array_equal(want[-1], acc0[-1]) and np.array_equal(want[-2, :D] - acc0[-2, :D], q[c.rows[start - (9 * per + 4):start]].sum(axis=0).astype(np.int64))
