"""The host side of gbrl_hip_rows_probe, without a device: the symbol, the refusals -- among them a NodeSplit whose n_left is not the count the
host finds itself, which would send destinations outside the node's segment --, and the references of tests/rows_cases.py counted by hand."""
import numpy as np

import rows_cases as R


def _call(kt=True):
    c = R.make_table(3, n_rows=200)
    c.use_kt = kt
    return R.add_splits(c, np.random.default_rng(3), [([30, 10], "num", 3), ([25], "cat", 17), ([7], "leaf", 0), ([20], "num", 18)])


def _refused(c, text, op=R.PARTITION, **kw):
    out, cur, acc = np.full(len(c.rows), R.SENT32, np.int32), R.start_cursors(c) if op == R.PARTITION else None, np.zeros(c.n_slots * 600, np.int64)
    rc, err = R.probe(c, op, rows_out=out if op == R.PARTITION else None, cursors=kw.pop("cursors", cur), acc=None if op == R.PARTITION else acc, **kw)
    assert np.all(out == R.SENT32) and not acc.any(), "a refused call must not touch its arrays"
    return rc == R.E_INVALID and text in err


def _leaf_call():
    c = R.Call()
    c.n_rows, c.D, c.lbits, c.n_slots = 4, 2, 1, 2
    c.grads = np.array([[0.25, -0.25], [0.75, 1.0], [-1.25, 3.0], [100.0, 0.5]], np.float32)
    c.rows = np.array([0, 1, 2, 2, 1], np.int32)
    c.chunks = np.array([(1, 0, 3), (0, 3, 0), (1, 3, 2)], np.int32)
    return c


def test_the_symbol_is_exported():
    assert R.lib().gbrl_hip_rows_probe
    assert R.lib().gbrl_hip_rows_probe(None) == R.E_INVALID


def test_refusals_on_the_host():
    assert _refused(_call(), "op must be", overrides={"op": 3})
    for name in ("rows", "chunks", "splits", "codes", "rows_out", "cursors"):
        assert _refused(_call(), "null array", drop=(name,)), name
    assert _refused(_call(), "null array", op=R.COUNT_RIGHT, drop=("acc",)) and _refused(_leaf_call(), "null array", op=R.LEAF_SUMS, drop=("grads",))
    for field, value in (("n_rows", 0), ("m", 0), ("n_chunks", 0), ("n_slots", 0), ("n_feature_slots", 0), ("n_feature_slots", 5000)):
        assert _refused(_call(), "a size is out of range", overrides={field: value}), (field, value)
    for field, value in (("output_dim", 0), ("output_dim", 513), ("lbits", -1), ("lbits", 41)):
        assert _refused(_leaf_call(), "a size is out of range", op=R.LEAF_SUMS, overrides={field: value}), (field, value)
    for value in (-1, 200):
        c = _call()
        c.rows[11] = value
        assert _refused(c, "a row index is outside"), value
    for chunk in ((4, 0, 5), (-1, 0, 5), (0, -1, 5), (0, 90, 3), (0, 0, -1), (0, 93, 0)):
        c = _call()
        c.chunks[1] = chunk
        assert _refused(c, "a chunk lies outside"), chunk
        assert _refused(c, "a chunk lies outside", op=R.COUNT_RIGHT)
    c = _call()
    c.rows = np.concatenate([c.rows, np.zeros(5000, np.int32)])
    c.chunks[4] = (2, 92, 4097)                                    # (the leaf: only the chunk's length is wrong)
    assert _refused(c, "more than 4096 rows") and not _refused(c, "more than 4096 rows", op=R.COUNT_RIGHT, overrides={"n_rows": 0})
    for value in (-1, R.N_FSLOTS):
        c = _call()
        c.splits[2, 1] = value                                     # (checked for a node that does not split too: k_count_right reads every slot's split)
        assert _refused(c, "a split names a feature slot outside") and _refused(c, "a split names a feature slot outside", op=R.COUNT_RIGHT), value
    # the destinations of the partition
    for delta in (1, -1):
        for kt in (True, False):
            c = _call(kt)
            c.splits[3, 5] += delta
            assert _refused(c, "n_left is not the number of rows the split sends left"), (delta, kt)
    c = _call()
    c.splits[3, 6] = -1                                            # the highest threshold key: every row goes left now, the descriptor's count stays
    assert _refused(c, "n_left is not") and not _refused(_call(False), "n_left is not", overrides={"op": 3})
    c = _call()
    c.splits[1, 4] = 39                                            # node 1's segment would begin inside node 0's
    assert _refused(c, "the segments of two splitting nodes overlap")
    c = _call()
    c.splits[3, 4] = 73                                            # 20 rows from 73 in a list of 92
    assert _refused(c, "a segment lies outside the row list")
    c = _call()
    cur = R.start_cursors(c)
    cur[1, 1] = 2
    assert _refused(c, "must start at 0", cursors=cur)
    c = _call()
    c.splits[2, 4], c.splits[2, 5] = 10, 99                        # a node that does not split may say anything
    out, cur = np.full(len(c.rows), R.SENT32, np.int32), R.start_cursors(c)
    assert R.probe(c, R.PARTITION, rows_out=out, cursors=cur, overrides={"op": 3})[1].startswith("rows_probe: op must be")


def test_the_references_on_cases_small_enough_to_count_by_hand():
    c = R.Call()
    c.n_rows, c.use_kt, c.n_slots = 4, True, 2
    c.codes = np.zeros((2, 4, 16), np.uint16)
    c.codes[0, :, 2] = (0, 3, 5, 3)
    c.codes[1, :, 1] = (1, 1, 2, 0)
    c.kt = np.zeros((R.N_FSLOTS, 4), np.uint32)
    c.kt[2] = (10, 20, 30, 40)
    c.rows = np.array([0, 1, 2, 3, 3, 2, 2], np.int32)
    c.chunks = np.array([(0, 0, 3), (0, 3, 1), (1, 4, 3)], np.int32)
    c.splits = np.array([(1, 2, 0, 0, 0, 2, 20, 0), (1, 17, 2, 1, 4, 1, 0, 0)], np.int32)     # keys > 20: rows 2, 3 (the codes would say 1, 2, 3); code == 2: row 2
    parts, cur = R.reference_partition(c)
    assert [p.tolist() for p in parts[0]] == [[0, 1], [2, 3]] and [p.tolist() for p in parts[1]] == [[3], [2, 2]] and cur.tolist() == [[2, 2], [1, 2]]
    assert R.reference_count_right(c, [100, -5]).tolist() == [102, -3]
    c.use_kt = False                                               # by codes: code > 0
    assert [p.tolist() for p in R.reference_partition(c)[0][0]] == [[0], [1, 2, 3]] and R.reference_count_right(c, [0, 0]).tolist() == [3, 2]
    c = _leaf_call()                                               # scale 2: 0.25 -> 0.5 -> 0 and 0.75 -> 1.5 -> 2 (ties to even), -1.25 -> -2.5 -> -2
    want = [[7, 0, 0], [0 + 2 - 2 - 2 + 2 - 100, 0 + 2 + 6 + 6 + 2 + 1, 5 + 3]]
    assert R.reference_leaf_sums(c, [[7, 0, 0], [-100, 1, 3]]).tolist() == want
