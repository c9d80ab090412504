"""The inputs, the NumPy references and the entry point shared by tests/test_rows_host.py (CPU: the refusals of gbrl_hip_rows_probe, the references
themselves) and tests/test_gpu_rows_cells.py (the kernels of step_partition.hip: k_partition, k_count_right, k_leaf_sums).  Everything is an
integer or an exactly rounded product by a power of two: every comparison is exact."""
import ctypes
import os

import numpy as np

PARTITION, COUNT_RIGHT, LEAF_SUMS = 0, 1, 2
SENT32 = 0x5a5a5a5b
E_INVALID = -1
PART_ROWS = 4096                        # kPartRows: rows per partition block
N_FSLOTS = 20                           # two code groups of 16: slots 16.. live in the second
N_CODES = 8


class RowsArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("rows", "chunks", "splits", "codes", "kt", "grads", "rows_out", "cursors", "acc")] + \
               [(n, ctypes.c_int) for n in ("op", "n_rows", "m", "n_chunks", "n_slots", "n_feature_slots", "output_dim", "lbits")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        import gbrl_amd
        so = ctypes.CDLL(os.path.join(os.path.dirname(gbrl_amd.__file__), "libgbrl_hip.so"))
        so.gbrl_hip_rows_probe.restype = ctypes.c_int
        so.gbrl_hip_rows_probe.argtypes = [ctypes.POINTER(RowsArgs)]
        so.gbrl_hip_last_error.restype = ctypes.c_char_p
        _lib = so
    return _lib


class Call:
    pass


def make_table(seed, n_rows=6000):
    """codes [2][n_rows][16] in [0, 8) and feature-major keys [20][n_rows] drawn INDEPENDENTLY of the codes, so that a kernel that reads the wrong
    one of the two shows; slot 19 holds one code only (a categorical split can send every row right)"""
    rng = np.random.default_rng(seed)
    c = Call()
    c.n_rows = n_rows
    c.codes = rng.integers(0, N_CODES, size=(2, n_rows, 16)).astype(np.uint16)
    c.codes[1, :, 3] = 5
    c.kt = rng.integers(1, 1 << 32, size=(N_FSLOTS, n_rows), dtype=np.uint64).astype(np.uint32)
    c.use_kt = True
    return c


def goes_right(c, split, rows):
    """the predicate of k_partition and k_count_right for one NodeSplit (do_split, fslot, bin, is_cat, seg_start, n_left, thr_key, 0)"""
    f, b, is_cat = int(split[1]), int(split[2]), int(split[3])
    if not is_cat and c.use_kt:
        return c.kt[f, rows] > np.uint32(int(split[6]) & 0xffffffff)
    code = c.codes[f >> 4, rows, f & 15].astype(np.int64)
    return code == b if is_cat else code > b


def add_splits(c, rng, nodes):
    """nodes: (chunk lengths, kind, fslot) with kind "num", "cat", "num-left", "num-right", "cat-left", "cat-right" or "leaf" (do_split = 0).  The
    row list holds the nodes' segments one behind the other, each cut into its chunks; two len = 0 entries follow."""
    c.rows = rng.integers(0, c.n_rows, size=sum(sum(n[0]) for n in nodes)).astype(np.int32)
    c.splits = np.zeros((len(nodes), 8), np.int32)
    chunks, start = [], 0
    for k, (lens, kind, f) in enumerate(nodes):
        seg = c.rows[start:start + sum(lens)]
        sp = c.splits[k]
        sp[0], sp[1], sp[3], sp[4] = kind != "leaf", f, kind.startswith("cat"), start
        if kind in ("num", "leaf"):
            mid = seg[np.abs(c.codes[f >> 4, seg, f & 15].astype(np.int64) - 3) <= 1]             # a row of the node with a code in the middle:
            pick = int(mid[len(mid) // 2]) if len(mid) else int(seg[len(seg) // 2]) if len(seg) else 0      # its key IS the threshold, its code the bin
            sp[2], key = c.codes[f >> 4, pick, f & 15], c.kt[f, pick]
        elif kind == "cat":
            sp[2], key = c.codes[f >> 4, int(seg[0]), f & 15], 0
        else:
            sp[2], key = {"num-left": (N_CODES - 1, 0xffffffff), "num-right": (-1, 0), "cat-left": (100, 0), "cat-right": (5, 0)}[kind]
        sp[6] = np.array([key], np.uint32).view(np.int32)[0]
        sp[5] = int((~goes_right(c, sp, seg)).sum())
        for n in lens:
            chunks.append((k, start, n))
            start += n
    c.chunks = np.array(chunks + [(0, 0, 0), (len(nodes) - 1, start, 0)], np.int32)
    c.n_slots = len(nodes)
    return c


def reference_partition(c):
    """-> per node None (nothing written) or (sorted left rows, sorted right rows), and the cursors as they must end"""
    out, cur = [], start_cursors(c)
    for k in range(c.n_slots):
        sp = c.splits[k]
        seg = np.concatenate([c.rows[s:s + n] for (slot, s, n) in c.chunks if slot == k] + [np.zeros(0, np.int32)])
        if not sp[0] or len(seg) == 0:
            out.append(None)
            continue
        r = goes_right(c, sp, seg)
        out.append((np.sort(seg[~r]), np.sort(seg[r])))
        cur[k] = (int((~r).sum()), int(r.sum()))
    return out, cur


def reference_count_right(c, acc0):
    acc = np.array(acc0, np.int64)
    for (slot, s, n) in c.chunks:
        acc[slot] += int(goes_right(c, c.splits[slot], c.rows[s:s + n]).sum())
    return acc


def reference_leaf_sums(c, acc0):
    """np.rint(g * 2^lbits) in float64 -- exact: a power-of-two scale, ties to even -- summed in int64; field D counts the rows"""
    q = np.rint(c.grads.astype(np.float64) * 2.0 ** c.lbits).astype(np.int64)
    acc = np.array(acc0, np.int64)
    for (slot, s, n) in c.chunks:
        acc[slot, :c.D] += q[c.rows[s:s + n]].sum(axis=0)
        acc[slot, c.D] += n
    return acc


def probe(c, op, *, rows_out=None, cursors=None, acc=None, overrides=None, drop=()):
    """one gbrl_hip_rows_probe call -> (rc, error text); rows_out / cursors / acc are changed in place"""
    keep = [np.ascontiguousarray(c.rows, np.int32), np.ascontiguousarray(c.chunks, np.int32)]
    a = RowsArgs()
    a.rows, a.chunks = (x.ctypes.data for x in keep)
    a.op, a.n_rows, a.m, a.n_chunks, a.n_slots = op, c.n_rows, len(c.rows), len(c.chunks), c.n_slots
    if op != LEAF_SUMS:
        keep += [np.ascontiguousarray(c.splits, np.int32), np.ascontiguousarray(c.codes, np.uint16), np.ascontiguousarray(c.kt, np.uint32)]
        a.splits, a.codes, a.n_feature_slots = keep[-3].ctypes.data, keep[-2].ctypes.data, N_FSLOTS
        a.kt = keep[-1].ctypes.data if c.use_kt else None
    else:
        keep.append(np.ascontiguousarray(c.grads, np.float32))
        a.grads, a.output_dim, a.lbits = keep[-1].ctypes.data, c.D, c.lbits
    for name, arr, dt in (("rows_out", rows_out, np.int32), ("cursors", cursors, np.int32), ("acc", acc, np.int64)):
        if arr is not None:
            assert arr.dtype == dt and arr.flags.c_contiguous
            setattr(a, name, arr.ctypes.data)
    for n in drop:
        setattr(a, n, None)
    for n, v in (overrides or {}).items():
        setattr(a, n, v)
    rc = lib().gbrl_hip_rows_probe(ctypes.byref(a))
    err = (lib().gbrl_hip_last_error() or b"").decode() if rc != 0 else ""
    if rc not in (0, E_INVALID):                               # a device error: nothing more is started on a device that may have faulted
        import pytest
        pytest.exit("gbrl_hip_rows_probe failed on the device: " + err, returncode=3)
    return rc, err


def start_cursors(c):
    """0 for the nodes that split (the kernel adds to them), the sentinel elsewhere"""
    cur = np.full((c.n_slots, 2), SENT32, np.int32)
    cur[c.splits[:, 0] != 0] = 0
    return cur
