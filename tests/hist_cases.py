"""The case table, the NumPy reference and the entry points shared by tests/test_hist_host.py (CPU: gbrl_hip_hist_plan, the refusals of
gbrl_hip_hist_probe) and tests/test_gpu_hist_cells.py (the kernels of step_hist_build.hip and step_hist_reduce.hip, cell by cell).

CASES holds one entry per kernel instantiation the route of step_hist_build.hip (hist_route) can choose: (n_classes, output_dim) pairs whose
features-per-block FG is the ENGINE'S OWN choice for that pair, so that a case is a shape a step can meet.  test_hist_host.py sweeps the route
and fails when it reaches an (FG, kind, param, pipe) that has no case here.

The sums are integers: the reference is np.add.at in int64 and every comparison is exact."""
import collections
import ctypes
import os

import numpy as np

GENERIC, FIXED_D, WIDE, QUAD = 0, 1, 2, 3
KIND_NAMES = {GENERIC: "generic", FIXED_D: "fixed", WIDE: "wide", QUAD: "quad"}
LDS_LIMIT = 160 * 1024 - 512            # the engine's limit for one block's LDS tile (kern::kHistLdsLimit)
THREADS = 1024                          # kHistThreads
HIST_U = 8                              # GBRL_HIST_U: rows in flight per row slot of k_hist_build<D>
SENTINEL = -0x5a5a5a5a5a5a5a5b          # what a cell that no kernel stored must still hold
E_INVALID = -1                          # GBRL_HIP_E_INVALID

# name; n_classes, output_dim; the FG, kind, param and pipe the probe must report; count_rows; hooks (environment); feature slots
Case = collections.namedtuple("Case", "name NB D FG kind param pipe count_rows env n_fslots")


def lds_bytes(NB, D, FG):
    return NB * (D + 1) * FG * 4


def feature_group(NB, D):
    """the engine's rule (kern::hist_feature_group), restated"""
    FG = 16
    while FG > 1 and lds_bytes(NB, D, FG) > LDS_LIMIT:
        FG //= 2
    while D > 16 and FG > 4 and (16 // FG) * 16 < D + 1:
        FG //= 2
    return FG


def route(D, FG, n_rows, generic=False, pipe=True):
    """hist_route, restated -> (kind, param, pipe, direct_ok, countless_ok)"""
    direct_ok = FG not in (8, 4)
    if generic or n_rows > (1 << 26):
        return GENERIC, 0, False, direct_ok, False
    if FG == 16 and 1 <= D <= 16:
        return FIXED_D, D, pipe, direct_ok, pipe
    if FG == 8 and D + 1 <= 32:
        return WIDE, (D + 2) // 2, False, direct_ok, False
    if FG == 4 and D + 1 <= 64:
        return QUAD, (D + 4) // 4, False, direct_ok, False
    return GENERIC, 0, False, direct_ok, False


def unroll(kind, param):
    """rows in flight per row slot of the kernel of a route"""
    if kind == FIXED_D:
        return HIST_U
    if kind == QUAD:
        return 4 if param <= 8 else 2
    return 4


def _smallest_nb(D, FG):
    """the smallest class count whose tile does not fit FG * 2 features (and fits FG)"""
    nb = LDS_LIMIT // (4 * (D + 1) * FG * 2) + 1
    assert lds_bytes(nb, D, FG) <= LDS_LIMIT < lds_bytes(nb, D, FG * 2)
    return nb


def _cases():
    out = []
    for D in range(1, 17):                                   # k_hist_build<D, 8, PIPE, HistLoads, COUNT>
        slots = 19 if D % 2 else 35
        out.append(Case(f"fixed-D{D}-pipe", 32, D, 16, FIXED_D, D, True, True, {}, slots))
        out.append(Case(f"fixed-D{D}-nopipe", 32, D, 16, FIXED_D, D, False, True, {"GBRL_HIP_HIST_PIPE": "0"}, slots))
        out.append(Case(f"fixed-D{D}-countless", 32, D, 16, FIXED_D, D, True, False, {}, slots))
    for H in range(1, 17):                                   # k_hist_build_wide<2, H, 4>: D = 2H - 2 and 2H - 1
        for D in sorted({max(1, 2 * H - 2), 2 * H - 1}):
            NB = _smallest_nb(D, 8) if D <= 16 else 24       # D <= 16 reaches FG 8 through the class count alone; D 17..31 through the D > 16 rule
            out.append(Case(f"wide-H{H}-D{D}", NB, D, 8, WIDE, H, False, True, {}, 19 if H % 2 else 35))
    for R in range(1, 17):                                   # k_hist_build_quad<R, R <= 8 ? 4 : 2>: D = 4R - 4 (the count opens a register) and 4R - 1
        for D in (max(1, 4 * R - 4), 4 * R - 1):
            NB = _smallest_nb(D, 4) if D <= 31 else 12
            out.append(Case(f"quad-R{R}-D{D}", NB, D, 4, QUAD, R, False, True, {}, 19 if R % 2 else 35))
    # the run-time-D kernel k_hist_build<0, 4, false>
    out.append(Case("generic-FG16-D5", 32, 5, 16, GENERIC, 0, False, True, {"GBRL_HIP_HIST_GENERIC": "1"}, 19))
    out.append(Case("generic-FG16-D16", 20, 16, 16, GENERIC, 0, False, True, {"GBRL_HIP_HIST_GENERIC": "1"}, 35))
    out.append(Case("generic-FG4-D64", 12, 64, 4, GENERIC, 0, False, True, {}, 19))
    out.append(Case("generic-FG4-D100", 9, 100, 4, GENERIC, 0, False, True, {}, 35))
    out.append(Case("generic-FG2-D3", _smallest_nb(3, 2), 3, 2, GENERIC, 0, False, True, {}, 19))            # n_acc % 4 == 0: 16-byte LDS clear and store
    out.append(Case("generic-FG2-D2-odd", _smallest_nb(2, 2), 2, 2, GENERIC, 0, False, True, {}, 19))        # n_acc % 4 == 2: the scalar clear and store
    out.append(Case("generic-FG1-D4", 4100, 4, 1, GENERIC, 0, False, True, {}, 19))                          # n_acc % 4 == 0
    out.append(Case("generic-FG1-D4-odd", 4099, 4, 1, GENERIC, 0, False, True, {}, 19))                      # n_acc % 4 == 3
    for c in out:
        assert feature_group(c.NB, c.D) == c.FG and lds_bytes(c.NB, c.D, c.FG) <= LDS_LIMIT, c
        assert route(c.D, c.FG, 10000, c.env.get("GBRL_HIP_HIST_GENERIC") == "1", c.env.get("GBRL_HIP_HIST_PIPE") != "0")[:3] == (c.kind, c.param, c.pipe), c
    assert (_smallest_nb(2, 2) * 3 * 2) % 4 == 2 and (_smallest_nb(3, 2) * 4 * 2) % 4 == 0
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------ entry points

class Plan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("fg", "kind", "param", "pipe", "direct_ok", "countless_ok")] + [("hist_lds_bytes", ctypes.c_size_t)]


class ProbeArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("codes", "qg", "rows", "chunks", "root_le", "slot_map", "hist")] + \
               [("hist_elems", ctypes.c_longlong), ("root_n", ctypes.c_longlong)] + \
               [(n, ctypes.c_int) for n in ("n_rows", "output_dim", "m", "n_chunks", "n_nodes", "n_feature_slots", "fg", "n_classes", "mode", "count_rows",
                                            "root_F", "root_B", "chunks_per_slot", "scatter_fs", "kind", "param", "pipe", "counted", "wrote_direct")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        import gbrl_amd
        so = ctypes.CDLL(os.path.join(os.path.dirname(gbrl_amd.__file__), "libgbrl_hip.so"))
        so.gbrl_hip_hist_plan.restype = ctypes.c_int
        so.gbrl_hip_hist_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Plan)]
        so.gbrl_hip_hist_probe.restype = ctypes.c_int
        so.gbrl_hip_hist_probe.argtypes = [ctypes.POINTER(ProbeArgs)]
        so.gbrl_hip_last_error.restype = ctypes.c_char_p
        _lib = so
    return _lib


def plan(NB, D, n_rows=10000, FG_in=0):
    """-> Plan, or None when gbrl_hip_hist_plan refuses the arguments"""
    p = Plan()
    rc = lib().gbrl_hip_hist_plan(NB, D, n_rows, FG_in, ctypes.byref(p))
    return p if rc == 0 else None


# ------------------------------------------------------------------------------------------------------------ inputs

class Call:
    """One probe call: the arrays, the chunk table and the switches.  `nodes` (make_call) is a list of chunk-length lists, one per node."""

    def padded(self):
        FG = self.FG if self.FG in (1, 2, 4, 8, 16) else 16          # (a refused FG: the arrays still need a shape)
        return -(-self.n_fslots // FG) * FG

    def hist_shape(self):
        Fp = self.padded()
        if self.scatter_fs:
            return (-(-Fp // self.scatter_fs), self.n_nodes, self.scatter_fs, self.NB, self.D + 1)
        return (self.n_hist_slots, Fp, self.NB, self.D + 1)


def make_codes(rng, n_rows, Fp, NB):
    """[ceil(Fp / 16)][n_rows][16] class codes.  Every third feature slot draws from a few classes only, so that most of its classes stay empty;
    the lanes behind Fp of the last group hold valid codes too."""
    G = -(-Fp // 16)
    codes = rng.integers(0, NB, size=(G, n_rows, 16), dtype=np.int64)
    for f in range(0, G * 16, 3):
        few = rng.choice(NB, size=min(NB, 3), replace=False)
        codes[f >> 4, :, f & 15] = few[rng.integers(0, len(few), size=n_rows)]
    return codes.astype(np.uint16)


def make_call(case, nodes, *, seed=0, n_rows=10000, m=8192, qmax=1 << 16, mode=0, trailing=0, n_hist_slots=None, slot_map=None, chunks_per_slot=1,
              scatter_fs=0, FG=None, count_rows=None):
    rng = np.random.default_rng(seed)
    c = Call()
    c.NB, c.D, c.FG, c.n_fslots = case.NB, case.D, case.FG if FG is None else FG, case.n_fslots
    c.count_rows = case.count_rows if count_rows is None else count_rows
    c.env = dict(case.env)
    c.n_rows, c.mode, c.chunks_per_slot, c.scatter_fs = n_rows, mode, chunks_per_slot, scatter_fs
    c.m = max(m, max([sum(n) for n in nodes] + [1]))
    c.codes = make_codes(rng, n_rows, c.padded(), c.NB)
    c.qg = rng.integers(-qmax, qmax + 1, size=(n_rows, c.D), dtype=np.int64).astype(np.int32)
    c.rows = rng.integers(0, n_rows, size=c.m, dtype=np.int64).astype(np.int32)        # drawn with replacement: a row may repeat inside a node
    chunks = []
    for k, lens in enumerate(nodes):
        start = int(rng.integers(0, c.m - sum(lens) + 1))                               # nodes may overlap in the row list: each is summed on its own
        for n in lens:
            chunks.append((k, start, n))
            start += n
    chunks += [(0, 0, 0)] * trailing
    c.chunks = np.array(chunks, np.int32).reshape(-1, 3)
    c.n_nodes = len(nodes)
    c.n_hist_slots = c.n_nodes if n_hist_slots is None else n_hist_slots
    c.slot_map = None if slot_map is None else np.asarray(slot_map, np.int32)
    c.root_le, c.root_F, c.root_B, c.root_n = None, 0, 0, 0
    return c


def reference(c):
    """The int64 histograms of a call, in the layout the call asks for; SENTINEL where nothing is stored."""
    Fp, D = c.padded(), c.D
    q1 = np.concatenate([c.qg.astype(np.int64), np.ones((c.n_rows, 1), np.int64)], axis=1)               # field D holds the count
    if not c.count_rows:
        q1[:, D] = 0
    by_row = c.codes.transpose(1, 0, 2).reshape(c.n_rows, -1)[:, :Fp].astype(np.int64)                   # [row][feature slot]
    H = np.zeros((c.n_nodes, Fp, c.NB, D + 1), np.int64)
    pos = [np.arange(s, s + n) for (_, s, n) in c.chunks if n > 0]
    node = [np.full(n, k) for (k, _, n) in c.chunks if n > 0]
    if pos:
        r = c.rows[np.concatenate(pos)]
        np.add.at(H, (np.concatenate(node)[:, None], np.arange(Fp)[None, :], by_row[r]), q1[r][:, None, :])
    if c.root_le is not None:
        # hist_reduce: "the count field of class c of numeric feature f becomes le[c] - le[c-1] (c = B: n_total - le[B-1])"; classes past B hold none
        le = c.root_le.astype(np.int64)
        full = np.concatenate([np.zeros((c.root_F, 1), np.int64), le, np.full((c.root_F, 1), c.root_n, np.int64)], axis=1)
        cnt = np.zeros((c.root_F, c.NB), np.int64)
        n = min(c.NB, c.root_B + 1)
        cnt[:, :n] = np.diff(full, axis=1)[:, :n]
        H[:, :c.root_F, :, D] = cnt[None]
    out = np.full(c.hist_shape(), SENTINEL, np.int64)
    if c.scatter_fs:
        fs = c.scatter_fs
        for f in range(Fp):                                                                             # [f / fs][node][f % fs][class][D+1]
            out[f // fs, :, f % fs] = H[:, f]
    else:
        for k in range(c.n_nodes):
            out[c.slot_map[k] if c.slot_map is not None else k] = H[k]
    return out


def probe(c, hist=None):
    """-> (return code, histograms, (kind, param, pipe, counted) of the kernel that ran, wrote_direct) of one gbrl_hip_hist_probe call under the call's hooks"""
    hist = np.full(c.hist_shape(), SENTINEL, np.int64) if hist is None else hist
    keep = [np.ascontiguousarray(c.codes, np.uint16), np.ascontiguousarray(c.qg, np.int32), np.ascontiguousarray(c.rows, np.int32),
            np.ascontiguousarray(c.chunks, np.int32)]
    a = ProbeArgs()
    a.codes, a.qg, a.rows, a.chunks = (x.ctypes.data for x in keep)
    if c.root_le is not None:
        keep.append(np.ascontiguousarray(c.root_le, np.uint32))
        a.root_le = keep[-1].ctypes.data
    if c.slot_map is not None:
        keep.append(np.ascontiguousarray(c.slot_map, np.int32))
        a.slot_map = keep[-1].ctypes.data
    a.hist, a.hist_elems, a.root_n = hist.ctypes.data, hist.size, c.root_n
    a.n_rows, a.output_dim, a.m, a.n_chunks, a.n_nodes, a.n_feature_slots = c.n_rows, c.D, c.m, len(c.chunks), c.n_nodes, c.n_fslots
    a.fg, a.n_classes, a.mode, a.count_rows, a.root_F, a.root_B = c.FG, c.NB, c.mode, int(c.count_rows), c.root_F, c.root_B
    a.chunks_per_slot, a.scatter_fs = c.chunks_per_slot, c.scatter_fs
    a.kind = a.param = a.pipe = a.counted = a.wrote_direct = -1
    saved = {k: os.environ.get(k) for k in ("GBRL_HIP_HIST_GENERIC", "GBRL_HIP_HIST_PIPE")}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(c.env)
        rc = lib().gbrl_hip_hist_probe(ctypes.byref(a))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return rc, hist, (a.kind, a.param, a.pipe, a.counted), a.wrote_direct
