"""The host side of the split-score histogram build, without a device: which kernel a shape gets (gbrl_hip_hist_plan against both rules written
out once more in tests/hist_cases.py: the features-per-block rule of the engine and the route of step_hist_build.hip), that every instantiation
the route can reach has a case in tests/hist_cases.py (tests/test_gpu_hist_cells.py runs them), and that gbrl_hip_hist_probe refuses on the
host whatever would make a kernel index outside its arrays."""
import ctypes
import os

import numpy as np
import pytest

import hist_cases as H


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    monkeypatch.delenv("GBRL_HIP_HIST_GENERIC", raising=False)
    monkeypatch.delenv("GBRL_HIP_HIST_PIPE", raising=False)


def _nb_sweep():
    """2..300, then both sides of every class count at which some D in 1..128 changes FG (the LDS breaks), up to 4100"""
    nbs = set(range(2, 301))
    for D in range(1, 129):
        for FG in (16, 8, 4, 2, 1):
            edge = H.LDS_LIMIT // (4 * (D + 1) * FG)
            nbs.update(n for n in (edge, edge + 1) if 2 <= n <= 4100)
    nbs.update((4099, 4100))
    return sorted(nbs)


def _sweep(hooks):
    """every (NB, D) of the sweep -> (Plan, restated FG, restated route)"""
    generic, pipe = hooks.get("GBRL_HIP_HIST_GENERIC") == "1", hooks.get("GBRL_HIP_HIST_PIPE") != "0"
    for NB in _nb_sweep():
        for D in range(1, 129):
            FG = H.feature_group(NB, D)
            yield NB, D, H.plan(NB, D), FG, H.route(D, FG, 10000, generic, pipe)


def test_the_symbols_are_exported():
    so = H.lib()
    assert so.gbrl_hip_hist_plan and so.gbrl_hip_hist_probe
    so.gbrl_hip_abi_version.restype = ctypes.c_int
    assert so.gbrl_hip_abi_version() == 1


@pytest.mark.parametrize("hooks", [{}, {"GBRL_HIP_HIST_PIPE": "0"}, {"GBRL_HIP_HIST_GENERIC": "1"}], ids=["default", "nopipe", "generic"])
def test_plan_equals_the_restated_rules(hooks, monkeypatch):
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    n = 0
    for NB, D, p, FG, (kind, param, pipe, direct_ok, countless_ok) in _sweep(hooks):
        got = (p.fg, p.kind, p.param, p.pipe, p.direct_ok, p.countless_ok, p.hist_lds_bytes)
        assert got == (FG, kind, param, int(pipe), int(direct_ok), int(countless_ok), H.lds_bytes(NB, D, FG)), (NB, D, got)
        n += 1
    assert n > 300 * 128


def test_plan_with_a_given_fg():
    """FG_in != 0 is used as given, whatever the engine would choose; anything but 1, 2, 4, 8, 16 is refused"""
    for NB, D in ((32, 8), (32, 17), (32, 31), (32, 32), (32, 63), (32, 64), (3000, 1), (20000, 1)):
        for FG in (1, 2, 4, 8, 16):
            p = H.plan(NB, D, 10000, FG)
            kind, param, pipe, direct_ok, countless_ok = H.route(D, FG, 10000)
            assert (p.fg, p.kind, p.param, p.pipe, p.direct_ok, p.countless_ok, p.hist_lds_bytes) == \
                   (FG, kind, param, int(pipe), int(direct_ok), int(countless_ok), H.lds_bytes(NB, D, FG)), (NB, D, FG)
    for bad in (-1, 3, 5, 12, 32):
        assert H.plan(32, 8, 10000, bad) is None
    assert H.plan(0, 8) is None and H.plan(32, 0) is None and H.plan(32, 8, 0) is None
    assert H.lib().gbrl_hip_hist_plan(32, 8, 10000, 0, None) == H.E_INVALID


def test_the_row_bound_of_the_compile_time_kernels():
    """32-bit byte offsets from block-uniform bases: 2^26 rows keep the routed kernel, one more takes the run-time-D kernel"""
    for NB, D, kind in ((32, 8, H.FIXED_D), (32, 16, H.FIXED_D), (24, 20, H.WIDE), (12, 40, H.QUAD)):
        at, over = H.plan(NB, D, 1 << 26), H.plan(NB, D, (1 << 26) + 1)
        assert at.kind == kind and (at.countless_ok == 1) == (kind == H.FIXED_D)
        assert (over.kind, over.param, over.pipe, over.countless_ok) == (H.GENERIC, 0, 0, 0) and over.fg == at.fg and over.direct_ok == at.direct_ok


def test_every_reachable_instantiation_has_a_case():
    """Closure: every (FG, kind, param, pipe) the route reaches with the engine's own FG -- over the sweep, with and without the pipeline hook,
    on shapes whose tile fits the LDS -- is the key of a case of tests/hist_cases.py, and the count-less form of every pipelined key as well."""
    have = {(c.FG, c.kind, c.param, c.pipe) for c in H.CASES}
    countless = {(c.FG, c.kind, c.param) for c in H.CASES if not c.count_rows}
    reached = set()
    for hooks in ({}, {"GBRL_HIP_HIST_PIPE": "0"}):
        for k, v in hooks.items():
            os.environ[k] = v
        try:
            for NB, D, p, FG, _ in _sweep(hooks):
                if p.hist_lds_bytes <= H.LDS_LIMIT:
                    reached.add((p.fg, p.kind, p.param, bool(p.pipe)))
                    if p.countless_ok:
                        assert (p.fg, p.kind, p.param) in countless, (NB, D)
        finally:
            for k in hooks:
                os.environ.pop(k, None)
    assert reached - have == set(), sorted(reached - have)
    # and the table holds every form by name: compile-time D 1..16 pipelined, unpipelined and count-less, wide H 1..16, quad R 1..16, the run-time-D kernel at
    # FG 16 (hook), FG 4 with D = 64 and 100, FG 2 and FG 1 with an LDS tile whose size is no multiple of 4 (the scalar clear and store)
    assert {(c.param, c.pipe, c.count_rows) for c in H.CASES if c.kind == H.FIXED_D} == {(D, p, cr) for D in range(1, 17) for p, cr in ((True, True), (False, True), (True, False))}
    assert {c.param for c in H.CASES if c.kind == H.WIDE} == set(range(1, 17)) and {c.param for c in H.CASES if c.kind == H.QUAD} == set(range(1, 17))
    assert {c.FG for c in H.CASES if c.kind == H.GENERIC} == {16, 4, 2, 1}
    assert {c.D for c in H.CASES if c.kind == H.GENERIC and c.FG == 4} == {64, 100}
    assert any((c.NB * (c.D + 1) * c.FG) % 4 for c in H.CASES if c.FG in (1, 2))
    for c in H.CASES:                                         # the engine's own FG, by the library's word too
        assert H.plan(c.NB, c.D).fg == c.FG, c


# ------------------------------------------------------------------------------------------------------------ refusals

def _small_call(**kw):
    c = H.make_call(H.BY_NAME["fixed-D3-pipe"], [[5], [7, 7], [3]], n_rows=64, m=40, **kw)
    return c


def _refused(c, why, hist=None):
    """the call is refused, for the reason meant, and nothing was written anywhere"""
    rc, hist, ran, direct = H.probe(c, hist)
    assert ran == (-1, -1, -1, -1) and direct == -1
    assert np.all(hist == H.SENTINEL)
    msg = H.lib().gbrl_hip_last_error().decode()
    return rc == H.E_INVALID and why in msg


def test_probe_refuses_on_the_host():
    """Every refusal returns GBRL_HIP_E_INVALID with its own reason -- not the HIP error that a call which reaches hipMalloc gets without a device"""
    c = _small_call()
    c.codes[1, 63, 15] = c.NB                              # a code in the padding of the last group
    assert _refused(c, "class code")
    c = _small_call()
    c.codes[0, 0, 0] = 65535
    assert _refused(c, "class code")
    for bad in (-1, 64):
        c = _small_call()
        c.rows[17] = bad
        assert _refused(c, "row index")
    for chunk in ((0, 38, 3), (0, -1, 2), (0, 41, 0), (0, 0, 41), (3, 0, 1), (-1, 0, 1), (0, 1 << 30, 1 << 30)):
        c = _small_call()
        c.chunks[0] = chunk
        assert _refused(c, "a chunk lies outside"), chunk
    c = _small_call()
    c.chunks[[0, 3]] = c.chunks[[3, 0]]                    # slots descend
    assert _refused(c, "ascend")
    c = _small_call()
    c.chunks[1, 2] = 0                                     # an empty chunk in front of chunks with rows: no block would write its partials
    assert _refused(c, "empty chunk")
    for FG in (0, 3, 5, 32):
        assert _refused(_small_call(FG=FG), "FG must be"), FG
    # the LDS tile: n_classes x (D + 1) x FG x 4 bytes over 160 KiB - 512
    big = H.Case("big", H.LDS_LIMIT // (4 * 4 * 16) + 1, 3, 16, H.FIXED_D, 3, True, True, {}, 19)
    assert _refused(H.make_call(big, [[5]], n_rows=64, m=40), "does not fit the LDS")
    # HistDirect: only where direct_ok holds, and every node one chunk
    wide, quad = H.BY_NAME["wide-H10-D18"], H.BY_NAME["quad-R9-D35"]
    assert _refused(H.make_call(wide, [[5], [7]], n_rows=64, m=40, mode=1), "no direct store")
    assert _refused(H.make_call(quad, [[5], [7]], n_rows=64, m=40, mode=1), "no direct store")
    assert _refused(_small_call(mode=1), "every node to be one chunk")                   # node 1 is two chunks
    c = H.make_call(H.BY_NAME["fixed-D3-pipe"], [[5], [7], [3]], n_rows=64, m=40, mode=1)
    c.chunks[1, 0] = 2                                     # a node without a chunk, another with two
    assert _refused(c, "every node to be one chunk")
    assert _refused(_small_call(mode=2), "mode must be")
    # root_le and the count-less build: only where countless_ok holds
    le = np.zeros((3, 31), np.uint32)
    for case in (H.BY_NAME["fixed-D3-nopipe"], wide, quad, H.BY_NAME["generic-FG16-D5"]):
        c = H.make_call(case, [[5], [7]], n_rows=64, m=40)
        c.root_le, c.root_F, c.root_B, c.root_n = le, 3, 31, 64
        assert _refused(c, "no count-less build"), case.name
        assert _refused(H.make_call(case, [[5], [7]], n_rows=64, m=40, count_rows=False), "no count-less build"), case.name
    # slot_map and the histogram buffer
    assert _refused(_small_call(slot_map=[0, 1, 3]), "slot_map")
    assert _refused(_small_call(slot_map=[0, 1, 1]), "slot_map")
    assert _refused(_small_call(slot_map=[0, -1, 2]), "slot_map")
    assert _refused(_small_call(n_hist_slots=2), "hist_elems")
    c = _small_call()
    assert _refused(c, "hist_elems", np.full(c.hist_shape()[0] * c.hist_shape()[1] * c.NB * (c.D + 1) - 1, H.SENTINEL, np.int64))
    c = _small_call(scatter_fs=5)
    assert _refused(c, "hist_elems", np.full((3, 32, c.NB, c.D + 1), H.SENTINEL, np.int64))
    c = _small_call()
    c.n_nodes = 65536                                      # hist_reduce takes one grid z per node: 65535 at the most
    assert _refused(c, "a size is out of range")
    a = H.ProbeArgs()
    assert H.lib().gbrl_hip_hist_probe(ctypes.byref(a)) == H.E_INVALID and H.lib().gbrl_hip_hist_probe(None) == H.E_INVALID


def test_the_reference_on_a_case_small_enough_to_count_by_hand():
    """the NumPy reference of tests/hist_cases.py itself: two rows, one of them twice, in the node layout and in the scatter layout"""
    case = H.Case("tiny", 3, 2, 16, H.FIXED_D, 2, True, True, {}, 2)
    c = H.make_call(case, [[3], []], n_rows=2, m=3, n_hist_slots=3, slot_map=[2, 0])
    c.rows[:] = (1, 0, 1)
    c.chunks[0] = (0, 0, 3)
    c.codes[:] = 0
    c.codes[0, :, 0] = (2, 1)
    c.qg[:] = ((5, -7), (100, 1000))
    ref = H.reference(c)
    assert ref.shape == (3, 16, 3, 3)
    assert ref[2, 0].tolist() == [[0, 0, 0], [200, 2000, 2], [5, -7, 1]] and ref[2, 1].tolist() == [[205, 1993, 3], [0, 0, 0], [0, 0, 0]]
    assert np.all(ref[0] == 0) and np.all(ref[1] == H.SENTINEL)
    c.slot_map, c.scatter_fs = None, 5
    ref = H.reference(c)
    assert ref.shape == (4, 2, 5, 3, 3) and ref[0, 0, 1].tolist() == [[205, 1993, 3], [0, 0, 0], [0, 0, 0]] and np.all(ref[3, :, 1:] == H.SENTINEL) and np.all(ref[3, 1, 0] == 0)
    c.root_le, c.root_F, c.root_B, c.root_n = np.array([[1, 1]], np.uint32), 1, 2, 3
    assert H.reference(c)[0, 0, 0, :, 2].tolist() == [1, 0, 2] and H.reference(c)[0, 0, 1, :, 2].tolist() == [3, 0, 0]
