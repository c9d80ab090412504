"""CPU-side check of the launch plan behind `leaf_counts_prepared` (include/gbrl_hip.h: gbrl_hip_leaves_prepared_geometry needs no device)."""
import ctypes

import pytest

import gbrl_amd

BUDGET, FLOOR = 156 * 1024, 4096          # the LDS opt-in; k_leaf_counts' chunk, the floor of the chosen one


# 40: a chunk above the floor; 69 / 70: the last width whose tile fits beside the floor, and the first that does not
@pytest.mark.parametrize("G", [1, 8, 40, 69, 70, 76, 77, 200])
def test_launch_plan(G):
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_leaves_prepared_geometry.restype = None
    group, chunk, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_uint64(0)
    lib.gbrl_hip_leaves_prepared_geometry(G, ctypes.byref(group), ctypes.byref(chunk), ctypes.byref(lds))
    assert (group.value, chunk.value, lds.value) == gbrl_amd.GBRL.leaves_prepared_geometry(G)
    tile = 64 * ((G * 8) | 1) * 4                                        # 64 rows at the documented odd word stride
    assert group.value == 16
    if tile + 4 * FLOOR > BUDGET:
        assert chunk.value == 0
        return
    c = chunk.value
    assert c >= FLOOR and c & (c - 1) == 0
    assert lds.value == tile + 4 * c and lds.value <= BUDGET
    per_cu = lambda nbytes: min(8, max(1, 160 * 1024 // nbytes))
    assert c == FLOOR or per_cu(tile + 4 * c) == per_cu(tile)            # above the floor the counters cost no block per CU
