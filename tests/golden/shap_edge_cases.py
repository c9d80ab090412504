"""Case list of the TreeSHAP launch-geometry fixtures (shap_edge_*.npz: made by make_shap_edge_golden.py, read by
tests/test_shap_edges_host.py and tests/test_gpu_shap_edges.py).  Same case dicts as cases.py; inputs come from cases.make_inputs.

The device kernel (csrc/shap.hip) runs one thread per (sample, output) and sizes its block by the MODEL's max_depth and output_dim D, whatever
depth the trees reach (kern::shap_block_threads; every thread holds 2 * (max_depth + 1)^2 floats of LDS, the budget is 156 KiB):

    max_depth <= 7        256 threads      2048 * (7 + 1)^2  = 128 KiB     (max_depth 8:  162 KiB)
    max_depth 8 .. 11     128 threads      1024 * (11 + 1)^2 = 144 KiB     (max_depth 12: 169 KiB)
    max_depth 12 .. 16     64 threads       512 * (16 + 1)^2 = 144.5 KiB   (max_depth 17: 162 KiB)
    max_depth > 16, or D above the block size: the host evaluation

threads / D samples share a block; when D does not divide the block size the remaining threads run the program as dead lanes.  PLAN below
states this table for every case as (threads, samples per block), (0, 0) = host.

Most cases set a large max_depth on trees that stop early (min_data_in_leaf against a small N): the kernel's LDS size and its loops over
max_depth columns follow the setting, while the values stay well conditioned.  `batches` (optional) gives the number of leading rows each
tree is stepped on; a batch smaller than 2 * min_data_in_leaf grows a depth-0 tree (one leaf, no condition).  `shap_rows` is how many
leading rows the fixture stores the reference's SHAP values for (few for wide outputs: the arrays are [rows][features][D]).

The reference's unpatched build cannot construct most of these models: its constructor allocates 50000 * 2^max_depth leaves up front
(gbrl.cpp:82, types.cpp:207-251) and computes the sizes in int.  Refused (an int overflows: bad_alloc): every greedy case with max_depth
>= 6 -- (7, 3), (8, 65), (8, 129), (11, 5), (12, 3), (12, 65), (16, 2) -- through the per-leaf 128-byte categorical values; (16, 5) and
(17, 2) through the leaf count; (12, 64) through leaves * output_dim.  Constructible only with 7 GB and more of memory: (8, 128).  The
fixtures are therefore made by the capacity-only build `make -C oracle ref-small` (ONE define, the initial tree capacity 50000 -> 4; same
flags, same arithmetic), like cases.py's `ref_patch` cases, and no shape of the table had to be replaced by a neighbour.
"""
from cases import _c

REF_PATCH = "types.h:49 INITAL_MAX_TREES 50000 -> 4 (capacity only)"


def _s(name, depth, D, **kw):
    kw.setdefault("N", 200)
    kw.setdefault("F", 4)
    kw.setdefault("trees", 3)
    kw.setdefault("n_bins", 32)
    kw.setdefault("min_data_in_leaf", 25)
    kw.setdefault("shap_rows", 40 if D <= 8 else 6)
    return _c(name, depth=depth, D=D, ref_patch=REF_PATCH, **kw)


CASES = [
    # ---- 256-thread plan ----
    # greedy, two features, min_data_in_leaf 1 on 48 rows: paths of depth 5 .. 7 on which a feature occurs three times and more (a chain of
    # nodes tied to their parents); 85 samples per block + 1 dead lane
    _s("t256_d7_D3_grd_tied", 7, 3, seed=101, N=48, F=2, policy="greedy", min_data_in_leaf=1, trees=3),
    # oblivious, two features on 7 levels (40 rows, no min_data_in_leaf): every tree repeats both features; 51 samples per block + 1 dead lane
    _s("t256_d7_D5_obl_repeat", 7, 5, seed=102, N=40, F=2, min_data_in_leaf=0, trees=3),
    # numeric + categorical columns at the trees' full depth; 36 samples per block + 4 dead lanes
    _s("t256_d4_D7_grd_cat", 4, 7, seed=103, N=400, F=3, Fc=2, policy="greedy", score="Cosine", gen="Uniform", min_data_in_leaf=0, n_tokens=5),
    _s("t256_d4_D128_obl", 4, 128, seed=104, F=3, trees=2),                               # 2 samples per block, no dead lane
    _s("t256_d4_D129_grd", 4, 129, seed=105, F=3, policy="greedy", trees=2),              # 1 sample per block, 127 dead lanes
    _s("t256_d4_D200_obl_cat", 4, 200, seed=106, N=300, F=1, Fc=2, trees=2, n_tokens=4, min_data_in_leaf=10),   # 1 sample per block, 56 dead lanes
    _s("t256_d4_D256_grd", 4, 256, seed=107, F=3, policy="greedy", score="Cosine", trees=2),   # 1 sample per block, the block is full
    _s("host_d4_D257_obl", 4, 257, seed=108, F=3, trees=2),                               # one sample's outputs do not fit 256 threads
    # ---- 128-thread plan ----
    # oblivious trees that really reach depth 8 (256 leaves on 300 rows; three features, so at most 3 distinct per path: the normalisation
    # rows stay small); 42 samples per block + 2 dead lanes
    _s("t128_d8_D3_obl_deep", 8, 3, seed=109, N=300, F=3, min_data_in_leaf=0, trees=2),
    _s("t128_d11_D5_grd_catonly", 11, 5, seed=110, F=0, Fc=3, policy="greedy", n_tokens=6, min_data_in_leaf=10),   # categorical columns only
    _s("t128_d8_D64_obl", 8, 64, seed=111, F=3, score="Cosine", trees=2),                 # 2 samples per block
    _s("t128_d8_D65_grd", 8, 65, seed=112, F=3, policy="greedy", trees=2),                # 1 sample per block, 63 dead lanes
    _s("t128_d8_D128_obl", 8, 128, seed=113, F=3, gen="Uniform", trees=2),                # 1 sample per block, the block is full
    _s("host_d8_D129_grd", 8, 129, seed=114, F=3, policy="greedy", trees=2),
    # ---- 64-thread plan ----
    # greedy; the second of three trees is stepped on 30 rows against min_data_in_leaf 25: a depth-0 tree between full ones
    _s("t64_d12_D3_grd_stump", 12, 3, seed=115, policy="greedy", batches=[200, 30, 200]),
    _s("t64_d16_D5_obl", 16, 5, seed=116, score="Cosine"),                                # 12 samples per block + 4 dead lanes
    _s("t64_d12_D64_obl", 12, 64, seed=117, F=3, trees=2),                                # 1 sample per block, the block is full
    _s("host_d12_D65_grd", 12, 65, seed=118, F=3, policy="greedy", trees=2),
    # ---- depth boundary ----
    _s("t64_d16_D2_grd", 16, 2, seed=119, policy="greedy", score="Cosine"),               # 32 samples per block
    _s("host_d17_D2_obl", 17, 2, seed=120),
]

BY_NAME = {c["name"]: c for c in CASES}

# name -> (threads per block, samples per block) as derived above; (0, 0): the kernel declines, the host evaluates
PLAN = {
    "t256_d7_D3_grd_tied": (256, 85), "t256_d7_D5_obl_repeat": (256, 51), "t256_d4_D7_grd_cat": (256, 36), "t256_d4_D128_obl": (256, 2),
    "t256_d4_D129_grd": (256, 1), "t256_d4_D200_obl_cat": (256, 1), "t256_d4_D256_grd": (256, 1), "host_d4_D257_obl": (0, 0),
    "t128_d8_D3_obl_deep": (128, 42), "t128_d11_D5_grd_catonly": (128, 25), "t128_d8_D64_obl": (128, 2), "t128_d8_D65_grd": (128, 1),
    "t128_d8_D128_obl": (128, 1), "host_d8_D129_grd": (0, 0),
    "t64_d12_D3_grd_stump": (64, 21), "t64_d16_D5_obl": (64, 12), "t64_d12_D64_obl": (64, 1), "host_d12_D65_grd": (0, 0),
    "t64_d16_D2_grd": (64, 32), "host_d17_D2_obl": (0, 0),
}
DEVICE_CASES = [n for n, p in PLAN.items() if p[0]]
HOST_CASES = [n for n, p in PLAN.items() if not p[0]]


def batches(case):
    return case.get("batches", [case["N"]] * case["trees"])
