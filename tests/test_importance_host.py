"""Feature importance, the parts that need no GPU (include/gbrl_hip.h, "Feature importance"):
  * gbrl_cpp.permutation_host, perm_core.h's rule on the host -- a bijection at the tile edges and at sizes whose Feistel domain is 1x, 2x and
    nearly 4x the row count, a function of (n, seed, col, repeat) alone;
  * GBRL.feature_importance('split' | 'cover') on models LOADED from the reference's own files (tests/golden/explain_*.npz: oblivious, greedy, with
    categorical columns) against a NumPy restatement written from get_ensemble_data() alone -- prefix dedupe for split, the leaf sum for cover --
    with exact float64 equality (every value is an integer);
  * the refusals, the C symbols, and the hook table kept in step with INTEGRATION.md section 5.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import cases as K
import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 1000, 4097, 65537)
MODELS = ("obl_l2_q", "obl_l2_q_d6", "grd_l2_q_mdl", "grd_cos_q_ac", "obl_l2_q_cat", "grd_cos_u_cat", "grd_l2_q_catonly")


# ---------------------------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("n", SIZES)
def test_permutation_is_a_bijection(n):
    for seed, col, repeat in ((0, 0, 0), (12345, 17, 3), (2 ** 64 - 1, 4095, 99)):
        p = cpp.permutation_host(n, seed=seed, col=col, repeat=repeat)
        assert p.dtype == np.int32 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n, dtype=np.int32)), (n, seed, col, repeat)


def test_permutation_depends_on_every_argument_and_on_nothing_else():
    n = 1000
    base = cpp.permutation_host(n, seed=5, col=2, repeat=1)
    assert np.array_equal(base, cpp.permutation_host(n, seed=5, col=2, repeat=1))     # two calls, the same list
    assert np.array_equal(cpp.permutation_host(n), cpp.permutation_host(n, 0, 0, 0))  # the defaults
    for other in (dict(seed=6, col=2, repeat=1), dict(seed=5, col=3, repeat=1), dict(seed=5, col=2, repeat=2)):
        assert not np.array_equal(base, cpp.permutation_host(n, **other)), other
    assert (base != np.arange(n)).mean() > 0.9                                       # a shuffle, not a near-identity


def test_permutation_of_one_row_and_the_refusals():
    assert cpp.permutation_host(1).tolist() == [0]
    assert cpp.permutation_host(1, seed=9, col=3, repeat=7).tolist() == [0]
    for kw, word in ((dict(n=0), "no rows"), (dict(n=-3), "no rows"), (dict(n=4, col=-1), "col must be >= 0"), (dict(n=4, repeat=-1), "repeat must be >= 0")):
        with pytest.raises(RuntimeError, match=word):
            cpp.permutation_host(**kw)


def test_geometry_and_c_symbols():
    assert cpp.permutation_geometry() == {"launch_variants": 64, "tile_rows": 64}
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    for name in ("gbrl_hip_permutation_host", "gbrl_hip_permutation_importance_prepared", "gbrl_hip_permutation_geometry", "gbrl_hip_feature_importance"):
        assert hasattr(lib, name), name
    n = 257
    out = np.full(n, -1, np.int32)
    lib.gbrl_hip_permutation_host.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert lib.gbrl_hip_permutation_host(n, 11, 5, 2, out.ctypes.data) == 0
    assert np.array_equal(out, cpp.permutation_host(n, 11, 5, 2))
    assert lib.gbrl_hip_permutation_host(n, 11, 5, 2, None) != 0


def test_perm_generic_hook_is_in_the_table_and_documented():
    names = re.findall(r"^\s+X\(([A-Z0-9_]+)\)", open(os.path.join(ROOT, "gbrl_amd", "csrc", "hooks.h")).read(), re.M)
    assert "PERM_GENERIC" in names
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section5 = doc[doc.index("## 5"):]
    assert "`GBRL_HIP_PERM_GENERIC=1`" in section5
    assert "hooks::PERM_GENERIC" in open(os.path.join(ROOT, "gbrl_amd", "csrc", "engine_importance.hip")).read()


# ---------------------------------------------------------------------------------------------------------------- split and cover
def _load(name, tmp_path):
    g = np.load(os.path.join(GOLDEN, "explain_" + name + ".npz"))
    p = tmp_path / "ref.gbrl_model"
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


def _restated(m, kind, counts=None):
    """split / cover from get_ensemble_data() alone.  A decision is a level of an oblivious tree or a distinct internal node of a greedy tree: the node
    above a leaf at depth d is named by the leaf's first d directions.  The feature axis is ensemble_shap's: the raw feature index."""
    e, md = m.get_ensemble_data(), m.get_metadata()
    oblivious = md["grow_policy"] == "Oblivious"
    ti, depths, fidx = np.asarray(e["tree_indices"]), np.asarray(e["depths"]), np.asarray(e["feature_indices"])
    dirs = np.asarray(e["inequality_directions"])
    L = np.asarray(e["values"]).shape[0]
    out = np.zeros(md["input_dim"], np.float64)
    for t in range(len(ti)):
        first, end = int(ti[t]), int(ti[t + 1]) if t + 1 < len(ti) else L
        nodes = set()
        for leaf in range(first, end):
            row = t if oblivious else leaf
            for d in range(int(depths[row])):
                f = int(fidx[row, d])
                if kind == "cover":
                    out[f] += float(counts[leaf])
                    continue
                node = d if oblivious else (d, tuple(bool(x) for x in dirs[leaf, :d]))
                if node not in nodes:
                    nodes.add(node)
                    out[f] += 1.0
    return out


@pytest.mark.parametrize("name", MODELS)
def test_split_and_cover_equal_the_restatement(name, tmp_path):
    m = _load(name, tmp_path)
    md, e = m.get_metadata(), m.get_ensemble_data()
    case = K.BY_NAME[name]
    assert (md["grow_policy"] == "Oblivious") == (case["policy"] == "oblivious")
    L = np.asarray(e["values"]).shape[0]
    split = m.feature_importance("split")
    assert split.dtype == np.float64 and split.shape == (md["input_dim"],)
    want = _restated(m, "split")
    assert np.array_equal(split, want), (split, want)
    assert np.array_equal(m.feature_importance(), split)            # 'split' is the default
    assert split.sum() >= len(np.asarray(e["tree_indices"]))         # the fixtures' trees all split at least once
    if case["policy"] == "oblivious":
        assert split.sum() == np.asarray(e["depths"]).sum()
    else:   # a binary tree has one internal node fewer than leaves
        assert split.sum() == L - len(np.asarray(e["tree_indices"]))
    rng = np.random.default_rng(7)
    for counts in (rng.integers(0, 1000, L).astype(np.int64), np.ones(L, np.int64)):
        cover = m.feature_importance("cover", leaf_counts=counts)
        assert cover.dtype == np.float64
        assert np.array_equal(cover, _restated(m, "cover", counts))
    assert np.array_equal(m.feature_importance("cover", np.ones(L, np.int32)), _restated(m, "cover", np.ones(L, np.int64)))   # any integer vector


def test_the_fixtures_cover_both_policies_and_categorical_conditions(tmp_path):
    seen = set()
    for name in MODELS:
        m = _load(name, tmp_path)
        e = m.get_ensemble_data()
        depths, isnum = np.asarray(e["depths"]), np.asarray(e["is_numerics"])
        used = np.arange(isnum.shape[1])[None, :] < depths[:, None]
        seen.add((m.get_metadata()["grow_policy"], bool((~isnum & used).any())))
    assert seen >= {("Oblivious", False), ("Greedy", False), ("Oblivious", True), ("Greedy", True)}, seen


def test_feature_importance_refusals(tmp_path):
    m = _load("grd_l2_q_mdl", tmp_path)
    L = np.asarray(m.get_ensemble_data()["values"]).shape[0]
    with pytest.raises(RuntimeError, match="needs leaf_counts"):
        m.feature_importance("cover")
    with pytest.raises(RuntimeError, match="one count per leaf"):
        m.feature_importance("cover", np.ones(L + 1, np.int64))
    with pytest.raises(RuntimeError, match="one count per leaf"):
        m.feature_importance("cover", np.ones((L, 1), np.int64))
    with pytest.raises(RuntimeError, match="negative"):
        m.feature_importance("cover", -np.ones(L, np.int64))
    with pytest.raises(RuntimeError, match="Invalid kind"):
        m.feature_importance("gain")
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_feature_importance.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    out = np.zeros(m.get_metadata()["input_dim"], np.float64)
    assert lib.gbrl_hip_feature_importance(m._handle(), 0, None, out.ctypes.data) == 0 and np.array_equal(out, m.feature_importance("split"))
    assert lib.gbrl_hip_feature_importance(m._handle(), 1, None, out.ctypes.data) != 0     # cover without counts
    assert lib.gbrl_hip_feature_importance(m._handle(), 2, None, out.ctypes.data) != 0     # an unknown kind
    fresh = gbrl_amd.GBRL(input_dim=5, output_dim=2, policy_dim=2, max_depth=3, n_bins=16, split_score_func="L2", generator_type="Quantile",
                          grow_policy="oblivious", device="cpu", batch_size=64)
    assert np.array_equal(fresh.feature_importance("split"), np.zeros(5))                  # no trees: no decisions
