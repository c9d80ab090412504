"""Pins the oracle: the restatement (oracle/oracle.cpp) must reproduce, bit for bit, the golden vectors that the
reference's own CPU path produced (tests/golden/make_golden.py), and the reference itself on fresh seeds -- live when the
reference build oracle/_ref is present, else as recorded from it (tests/golden/ref_recordings.npz)."""
import os

import numpy as np
import pytest

import cases as K
import oracle
from helpers import STRUCTURE_KEYS, VALUE_KEYS, RefScalars, load_golden, ref_arrays


@pytest.mark.parametrize("name", [c["name"] for c in K.CASES])
def test_restatement_matches_golden_bit_exact(name):
    case, g, (X, Xc, G, y) = load_golden(name)
    m = oracle.OracleGBRL(**K.ctor_kwargs(case))
    pred = K.drive(m, case, X, Xc, G, y)
    e = m.get_ensemble_data()
    for k in STRUCTURE_KEYS + VALUE_KEYS:
        assert np.array_equal(e[k], g[k]), k
    assert np.array_equal(np.asarray(pred).reshape(g["pred"].shape), g["pred"])
    assert m.get_num_trees() == int(g["n_trees"]) and m.get_iteration() == int(g["iteration"])


@pytest.mark.parametrize("seed", [101, 102, 103])
@pytest.mark.parametrize("policy,score,gen", [("oblivious", "L2", "Quantile"), ("greedy", "Cosine", "Uniform"),
                                              ("greedy", "L2", "Quantile"), ("oblivious", "Cosine", "Quantile")])
def test_restatement_matches_reference_build_live(seed, policy, score, gen):
    case = dict(name="live", seed=seed, N=900, F=5, Fc=1, D=2, depth=3, n_bins=64, score=score, gen=gen,
                policy=policy, trees=2)
    X, Xc, G, y = K.make_inputs(case)

    def reference(ref):
        a = ref.GBRL(**K.ctor_kwargs(case))
        pa = K.drive(a, case, X, Xc, G, y)
        ea = a.get_ensemble_data()
        return dict({k: ea[k] for k in STRUCTURE_KEYS + VALUE_KEYS}, pred=pa)
    ea = ref_arrays("live_%d_%s_%s_%s" % (seed, policy, score, gen), reference)
    b = oracle.OracleGBRL(**K.ctor_kwargs(case))
    pb = K.drive(b, case, X, Xc, G, y)
    eb = b.get_ensemble_data()
    for k in STRUCTURE_KEYS + VALUE_KEYS:
        assert np.array_equal(np.asarray(ea[k]), eb[k]), k
    assert np.array_equal(np.asarray(ea["pred"]), pb)


def test_quantile_thresholds_are_order_statistics():
    """A3: threshold i of feature f is the data value at sorted rank cum(bin_counts)[i]-1, duplicates kept (Q1)."""
    case = K.BY_NAME["obl_l2_q_dups"]
    X, Xc, G, y = K.make_inputs(case)
    m = oracle.OracleGBRL(**K.ctor_kwargs(case))
    K.drive(m, dict(case, trees=1), X, Xc, G, y)
    fi, val, is_cat, _ = m.last_candidates()
    N, F, B = case["N"], case["F"], case["n_bins"]
    assert len(fi) == F * B and not is_cat.any()
    counts = np.full(B + 1, N // (B + 1)); counts[: N % (B + 1)] += 1
    ranks = np.cumsum(counts)[:B] - 1
    for f in range(F):
        assert np.array_equal(val[f * B:(f + 1) * B], np.sort(X[:, f])[ranks])
        assert (fi[f * B:(f + 1) * B] == f).all()


def test_uniform_thresholds_are_fused_multiply_add():
    """A4 / Q5: min + b*step evaluated with ONE rounding (float64 product+sum rounds identically here)."""
    case = K.BY_NAME["obl_l2_u"]
    X, Xc, G, y = K.make_inputs(case)
    m = oracle.OracleGBRL(**K.ctor_kwargs(case))
    K.drive(m, dict(case, trees=1), X, Xc, G, y)
    _, val, _, _ = m.last_candidates()
    B = case["n_bins"]
    for f in range(case["F"]):
        mn, mx = X[:, f].min(), X[:, f].max()
        step = np.float32((mx - mn) / np.float32(B))
        want = (np.arange(B, dtype=np.float64) * np.float64(step) + np.float64(mn)).astype(np.float32)
        assert np.array_equal(val[f * B:(f + 1) * B], want)


def test_restatement_agrees_with_the_reference_build_beyond_the_fixtures():
    """scripts/oracle_vs_ref_sweep.py in miniature: the restatement against the REAL reference build on random cases from regimes no
    committed fixture covers (13-33 outputs, 500 bins, feature weights with zeros, many categorical columns).  150 cases were run when
    the script was written: 149 bit-identical, 1 explained near-tie.  Without oracle/_ref the script reads the reference's trees from the
    recording."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "oracle_vs_ref_sweep.py"), "16", "977"], capture_output=True, text=True,
                         timeout=900, env=dict(os.environ, OMP_NUM_THREADS="8"))
    assert out.returncode == 0 and "unexplained 0" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("policy,score", [("oblivious", "L2"), ("oblivious", "Cosine"), ("greedy", "Cosine"), ("greedy", "L2")])
def test_fullsize_checker_agrees_with_the_reference_build(policy, score):
    """tests/fullsize.py (the float64 histogram re-evaluation the full-size GPU tests use as their third opinion) is itself pinned:
    on a batch the reference's brute force still handles, the reference's own tree must pass it level by level."""
    import fullsize
    ref = oracle.load_ref()
    impl = ref.GBRL if ref is not None else oracle.OracleGBRL
    rng = np.random.default_rng(31)
    N, F, D, B, depth = 6000, 6, 3, 40, 3
    X = rng.standard_normal((N, F)).astype(np.float32)
    X[:, 4] = np.round(X[:, 4] * 2) / 2                       # duplicates: candidates with equal thresholds
    W = rng.standard_normal((3, D)).astype(np.float32)
    G = (np.tanh(X[:, :3] @ W) + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    case = dict(name="fs", seed=0, N=N, F=F, D=D, depth=depth, n_bins=B, score=score, gen="Quantile", policy=policy, trees=1)
    m = impl(**K.ctor_kwargs(case))
    K.drive(m, case, X, None, G, None)
    e = {k: np.asarray(v) for k, v in m.get_ensemble_data().items()}
    tol = 4.0 * np.finfo(np.float32).eps * np.sqrt(N)          # the reference's own float32 summation noise (tests/neartie.py)
    if policy == "oblivious":
        recs = fullsize.check_oblivious_tree(X, G, e, B, score, rel_tol=tol)
        assert len(recs) == depth
    else:
        leaves = [0, len(e["values"]) - 1]
        recs = fullsize.check_greedy_nodes(X, G, e, B, score, leaves, [0, int(e["depths"][leaves[1]]) - 1], rel_tol=tol)
    assert all(r["exact"] for r in recs), recs


def _random_node(rng, rep):
    D = int(rng.integers(1, 41)) if rep % 7 else int(rng.integers(1, 131))
    N = int(rng.integers(1, 600))
    F = int(rng.integers(1, 6))
    obs = rng.standard_normal((N, F)).astype(np.float32)
    sc = np.exp(rng.standard_normal() * 3)
    g = (rng.standard_normal((N, D)) * sc + (0.3 * sc if rep % 3 else 0)).astype(np.float32)
    rows = np.flatnonzero(rng.integers(0, 4, N) > 0).astype(np.int32)
    if rep % 11 == 0:
        rows = rows[:int(rng.integers(1, 4))]
    return obs, g, rows, int(rng.integers(0, F)), float(np.float32(rng.standard_normal() * 0.7))


@pytest.mark.parametrize("cosine", [True, False])
def test_replay_sequence_is_the_reference_functions_bit_for_bit(cosine):
    """oracle/replay_sequence.cpp (explicit fmaf / rounded products, built without contraction) against TreeNode::splitScoreCosine /
    splitScoreL2 and scoreCosine / scoreL2 of the reference build on random nodes: every output width 1..130, nodes of 0..600 rows,
    gradient scales over six decades.  This pins the operation sequence the product's near-tie replay implements."""
    rng = np.random.default_rng(5 if cosine else 6)
    ref = RefScalars("replay_cosine" if cosine else "replay_l2")
    for rep in range(3000):
        obs, g, rows, f, v = _random_node(rng, rep)
        md = 0 if rep % 5 else int(rng.integers(0, 4))
        a = ref.next(lambda: oracle.ref_scores(obs, g, rows, f, v, md, cosine))
        b = oracle.replay_scores(obs, g, rows, f, v, md, cosine)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (rep, a, b, g.shape, len(rows))
    ref.finish()


@pytest.mark.parametrize("cosine", [True, False])
def test_categorical_scores_follow_the_same_sequence(cosine):
    """TreeNode::splitScoreCosineCategorical / splitScoreL2Categorical (node.cpp:253-319, 378-434) are separate functions of the reference: the
    compiler could have contracted their expressions differently.  It did not: same bits as the restated sequence on the equivalent 0/1 column."""
    rng = np.random.default_rng(3)
    ref = RefScalars("categorical_cosine" if cosine else "categorical_l2")
    for rep in range(1500):
        D, N = int(rng.integers(1, 41)), int(rng.integers(1, 500))
        sc = np.exp(rng.standard_normal() * 3)
        g = (rng.standard_normal((N, D)) * sc + (0.3 * sc if rep % 3 else 0)).astype(np.float32)
        tok = rng.integers(0, 3, N)
        cat = np.zeros((N, 1), "S128")
        cat[:, 0] = np.array([b"a", b"b", b"c"])[tok]
        rows = np.flatnonzero(rng.integers(0, 4, N) > 0).astype(np.int32)
        a = ref.next(lambda: (oracle.ref_split_score_cat(cat, g, rows, 0, b"a", 0, cosine),))[0]
        b = oracle.replay_scores((tok == 0).astype(np.float32).reshape(N, 1), g, rows, 0, 0.5, 0, cosine)[0]
        assert a.tobytes() == b.tobytes(), (rep, a, b)
    ref.finish()


@pytest.mark.parametrize("seed", [9894, 23064, 23089])
def test_restatement_takes_the_references_side_of_a_mirror_tie(seed):
    """Two-token categorical columns make mirror-image candidates ("== a" against "== b"): their scores tie exactly in exact arithmetic and the
    reference's asymmetric float32 expression decides (fma(norm_r, n_r, norm_l * n_l)).  The restatement evaluates that expression as the
    reference's build does (replay_sequence.cpp) -- before round 5 its own compiler's contraction decided, and these seeds came out the other way."""
    rng = np.random.default_rng(seed)
    case = dict(name="mirror", seed=seed, N=2500, F=0, Fc=2, D=int(rng.choice([1, 2])), depth=4, n_bins=4, score="Cosine", gen="Quantile", policy="greedy",
                trees=1, min_data_in_leaf=5, n_tokens=3)
    X, Xc, G, y = K.make_inputs(case)

    def reference(ref):
        a = ref.GBRL(**K.ctor_kwargs(case))
        K.drive(a, case, X, Xc, G, y)
        ea = a.get_ensemble_data()
        return {k: ea[k] for k in STRUCTURE_KEYS + VALUE_KEYS}
    ea = ref_arrays("mirror_%d" % seed, reference)
    b = oracle.OracleGBRL(**K.ctor_kwargs(case))
    K.drive(b, case, X, Xc, G, y)
    eb = b.get_ensemble_data()
    for k in STRUCTURE_KEYS + VALUE_KEYS:
        assert np.array_equal(np.asarray(ea[k]), eb[k]), k
