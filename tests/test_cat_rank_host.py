"""The categorical-ranking fixtures (catrank_*.npz) without a GPU: their inputs regenerate from the seeds, they sit in the regime they are
meant to test (more distinct categories than Fc * n_bins), the reference agreed with itself when they were made, the categories the
reference's trees split on are among the Fc * n_bins with the largest mean squared gradient norm, and the oracle restatement of the
reference grows the same trees."""
import os

import numpy as np
import pytest

import cases as K
import catrank_cases as C
from helpers import GOLDEN, assert_structure_equal, rel_err


def _load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = C.BY_NAME[name]
    X, Xc, G, y = C.make_inputs(case)
    assert K.inputs_digest(X, Xc, G, y) == str(g["inputs_sha256"]), "input synthesis drifted from the fixture"
    return case, g, (X, Xc, G, y)


@pytest.mark.parametrize("name", sorted(C.BY_NAME))
def test_fixture_is_in_the_overflow_regime_and_was_stable(name):
    case, g, (X, Xc, G, y) = _load(name)
    distinct = sum(len(np.unique(Xc[:, f])) for f in range(case["Fc"]))
    assert distinct > case["Fc"] * case["n_bins"]
    assert bool(g["ref_stable_across_threads"])
    assert (~np.asarray(g["is_numerics"]).astype(bool)).any(), "no tree of the fixture splits on a category"
    if name == "catrank_ties":
        assert distinct >= 40                                                       # std::sort beyond its insertion-sort regime (16 elements)
        assert np.all(np.abs(G) == 1.0) and case["D"] == 4
    if "fit_iterations" in case:                                                     # MultiRMSE skips n_elements % n_threads elements
        assert (case["N"] * case["D"]) % 24 == 0 and (case["batch_size"] * case["D"]) % 24 == 0
        assert int(g["fit2_n_trees"]) == case["fit_iterations"] + case["fit2_iterations"] and case["fit2_iterations"] > case["fit_iterations"]


@pytest.mark.parametrize("name", ["catrank_grd_l2_q", "catrank_obl_cos_u"])
def test_reference_trees_split_only_on_the_top_ranked_categories(name):
    case, g, (X, Xc, G, y) = _load(name)
    keep = case["Fc"] * case["n_bins"]
    norm = np.zeros(case["N"], np.float64)
    for d in range(case["D"]):
        norm += G[:, d].astype(np.float64) ** 2
    means = {}
    for f in range(case["Fc"]):
        for tok in np.unique(Xc[:, f]):
            means[(f, bytes(tok))] = float(norm[Xc[:, f] == tok].mean())
    ranked = sorted(means, key=means.get, reverse=True)
    assert means[ranked[keep - 1]] - means[ranked[keep]] > 1e-4 * means[ranked[keep]], "the boundary of the kept set is a near-tie: pick another seed"
    kept = set(ranked[:keep])
    isnum = np.asarray(g["is_numerics"]).astype(bool).reshape(-1)
    fidx = np.asarray(g["feature_indices"]).reshape(-1)
    cats = np.asarray(g["categorical_values"]).reshape(-1)
    depths = np.asarray(g["depths"]).reshape(-1)
    MD, used = case["depth"], 0
    for row in range(len(depths)):
        for i in range(int(depths[row])):
            j = row * MD + i
            if not isnum[j]:
                tok = bytes(np.asarray(cats[j])).split(b"\0")[0]
                assert (int(fidx[j]), tok) in kept, (row, i, fidx[j], tok)
                used += 1
    assert used > 0


@pytest.mark.parametrize("name", [c["name"] for c in C.STEP_CASES])
def test_oracle_restatement_grows_the_fixture_trees(name):
    import oracle
    case, g, (X, Xc, G, y) = _load(name)
    r = oracle.OracleGBRL(**K.ctor_kwargs(case))
    pred = np.asarray(K.drive(r, case, X, Xc, G, y))
    assert_structure_equal(r.get_ensemble_data(), g)
    assert rel_err(pred, g["pred"], float(np.abs(G).mean())) <= 1e-5
