"""Path attribution (Saabas) without a device: gbrl_cpp.path_contrib_host / path_expected_host (gbrl_amd/csrc/path_core.h has the rule) against a
float64 NumPy walk over get_ensemble_data(), the slot plan, the refusals, the hook table, and tests/cxx/path_core_check.cpp under the host
sanitizers.  The calls on a data set run in tests/test_gpu_path_contrib.py, which imports path_reference from here.

The bound per element is c * 2^-23 * S + 2^-23 * |phi|, c the number of terms and S the sum of their magnitudes: the float32 adds and the one
rounding of each delta.  predict has no CPU path: additivity is checked here against the float64 prediction of the same walk, on the GPU against predict."""
import os
import re
import subprocess

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23


def _rate(o, t):
    f = np.float32   # scheduler_lr: every operation rounds to float32
    if o["scheduler_func"] != "Linear":
        return float(f(o["init_lr"]))
    left = (f(o["T"]) - (f(t) + f(1))) / f(o["T"])
    return float(max(f(o["init_lr"]) + (f(1) - left) * (f(o["stop_lr"]) - f(o["init_lr"])), f(o["stop_lr"])))


def path_reference(m, X, n_trees=None):
    """float64: phi [n, F, D], S = sum |terms| [n, F, D], the term count c [n, F, 1], expected [D] and the prediction [n, D] of the trees [0, n_trees)"""
    e, opts, obl = m.get_ensemble_data(), m.get_optimizers(), m.get_metadata()["grow_policy"] == "Oblivious"
    ti, dep, fi, fv, dirs = (np.asarray(e[k]) for k in ("tree_indices", "depths", "feature_indices", "feature_values", "inequality_directions"))
    val, ew = np.asarray(e["values"], np.float64), np.asarray(e["edge_weights"], np.float64)
    (n, F), D, L = X.shape, val.shape[1], len(val)
    phi, S, c = np.zeros((n, F, D)), np.zeros((n, F, D)), np.zeros((n, F, 1))
    expected = np.asarray(e["bias"], np.float64).copy()
    pred = np.tile(expected, (n, 1))
    for t in range(len(ti) if n_trees is None else n_trees):
        l0, l1 = ti[t], ti[t + 1] if t + 1 < len(ti) else L
        lr = np.array([sum(_rate(o, t) for o in opts if o["start_idx"] <= d < o["stop_idx"]) for d in range(D)])
        row = (lambda l: t) if obl else (lambda l: l)
        cover = {l: np.prod(ew[l, :dep[row(l)]]) for l in range(l0, l1)}

        def E(l, j):   # the node at depth j above leaf l: the leaves that share its first j decisions
            if j == dep[row(l)]:
                return val[l]
            below = [q for q in range(l0, l1) if dep[row(q)] >= j and (dirs[q, :j] == dirs[l, :j]).all()]
            w = np.array([cover[q] for q in below])
            return (w[:, None] * val[below]).sum(0) / w.sum() if w.sum() > 0 else np.zeros(D)   # (a node no training row reached)

        expected += -lr * E(l0, 0)
        passed = X[:, fi[[row(l) for l in range(l0, l1)]]] > fv[[row(l) for l in range(l0, l1)]][None]          # [n, leaves, depth]
        for k, l in enumerate(range(l0, l1)):
            k_l = dep[row(l)]
            here = (passed[:, k, :k_l] == (dirs[l, :k_l] != 0)[None]).all(1)
            pred[here] += -lr * val[l]
            for j in range(k_l):
                term = -lr * (E(l, j + 1) - E(l, j))
                f = fi[row(l), j]
                phi[here, f] += term
                S[here, f] += np.abs(term)
                c[here, f] += 1
    return phi, S, c, expected, pred


def _loaded(name, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


@pytest.mark.parametrize("name,n_trees", [("obl_l2_q", None), ("explain_obl_l2_q_d6", None), ("grd_cos_q_ac", None), ("sched_obl_l2_q", None),
                                          ("sched_grd_cos_q_ac", None), ("sched_grd_cos_q_ac", 5)])
def test_host_rule_against_the_float64_walk(name, n_trees, tmp_path):
    m = _loaded(name, tmp_path)
    F = m.get_metadata()["input_dim"]
    X = np.random.default_rng(7).standard_normal((97, F)).astype(np.float32)
    got, expected = cpp.path_contrib_host(m, X, n_trees), cpp.path_expected_host(m, n_trees)
    phi, S, c, want_expected, pred = path_reference(m, X, n_trees)
    assert got.dtype == np.float32 and got.shape == phi.shape and expected.dtype == np.float64
    bound = c * EPS * S + EPS * np.abs(phi)
    err = np.abs(got.astype(np.float64) - phi)
    print("%s: max error %.3g, bound there %.3g, max |phi| %.3g, terms up to %d" % (name, err.max(), bound.flat[err.argmax()], np.abs(phi).max(), c.max()))
    assert (err <= bound).all() and np.abs(phi).max() > 0
    assert np.abs(expected - want_expected).max() <= 1e-12 * (1 + np.abs(want_expected).max())
    # additivity: the contributions of a row and the expected value are its prediction, within the summed bounds
    assert (np.abs(got.astype(np.float64).sum(1) + expected - pred) <= bound.sum(1) + 1e-12 * (1 + np.abs(pred))).all()
    unused = (c.sum((0, 2)) == 0)
    assert not got[:, unused].view(np.uint32).any()            # a column no tree tests: exact (positive) zeros


def test_refusals(tmp_path):
    m = _loaded("obl_l2_q", tmp_path)
    for bad in (0, 4, -2):
        with pytest.raises(RuntimeError, match=r"path_contrib_host: n_trees %d is outside \[1, 3\]" % bad):
            cpp.path_contrib_host(m, np.zeros((4, 8), np.float32), bad)
    empty = gbrl_amd.GBRL(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    empty.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2)
    with pytest.raises(RuntimeError, match="the model has no trees"):
        cpp.path_contrib_host(empty, np.zeros((4, 4), np.float32))
    cat = _loaded("obl_l2_q_cat", tmp_path)
    with pytest.raises(RuntimeError, match="not available on a model with categorical columns"):
        cpp.path_expected_host(cat)
    for model, text in ((m, "null data set"), (cat, "not available on a model with categorical columns")):   # the calls on a data set, without a device
        for call in (model.path_contrib_prepared, model.path_importance_prepared):
            with pytest.raises(RuntimeError, match=text):
                call(None)


def test_path_generic_hook_is_in_the_table_and_documented():
    names = re.findall(r"^\s+X\(([A-Z0-9_]+)\)", open(os.path.join(ROOT, "gbrl_amd", "csrc", "hooks.h")).read(), re.M)
    assert "PATH_GENERIC" in names and names == sorted(names)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`GBRL_HIP_PATH_GENERIC=1`" in doc[doc.index("## 5"):]
    assert "path_importance_prepared" in doc[doc.index("## 4"):doc.index("## 5")]
    assert "hooks::PATH_GENERIC" in open(os.path.join(ROOT, "gbrl_amd", "csrc", "engine_path.hip")).read()


def test_path_core_check_runs_clean_under_the_sanitizers(tmp_path):
    exe, csrc = tmp_path / "path_core_check", os.path.join(ROOT, "gbrl_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cxx", "path_core_check.cpp"), os.path.join(csrc, "model.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "all sections passed" in out.stdout, out.stdout + out.stderr
