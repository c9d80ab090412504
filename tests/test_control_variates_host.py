"""Control variates without a device: gbrl_cpp.control_variates_host (gbrl_amd/csrc/cv_core.h has the rule) against NumPy, the refusals, the no-trees
case, the launch plan, and tests/cxx/cv_core_check.cpp under the host sanitizers.  tests/test_gpu_control_variates.py imports cv_chain, cv_statistics
and check_result from here, and checks the chain itself over the leaves predict_leaves reports (no call routes rows without a device).

Bounds: momentum and grads are equalities of bytes (NumPy float32 restates every operation).  scale: one float32 ulp (the host powf is the only
freedom).  alpha: one float32 ulp of the float64 value rounded once -- the gradients are 0.7 ms + 0.3 noise, so the covariance sum has no cancellation
and the float64 summation error n 2^-53 is far below a float32 ulp."""
import os
import subprocess

import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def cv_chain(values, leaves, shape, beta, momentum=None, start=0):
    """the raw momentum [n, D]: three float32 operations per tree over values[leaves] (leaves int [n, T]; -1 ends a row's walk)"""
    beta, c = f32(beta), f32(1) - f32(beta)
    m = np.zeros(shape, f32) if momentum is None else momentum.astype(f32).reshape(shape).copy()
    alive = np.ones(shape[0], bool)
    for t in range(start, leaves.shape[1]):
        alive &= leaves[:, t] >= 0
        v = values[np.maximum(leaves[:, t], 0)].reshape(shape)
        m[alive] = ((beta * m).astype(f32) + (c * v).astype(f32)).astype(f32)[alive]
    return m


def cv_statistics(m, G, beta, T):
    """scale (float32) and alpha (float64 sums, each result rounded once) from the raw momentum m and the gradients G, both [n, D]"""
    scale = f32(1) / np.sqrt(f32(1) - np.power(f32(beta), f32(T), dtype=f32), dtype=f32)
    ms, n = (m * scale).astype(f32), len(G)
    mc = (ms - (ms.astype(np.float64).sum(0) / n).astype(f32)).astype(f32).astype(np.float64)
    gc = (G - (G.astype(np.float64).sum(0) / n).astype(f32)).astype(f32).astype(np.float64)
    var, cov = ((mc * mc).sum(0) / (n - 1)).astype(f32), ((gc * mc).sum(0) / (n - 1)).astype(f32)
    return scale, np.clip((cov / (var + f32(1e-8)).astype(f32)).astype(f32), -1, 1)


def ulps(a, b):
    return np.abs(np.asarray(a, f32).view(np.int32).astype(np.int64) - np.asarray(b, f32).view(np.int32).astype(np.int64)).max()


def check_result(r, G, T, what, m_ref=None):
    """what every form must satisfy: (momentum bytes,) scale and alpha within an ulp of NumPy, grads recomputed from the RETURNED statistics"""
    G2 = G.reshape(len(G), -1)
    m = np.asarray(r["momentum"]).reshape(G2.shape)
    assert m_ref is None or m.tobytes() == m_ref.tobytes(), what
    scale, alpha = cv_statistics(m, G2, 0.9, T)
    assert ulps(r["scale"], scale) <= 1 and ulps(r["alpha"], alpha) <= 1, (what, r["scale"], scale, r["alpha"], alpha)
    mc = ((m * f32(r["scale"])).astype(f32) - r["mean_momentum"][None]).astype(f32)
    assert np.asarray(r["grads"]).tobytes() == (G2 - (mc * r["alpha"][None]).astype(f32)).astype(f32).tobytes(), what


def _loaded(name, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


@pytest.mark.parametrize("name", ["obl_l2_q", "explain_obl_l2_q_d6", "grd_cos_q_ac", "sched_grd_cos_q_ac"])
@pytest.mark.parametrize("n", [2, 97, 130])
def test_host_rule_against_numpy(name, n, tmp_path):
    m = _loaded(name, tmp_path)
    md = m.get_metadata()
    D, T = md["output_dim"], m.get_num_trees()
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, md["input_dim"])).astype(f32)
    shape = (n,) if D == 1 else (n, D)
    r0 = cpp.control_variates_host(m, X, np.zeros(shape, f32), beta=0.9)
    ms = (np.asarray(r0["momentum"]) * f32(r0["scale"])).astype(f32)
    G = (0.7 * ms + 0.3 * rng.standard_normal(shape)).astype(f32)
    r = cpp.control_variates_host(m, X, G, beta=0.9)
    assert r["n_trees"] == T and np.asarray(r["grads"]).shape == G.shape and np.asarray(r["momentum"]).tobytes() == np.asarray(r0["momentum"]).tobytes()
    check_result(r, G, T, name)
    c = cpp.control_variates_host(m, X, G, beta=0.9, momentum=np.asarray(r["momentum"]), start_tree_idx=T)   # nothing left to walk: the statistics alone
    for key in ("grads", "momentum", "alpha", "var", "cov"):
        assert np.asarray(c[key]).tobytes() == np.asarray(r[key]).tobytes(), key
    clipped = cpp.control_variates_host(m, X, (3 * ms).astype(f32), beta=0.9)
    assert (clipped["alpha"][np.asarray(clipped["var"]) > 1e-6] == 1.0).all()


def test_no_trees_constant_momentum_and_refusals(tmp_path):
    empty = gbrl_amd.GBRL(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")
    empty.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2)
    X, G = np.zeros((5, 4), f32), np.arange(10, dtype=f32).reshape(5, 2)
    r = cpp.control_variates_host(empty, X, G)
    assert r["grads"].tobytes() == G.tobytes() and not r["momentum"].any() and not r["alpha"].any() and r["n_trees"] == 0
    m = _loaded("obl_l2_q", tmp_path)
    md = m.get_metadata()
    F, D = md["input_dim"], md["output_dim"]
    X = np.tile(np.random.default_rng(1).standard_normal((1, F)).astype(f32), (9, 1))   # all rows equal: constant momentum
    G = np.random.default_rng(2).standard_normal((9, D)).astype(f32)
    G = G[:, 0].copy() if D == 1 else G
    r = cpp.control_variates_host(m, X, G)
    assert not r["var"].any() and not r["alpha"].any() and r["grads"].tobytes() == G.tobytes()
    for kw, text in ((dict(beta=0.0), "beta must lie in"), (dict(beta=1.0), "beta must lie in"), (dict(beta=float("nan")), "beta must lie in"),
                     (dict(start_tree_idx=m.get_num_trees() + 1), "start_tree_idx"), (dict(start_tree_idx=-1), "start_tree_idx"),
                     (dict(momentum=np.zeros((8, D), f32)), "momentum")):
        with pytest.raises(RuntimeError, match=text):
            cpp.control_variates_host(m, X, G, **kw)
    with pytest.raises(RuntimeError, match="at least 2 rows"):
        cpp.control_variates_host(m, X[:1], G[:1])
    bad = G.copy()
    bad.flat[0] = np.inf
    with pytest.raises(RuntimeError, match="is not finite"):
        cpp.control_variates_host(m, X + np.arange(9, dtype=f32)[:, None], bad)
    cat = _loaded("obl_l2_q_cat", tmp_path)
    with pytest.raises(RuntimeError, match="categorical columns"):
        cat.control_variates_prepared(None, np.zeros((9, cat.get_metadata()["output_dim"]), f32))
    with pytest.raises(RuntimeError, match="null data set"):
        m.control_variates_prepared(None, G)


def test_geometry_and_cv_core_check_under_the_sanitizers(tmp_path):
    g = cpp.control_variates_geometry(130, 20, False, 3)
    assert g == {"streaming": True, "dmax": 4, "walk_trees": 16, "value_trees": 8, "walk_slots": 3, "moment_slots": 3, "launches": 4, "lds_bytes": 64 * 21 * 4}
    assert cpp.control_variates_geometry(1 << 20, 8, True, 8)["moment_slots"] == 2048 and cpp.control_variates_geometry(1 << 20, 8, True, 8)["lds_bytes"] == 64 * 65 * 4
    assert not cpp.control_variates_geometry(130, 20, False, 96)["streaming"] and not cpp.control_variates_geometry(130, 1 << 20, False, 3)["streaming"]
    exe = tmp_path / "cv_core_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gbrl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "cv_core_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "all sections passed" in out.stdout, out.stdout + out.stderr
