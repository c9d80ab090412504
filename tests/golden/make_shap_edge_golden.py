"""Generate tests/golden/shap_edge_*.npz: models whose (max_depth, output_dim) select every launch plan of the device TreeSHAP kernel, grown
by the REFERENCE's CPU path, with the reference's own tree_shap / ensemble_shap values.  Authoring container only.

    make -C oracle ref-small
    OMP_NUM_THREADS=8 python tests/golden/make_shap_edge_golden.py [case ...]

The capacity-only build is needed because the unpatched constructor cannot allocate these models (shap_edge_cases.py says which and why).
Each fixture is self-contained like the explain_*.npz ones: the reference's saved .gbrl_model bytes (the product LOADS it), the digest of
the synthesised inputs and the SHAP values of the first `shap_rows` rows -- the whole ensemble and the first, middle and last tree.  The
polynomial vectors are cases.poly_vectors(max_depth), checked here against the reference's own Python helper.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import cases as K  # noqa: E402
import oracle  # noqa: E402
import shap_edge_cases as S  # noqa: E402


def grow(mod, case, X, Xc, G):
    """cases.drive's setters, then one step per entry of shap_edge_cases.batches on that many leading rows."""
    F, Fc = case["F"], case.get("Fc", 0)
    m = mod.GBRL(**K.ctor_kwargs(case))
    m.set_feature_weights(np.ones(F + Fc, np.float32))
    for o in K.optimizers(case):
        m.set_optimizer(**o)
    m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))
    for n in S.batches(case):
        m.step(None if X is None else np.ascontiguousarray(X[:n]), None if Xc is None else np.ascontiguousarray(Xc[:n]),
               np.ascontiguousarray(G[:n].copy()))
    return m


def reference_poly_vectors():
    for modname in ("gbrl", "gbrl.common"):
        sys.modules.setdefault(modname, types.ModuleType(modname))
    for modname in ("config", "utils"):
        spec = importlib.util.spec_from_file_location("gbrl.common." + modname, "/root/reference/gbrl/common/%s.py" % modname)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["gbrl.common." + modname] = mod
        spec.loader.exec_module(mod)
    return sys.modules["gbrl.common.utils"].get_poly_vectors


def main():
    ref = oracle.load_ref_small()
    assert ref is not None, "build the capacity-only reference first: make -C oracle ref-small"
    assert os.environ.get("OMP_NUM_THREADS") == "8", "fixtures are defined at OMP_NUM_THREADS=8"
    get_poly_vectors = reference_poly_vectors()
    for name in (sys.argv[1:] or [c["name"] for c in S.CASES]):
        case = S.BY_NAME[name]
        X, Xc, G, y = K.make_inputs(case)
        m = grow(ref, case, X, Xc, G)
        base, norm, offset = K.poly_vectors(case["depth"])
        rb, rn, ro = get_poly_vectors(case["depth"], np.float32)
        assert np.array_equal(rb, base) and np.array_equal(rn, norm) and np.array_equal(ro, offset), "poly vectors differ"
        n = case["shap_rows"]
        xs = None if X is None else np.ascontiguousarray(X[:n])
        xcs = None if Xc is None else np.ascontiguousarray(Xc[:n])
        T = m.get_num_trees()
        assert T == case["trees"] <= 4
        out = dict(case_json=np.array(json.dumps(case)), inputs_sha256=np.array(K.inputs_digest(X, Xc, G, y)), n_trees=np.int32(T))
        for t in sorted({0, T // 2, T - 1}):
            out["shap_tree_%d" % t] = np.array(m.tree_shap(t, xs, xcs, norm, base, offset))
        out["shap_ensemble"] = np.array(m.ensemble_shap(xs, xcs, norm, base, offset))
        e = m.get_ensemble_data()
        depths = np.array(e["depths"])
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "m.gbrl_model")
            assert m.save(p) == 0
            out["model_file"] = np.frombuffer(open(p, "rb").read(), np.uint8)
        finite = all(np.isfinite(v).all() for k, v in out.items() if k.startswith("shap_"))
        path = os.path.join(HERE, "shap_edge_" + name + ".npz")
        np.savez_compressed(path, **out)
        print("%-26s max_depth=%-2d D=%-3d trees=%d depths %d..%d leaves=%-4d shap|max|=%-9.4g finite=%s %4.0f KiB" % (
            name, case["depth"], case["D"], T, depths.min(), depths.max(), np.array(e["values"]).shape[0], np.abs(out["shap_ensemble"]).max(),
            finite, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
