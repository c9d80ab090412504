"""Generate the categorical-ranking fixtures (catrank_*.npz) from the REFERENCE's own CPU path (oracle/_ref).  Authoring container only;
the reference never travels.

    OMP_NUM_THREADS=8 python tests/golden/make_catrank_golden.py            # all cases
    OMP_NUM_THREADS=8 python tests/golden/make_catrank_golden.py NAME ...   # selected cases

The rules are make_golden.py's: fixtures are defined at OMP_NUM_THREADS=8, the -march=x86-64-v3 and the -march=native builds must agree
byte for byte, and a case whose digest changes at 1 or 3 threads is rejected (pick another seed).  A fit case also stores the model after
a SECOND fit() on the grown model under `fit2_*`.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import cases as K  # noqa: E402
import catrank_cases as C  # noqa: E402
import make_golden as MG  # noqa: E402
import oracle  # noqa: E402


def run(mod, case):
    X, Xc, G, y = C.make_inputs(case)
    m = mod.GBRL(**K.ctor_kwargs(case))
    out = {}
    if "fit_iterations" in case:
        fit_loss, pred = K.drive_fit(m, case, X, y, Xc)
        out["fit_loss"] = np.float32(fit_loss)
        out["bias"] = np.array(m.get_bias(), np.float32)
    else:
        pred = K.drive(m, case, X, Xc, G, y)
    e = m.get_ensemble_data()
    out.update({k: np.array(e[k]) for k in K.ENSEMBLE_KEYS})
    out["pred"] = np.array(pred, np.float32)
    out["n_trees"] = np.int32(m.get_num_trees())
    out["iteration"] = np.int32(m.get_iteration())
    if "fit2_iterations" in case:
        # a second model: the reference segfaults when this fit() follows the inspection calls above on the same object
        m = mod.GBRL(**K.ctor_kwargs(case))
        K.drive_fit(m, case, X, y, Xc)
        out["fit2_loss"] = np.float32(m.fit(X, Xc, y, case["fit2_iterations"], False, "MultiRMSE"))
        e = m.get_ensemble_data()
        out.update({"fit2_" + k: np.array(e[k]) for k in K.ENSEMBLE_KEYS})
        out["fit2_pred"] = np.array(m.predict(X, Xc, 0, 0), np.float32)
        out["fit2_n_trees"] = np.int32(m.get_num_trees())
    out["inputs_sha256"] = np.array(K.inputs_digest(X, Xc, G, y))
    out["case_json"] = np.array(json.dumps(case))
    return out


def digest(a):
    import hashlib
    h = hashlib.sha256(MG.digest(a).encode())
    if "fit2_loss" in a:                                  # (a fit: structure only, see make_golden.digest)
        for k in MG.STRUCTURE_KEYS:
            h.update(np.ascontiguousarray(a["fit2_" + k]).tobytes())
    return h.hexdigest()


def main():
    ref = oracle.load_ref()
    assert ref is not None, "build oracle/_ref first: make -C oracle ref"
    if len(sys.argv) == 3 and sys.argv[1] == "--digest":     # child mode: print the digest under this OMP_NUM_THREADS
        print(digest(run(ref, C.BY_NAME[sys.argv[2]])))
        return
    assert os.environ.get("OMP_NUM_THREADS") == "8", "fixtures are defined at OMP_NUM_THREADS=8"
    nat = oracle.load_ref(native=True)
    assert nat is not None, "the -march=native reference build is missing"
    names = sys.argv[1:] or [c["name"] for c in C.STEP_CASES + C.FIT_CASES]
    for name in names:
        case = C.BY_NAME[name]
        a = run(ref, case)
        b = run(nat, case)
        keys = MG.STRUCTURE_KEYS if "fit_loss" in a else K.ENSEMBLE_KEYS + ("pred",)
        same = all(np.array_equal(a[k], b[k]) for k in keys)
        stable = True
        for th in ("1", "3"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", name], capture_output=True, text=True,
                                 env=dict(os.environ, OMP_NUM_THREADS=th))
            stable &= bool(out.stdout.strip()) and out.stdout.strip().splitlines()[-1] == digest(a)
        a["ref_stable_across_threads"] = np.bool_(stable)
        if not stable or not same:
            print(f"{name}: REJECTED -- native==v3: {same}, stable across OMP_NUM_THREADS in (1,3,8): {stable}; pick another seed")
            continue
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **a)
        sz = os.path.getsize(os.path.join(HERE, name + ".npz"))
        print(f"{name:22s} trees={int(a['n_trees'])} leaves={a['values'].shape[0]} categorical conditions={int((~a['is_numerics'].astype(bool)).sum())} "
              f"{sz/1024:.0f} KiB native==v3 thread-stable={stable}")


if __name__ == "__main__":
    main()
