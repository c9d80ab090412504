"""Generate the Linear-scheduler fixtures (sched_*.npz, sched_recordings.npz) from the REFERENCE's own CPU path (oracle/_ref), which runs
SGD + Linear.  Authoring container only; the reference never travels.

    OMP_NUM_THREADS=8 python tests/golden/make_sched_golden.py            # all cases + the recordings
    OMP_NUM_THREADS=8 python tests/golden/make_sched_golden.py NAME ...   # selected cases

The rules are make_golden.py's: fixtures are defined at OMP_NUM_THREADS=8, the -march=x86-64-v3 and the -march=native builds must agree
byte for byte, and a case whose digest changes at 1 or 3 threads is rejected (pick another seed).  Beyond make_golden.py's arrays a
fixture may hold the reference's saved model file (`model_file`) and its exported header (`export_text`).
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import cases as K  # noqa: E402
import make_golden as MG  # noqa: E402
import oracle  # noqa: E402
import sched_cases as S  # noqa: E402


def run(mod, case):
    X, Xc, G, y = K.make_inputs(case)
    m = mod.GBRL(**K.ctor_kwargs(case))
    fit_loss = None
    if "fit_iterations" in case:
        fit_loss, pred = K.drive_fit(m, case, X, y, Xc)
    else:
        pred = K.drive(m, case, X, Xc, G, y)
    e = m.get_ensemble_data()
    out = {k: np.array(e[k]) for k in K.ENSEMBLE_KEYS}
    out["pred"] = np.array(pred, np.float32)
    for a, b in case.get("pred_ranges", []):
        out["pred_%d_%d" % (a, b)] = np.array(m.predict(X, Xc, a, b), np.float32)
    if fit_loss is not None:
        out["fit_loss"] = np.float32(fit_loss)
        out["bias"] = np.array(m.get_bias(), np.float32)
    out["n_trees"] = np.int32(m.get_num_trees())
    out["iteration"] = np.int32(m.get_iteration())
    out["scheduler_lrs"] = np.array(m.get_scheduler_lrs(), np.float32)
    out["inputs_sha256"] = np.array(K.inputs_digest(X, Xc, G, y))
    out["case_json"] = np.array(json.dumps(case))
    out["meta_json"] = np.array(json.dumps({k: (v if not isinstance(v, (np.generic,)) else v.item()) for k, v in m.get_metadata().items()}))
    with tempfile.TemporaryDirectory() as d:
        if case["name"] in S.MODEL_FILE_CASES:
            p = os.path.join(d, "m.gbrl_model")
            assert m.save(p) == 0
            out["model_file"] = np.frombuffer(open(p, "rb").read(), np.uint8)
        if case["name"] in S.EXPORT_CASES:
            # like make_explain_golden.py: the header comes from the model LOADED back by the reference -- the product loads the same file,
            # so both sides hold the same state (the header's comment prints the allocation size, which differs for a grown model)
            modelname, fmt, typ, prefix = S.EXPORT_CASES[case["name"]]
            p = os.path.join(d, "m.gbrl_model")
            assert m.save(p) == 0
            h = os.path.join(d, "m.h")
            assert mod.GBRL.load(p).export(h, modelname, fmt, typ, prefix) == 0
            out["export_text"] = np.frombuffer(open(h, "rb").read(), np.uint8)
    return out


def recordings(ref):
    out = {}
    rng = np.random.default_rng(7)
    X = K._normalish(rng, (64, 3))
    G = K._normalish(rng, (64, 2))
    for name, opts in S.LRS_SCHEDULES.items():
        m = ref.GBRL(**S.LRS_KW)
        m.set_feature_weights(np.ones(3, np.float32))
        for o in opts:
            m.set_optimizer(**o)
        m.set_feature_mapping(np.arange(3, dtype=np.int32), np.array([True] * 3, dtype=bool))
        lrs = [np.array(m.get_scheduler_lrs(), np.float32)]
        for _ in range(S.LRS_TREES):
            m.step(X, None, G.copy())
            lrs.append(np.array(m.get_scheduler_lrs(), np.float32))
        assert m.get_num_trees() == S.LRS_TREES
        out["lrs_" + name] = np.stack(lrs)
    m = ref.GBRL(**S.FRESH_KW)
    for o in S.FRESH_OPTS:
        m.set_optimizer(**o)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "fresh.gbrl_model")
        assert m.save(p) == 0
        out["fresh_model_file"] = np.frombuffer(open(p, "rb").read(), np.uint8)
    return out


def main():
    ref = oracle.load_ref()
    assert ref is not None, "build oracle/_ref first: make -C oracle ref"
    if len(sys.argv) == 3 and sys.argv[1] == "--digest":     # child mode: print the digest under this OMP_NUM_THREADS
        print(MG.digest(run(ref, S.BY_NAME[sys.argv[2]])))
        return
    assert os.environ.get("OMP_NUM_THREADS") == "8", "fixtures are defined at OMP_NUM_THREADS=8"
    nat = oracle.load_ref(native=True)
    assert nat is not None, "the -march=native reference build is missing"
    names = sys.argv[1:] or [c["name"] for c in S.CASES + S.FIT_CASES]
    for name in names:
        case = S.BY_NAME[name]
        a = run(ref, case)
        b = run(nat, case)
        same = all(np.array_equal(a[k], b[k]) for k in K.ENSEMBLE_KEYS + ("pred",))
        stable = True
        for th in ("1", "3"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", name], capture_output=True, text=True,
                                 env=dict(os.environ, OMP_NUM_THREADS=th))
            stable &= out.stdout.strip().splitlines()[-1] == MG.digest(a)
        a["ref_stable_across_threads"] = np.bool_(stable)
        if not stable or not same:
            print(f"{name}: REJECTED -- native==v3: {same}, stable across OMP_NUM_THREADS in (1,3,8): {stable}; pick another seed")
            continue
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **a)
        sz = os.path.getsize(os.path.join(HERE, name + ".npz"))
        print(f"{name:28s} trees={int(a['n_trees'])} leaves={a['values'].shape[0]} {sz/1024:.0f} KiB native==v3 thread-stable={stable}")
    if not sys.argv[1:]:
        np.savez_compressed(os.path.join(HERE, "sched_recordings.npz"), **recordings(ref))
        print("sched_recordings.npz")


if __name__ == "__main__":
    main()
