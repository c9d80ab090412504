"""fit_prepared with a classification objective (logistic, softmax) against the MultiRMSE loop, the same build; and objective_gradient alone.

    shapes   = 2^20 x 128 (T = 100), 65 536 x 128 (T = 1000), 4096 x 16 (T = 200); D = 8, depth 6, n_bins 256, oblivious / L2 / Quantile, lr 0.1
    legs     = a fresh model, fit_prepared(ds, targets, T, objective=o) for o in rmse, logistic, softmax; batch_size = n.  rmse and logistic fit the
               one-hot matrix of the labels, softmax the labels.  Two runs of every leg must leave byte-equal files before anything is timed.
    timing   = host clock around the call between two device synchronisations, medians of 10, the legs alternating in one process
    gradient = objective_gradient on device buffers at 2^20 x 8 and 2^20 x 128: time, and the bytes it must move per second

    python3 scripts/objective_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                      # failure; writes profiles/objective.txt (or FILE) when every shape has run
    python3 scripts/objective_sweep.py --shape NAME   # one shape, in this process
    python3 scripts/objective_sweep.py --gradient     # objective_gradient alone, in this process
    python3 scripts/objective_sweep.py --plain NAME [ROOT]   # only fit_prepared(ds, y, T) without the keyword, one JSON line: the leg that an
                                                      # earlier build (its tree at ROOT) runs too, alternated process by process by the caller
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, DEPTH, BINS = 8, 6, 256
# name: rows, features, iterations, time limit of the child (s)
SHAPES = {
    "2^20x128_T100": (1 << 20, 128, 100, 300),
    "65536x128_T1000": (65536, 128, 1000, 420),
    "4096x16_T200": (4096, 16, 200, 120),
}
LEGS = ("rmse", "logistic", "softmax")
REPS = 10


def setup(name, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, T, _ = SHAPES[name]

    def fresh(width=D):
        m = gbrl_amd.GBRL(input_dim=F, output_dim=width, policy_dim=width, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=rows, grow_policy="oblivious", verbose=0,
                          device="cuda", learner_name="sweep")
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=width)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(5)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    lab = torch.argmax(xt @ w + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32), dim=1).to(torch.int32).contiguous()
    onehot = torch.nn.functional.one_hot(lab.long(), D).to(torch.float32).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ds = fresh().prepare_dataset(tup(xt))
    targets = {"rmse": tup(onehot), "logistic": tup(onehot), "softmax": tup(lab)}
    return np, fresh, ds, targets, timed, (rows, F, T), (xt, lab, onehot)


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def run_plain(name, root):
    np, fresh, ds, targets, timed, (rows, F, T), _keep = setup(name, root)
    y = targets["rmse"]
    fresh().fit_prepared(ds, y, T)
    ms = []
    for _ in range(REPS):
        m = fresh()
        ms.append(timed(lambda: m.fit_prepared(ds, y, T)))
    print(json.dumps({"shape": name, "call": "fit_prepared(ds, y, T)", "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
                      "max_ms": round(max(ms), 3), "reps": REPS}), flush=True)
    return 0


def run(name):
    np, fresh, ds, targets, timed, (rows, F, T), _keep = setup(name, ROOT)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    kw = lambda o: {} if o == "rmse" else dict(objective=o)
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, REPS))
    files = {}
    for o in LEGS:
        a, b = fresh(), fresh()
        la, lb = a.fit_prepared(ds, targets[o], T, **kw(o)), b.fit_prepared(ds, targets[o], T, **kw(o))
        files[o] = file_bytes(a)
        same = files[o] == file_bytes(b) and np.float32(la).tobytes() == np.float32(lb).tobytes()
        print("    %-8s two runs, %d trees: %s   loss on all rows %.7g" % (o, a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", la))
        if not same:
            return 1
    named = fresh()
    named.fit_prepared(ds, targets["rmse"], T, objective="rmse")
    if file_bytes(named) != files["rmse"] or files["logistic"] == files["rmse"] or files["softmax"] == files["logistic"]:
        print("    objective='rmse' is NOT the call without the keyword, or two objectives left the same model")
        return 1
    print("    objective='rmse' leaves the bytes of fit_prepared(ds, y, T); the other objectives leave other models")
    ms = {o: [] for o in LEGS}
    for _ in range(REPS):
        for o in LEGS:
            m = fresh()
            ms[o].append(timed(lambda: m.fit_prepared(ds, targets[o], T, **kw(o))))
    spread = max(max(v) - min(v) for v in ms.values())
    for o in LEGS:
        print("    fit_prepared(objective=%-8s)  call %s   %.3f ms per iteration" % (o, fmt(ms[o]), med(ms[o]) / T))
    for o in LEGS[1:]:
        diff = med(ms[o]) - med(ms["rmse"])
        print("    %s / rmse: %.3f   %+.3f ms, %+.4f ms per iteration (spread between repeats %.3f ms: %s)" %
              (o, med(ms[o]) / med(ms["rmse"]), diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"), flush=True)
    return 0


def run_gradient():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n = 1 << 20
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    print("objective_gradient     %d rows, device buffers in and out, gradient and loss  [medians of %d, after two calls with equal bytes]" % (n, REPS))
    for width in (8, 128):
        m = gbrl_amd.GBRL(input_dim=4, output_dim=width, policy_dim=width, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=n, grow_policy="oblivious", verbose=0,
                          device="cuda", learner_name="sweep")
        torch.manual_seed(6)
        p = (4 * torch.randn(n, width, device="cuda:0", dtype=torch.float32)).contiguous()
        lab = torch.randint(0, width, (n,), device="cuda:0", dtype=torch.int32)
        onehot = torch.nn.functional.one_hot(lab.long(), width).to(torch.float32).contiguous()
        for o, t in (("rmse", onehot), ("logistic", onehot), ("softmax", lab)):
            ga, la = m.objective_gradient(tup(p), tup(t), o)
            gb, lb = m.objective_gradient(tup(p), tup(t), o)
            if not (torch.equal(torch.from_dlpack(ga), torch.from_dlpack(gb)) and np.float64(la).tobytes() == np.float64(lb).tobytes()):
                print("    D=%d %s: two calls DIFFER" % (width, o))
                return 1
            ms = []
            for _ in range(REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.objective_gradient(tup(p), tup(t), o)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            moved = 4 * n * width * 2 + t.numel() * 4   # scores in, gradient out, targets in
            print("    D=%-3d %-8s call %8.3f ms (min %8.3f max %8.3f)   %.1f MB that must move = %.0f GB/s   loss %.7g" %
                  (width, o, float(np.median(ms)), min(ms), max(ms), moved / 1e6, moved / 1e6 / float(np.median(ms)), la), flush=True)
    return 0


HEADER = """# python3 scripts/objective_sweep.py  -- one MI355X; each shape in its own process; targets are device tensors, the data set is prepared once
# legs = fit_prepared(ds, targets, T, objective=o) on a fresh model, o = rmse (the call without the keyword), logistic, softmax; batch_size = n
# rmse and logistic fit the one-hot matrix [n, 8] of the labels, softmax the int32 labels [n]
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
# objective_gradient = the call on device buffers (allocation of the result, the label check of softmax and the 8-byte loss read-back included)
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--gradient":
        return run_gradient()
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--plain":
        return run_plain(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "objective.txt")
    text, rc = HEADER, 0
    jobs = [(["--shape", name], SHAPES[name][3]) for name in SHAPES] + [(["--gradient"], 120)]
    for args, limit in jobs:
        child = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True)
        print(child.stdout, end="", flush=True)
        text += child.stdout
        rc = child.returncode
        if rc != 0:
            print("%s: exit status %d -- stopping" % (" ".join(args), rc), flush=True)
            break
    if rc == 0:
        with open(out_path, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
