"""fit_prepared(leaf_update="newton") against the gradient leaves of the same build; newton_leaves_prepared alone; trees to an equal validation loss.

    shapes   = 2^20 x 128 (T = 100), 65 536 x 128 (T = 1000), 4096 x 16 (T = 200); D = 8, depth 6, n_bins 256, oblivious / L2 / Quantile, lr 0.1
    legs     = a fresh model, fit_prepared(ds, targets, T, objective=o, leaf_update=u) for o in logistic, softmax and u in gradient, newton;
               batch_size = n.  Two runs of every leg must leave byte-equal files before anything is timed.
    timing   = host clock around the call between two device synchronisations, medians of 10, the legs alternating in one process; the
               newton_leaves phase (event pair around the memset, the launch and the read-back) from one more, profiled, run
    kernel   = newton_leaves_prepared on device buffers at 2^20 x 128, D = 8, one depth-6 tree: the streaming kernel and the general one
               (GBRL_HIP_CONTINUE_GENERIC=1), the newton_leaves phase as the time, and the bytes it must move per second
    trees    = the noisy linear rule of tests/test_gpu_fit_newton.py at 65 536 rows (F = 16, D = 1, depth 3, lr 0.1, leaf_l2 = 1, 16 384 validation
               rows): the validation loss of newton after k trees, and the gradient trees it takes to get there

    python3 scripts/newton_sweep.py [--out FILE]    # everything, each part in a child process of its own under a time limit; stops at the first
                                                    # failure; writes profiles/newton.txt (or FILE) when every part has run
    python3 scripts/newton_sweep.py --shape NAME    # one shape, in this process
    python3 scripts/newton_sweep.py --kernel        # newton_leaves_prepared alone
    python3 scripts/newton_sweep.py --trees         # trees to an equal validation loss
    python3 scripts/newton_sweep.py --plain NAME [ROOT]   # only fit_prepared(ds, y, T, objective="logistic") without the new keywords, one JSON line:
                                                    # the leg that an earlier build (its tree at ROOT) runs too, alternated process by process by the caller
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
    "2^20x128_T100": (1 << 20, 128, 100, 420),
    "65536x128_T1000": (65536, 128, 1000, 540),
    "4096x16_T200": (4096, 16, 200, 180),
}
OBJECTIVES = ("logistic", "softmax")
RULES = ("gradient", "newton")
REPS = 10


def make_model(gbrl_amd, np, F, width, rows, depth=DEPTH, bins=BINS):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=width, policy_dim=width, max_depth=depth, min_data_in_leaf=0, n_bins=bins, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=rows, grow_policy="oblivious", verbose=0,
                      device="cuda", learner_name="sweep")
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=width)
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def setup(name, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, T, _ = SHAPES[name]
    fresh = lambda: make_model(gbrl_amd, np, F, D, rows)
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
    targets = {"logistic": tup(onehot), "softmax": tup(lab)}
    return np, fresh, ds, targets, timed, (rows, F, T), (xt, lab, onehot)


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def run_plain(name, root):
    np, fresh, ds, targets, timed, (rows, F, T), _keep = setup(name, root)
    y = targets["logistic"]
    fresh().fit_prepared(ds, y, T, objective="logistic")
    ms = []
    for _ in range(REPS):
        m = fresh()
        ms.append(timed(lambda: m.fit_prepared(ds, y, T, objective="logistic")))
    print(json.dumps({"shape": name, "call": "fit_prepared(ds, y, T, objective='logistic')", "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
                      "max_ms": round(max(ms), 3), "reps": REPS}), flush=True)
    return 0


def run(name):
    np, fresh, ds, targets, timed, (rows, F, T), _keep = setup(name, ROOT)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    legs = [(o, u) for o in OBJECTIVES for u in RULES]
    kw = lambda o, u: dict(objective=o) if u == "gradient" else dict(objective=o, leaf_update=u, leaf_l2=1.0)
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, REPS))
    files = {}
    for o, u in legs:
        a, b = fresh(), fresh()
        la, lb = a.fit_prepared(ds, targets[o], T, **kw(o, u)), b.fit_prepared(ds, targets[o], T, **kw(o, u))
        files[(o, u)] = file_bytes(a)
        same = files[(o, u)] == file_bytes(b) and np.float32(la).tobytes() == np.float32(lb).tobytes()
        print("    %-8s %-8s two runs, %d trees: %s   loss on all rows %.7g" % (o, u, a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", la))
        if not same:
            return 1
    for o in OBJECTIVES:
        named = fresh()
        named.fit_prepared(ds, targets[o], T, objective=o, leaf_update="gradient")
        if file_bytes(named) != files[(o, "gradient")] or files[(o, "newton")] == files[(o, "gradient")]:
            print("    leaf_update='gradient' is NOT the call without the keyword, or newton left the gradient model")
            return 1
    print("    leaf_update='gradient' leaves the bytes of the call without the keyword; newton leaves another model")
    ms = {leg: [] for leg in legs}
    for _ in range(REPS):
        for o, u in legs:
            m = fresh()
            ms[(o, u)].append(timed(lambda: m.fit_prepared(ds, targets[o], T, **kw(o, u))))
    spread = max(max(v) - min(v) for v in ms.values())
    for o, u in legs:
        print("    fit_prepared(objective=%-8s, leaf_update=%-8s)  call %s   %.3f ms per iteration" % (o, u, fmt(ms[(o, u)]), med(ms[(o, u)]) / T))
    for o in OBJECTIVES:
        diff = med(ms[(o, "newton")]) - med(ms[(o, "gradient")])
        m = fresh()
        m.set_profiling(2)
        m.fit_prepared(ds, targets[o], T, **kw(o, "newton"))
        ph = dict(m.last_phase_times())
        print("    %s newton / gradient: %.3f   %+.3f ms, %+.4f ms per iteration (spread between repeats %.3f ms: %s);  newton_leaves phase of the last "
              "iteration %.4f ms, streaming kernel: %s" %
              (o, med(ms[(o, "newton")]) / med(ms[(o, "gradient")]), diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread",
               ph.get("newton_leaves", float("nan")), "yes" if ph.get("newton_streamed") == 1.0 else "no"), flush=True)
    return 0


def run_kernel():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n, F = 1 << 20, 128
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    print("newton_leaves_prepared   %d x %d, D = %d, one depth-%d tree (64 leaves), device buffers  [medians of %d, after two calls with equal bytes]" % (n, F, D, DEPTH, REPS))
    torch.manual_seed(7)
    xt = torch.randn(n, F, device="cuda:0", dtype=torch.float32)
    lab = torch.randint(0, D, (n,), device="cuda:0", dtype=torch.int32)
    onehot = torch.nn.functional.one_hot(lab.long(), D).to(torch.float32).contiguous()
    for o, t in (("logistic", onehot), ("softmax", lab)):
        m = make_model(gbrl_amd, np, F, D, n)
        ds = m.prepare_dataset(tup(xt))
        m.fit_prepared(ds, tup(t), 1, objective=o)
        pred = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).cuda().repeat(n, 1).contiguous()
        moved = n * (((F + 15) // 16) * 32 + 4 * D) + t.numel() * 4   # the code records, the prediction, the targets
        for generic in ("0", "1"):
            os.environ["GBRL_HIP_CONTINUE_GENERIC"] = generic
            ra = m.newton_leaves_prepared(ds, tup(pred), tup(t), o)
            rb = m.newton_leaves_prepared(ds, tup(pred), tup(t), o)
            if ra["sums"].tobytes() != rb["sums"].tobytes() or ra["values"].tobytes() != rb["values"].tobytes():
                print("    %s generic=%s: two calls DIFFER" % (o, generic))
                return 1
            m.set_profiling(2)
            dev, call = [], []
            for _ in range(REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.newton_leaves_prepared(ds, tup(pred), tup(t), o)
                torch.cuda.synchronize()
                call.append((time.perf_counter() - t0) * 1e3)
                ph = dict(m.last_phase_times())
                dev.append(ph["newton_leaves"])
            m.set_profiling(0)
            print("    %-8s %-9s newton_leaves phase %7.4f ms (min %7.4f max %7.4f)   call %7.3f ms   %.1f MB that must move = %.2f TB/s   rows summed %d" %
                  (o, "streaming" if ph["newton_streamed"] == 1.0 else "general", float(np.median(dev)), min(dev), max(dev), float(np.median(call)), moved / 1e6,
                   moved / 1e9 / float(np.median(dev)), int(ra["sums"][:, -1].sum())), flush=True)
        os.environ.pop("GBRL_HIP_CONTINUE_GENERIC", None)
    return 0


def run_trees():
    import numpy as np
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n, nv, F, Tg, Tn = 65536, 16384, 16, 600, 100
    rng = np.random.default_rng(20251)
    X = rng.standard_normal((n + nv, F)).astype(np.float32)
    w = rng.standard_normal(F).astype(np.float32)
    y = ((X @ w + rng.standard_normal(n + nv).astype(np.float32)) > 0).astype(np.float32)
    print("trees to an equal validation loss   %d rows (%d validation), F = %d, logistic D = 1, depth 3, lr 0.1, leaf_l2 = 1, labels from a noisy linear rule" % (n, nv, F))
    curves = {}
    for rule, T in (("gradient", Tg), ("newton", Tn)):
        m = make_model(gbrl_amd, np, F, 1, n, depth=3, bins=32)
        ds = m.prepare_dataset(X[:n])
        dsv = m.prepare_dataset(X[n:], reference=ds)
        curves[rule] = np.asarray(m.fit_prepared(ds, y[:n], T, valid=dsv, valid_targets=y[n:], objective="logistic", leaf_update=rule, leaf_l2=1.0)["valid_loss"])
    for k in (5, 10, 20, 50, 100):
        reach = np.nonzero(curves["gradient"] <= curves["newton"][k])[0]
        print("    newton after %3d trees: valid_loss %.6f   gradient reaches it after %s trees (gradient after %3d trees: %.6f)" %
              (k, curves["newton"][k], str(int(reach[0])) if reach.size else "more than %d" % Tg, k, curves["gradient"][k]), flush=True)
    return 0


HEADER = """# python3 scripts/newton_sweep.py  -- one MI355X; each part in its own process; targets are device tensors, the data set is prepared once
# legs = fit_prepared(ds, targets, T, objective=o[, leaf_update="newton", leaf_l2=1.0]) on a fresh model, o = logistic (the one-hot matrix [n, 8]), softmax (int32 labels [n])
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
# newton_leaves phase = an event pair around the memset of the accumulators, the launch and the enqueue of the read-back, in a profiled run of its own
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--kernel":
        return run_kernel()
    if len(sys.argv) == 2 and sys.argv[1] == "--trees":
        return run_trees()
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--plain":
        return run_plain(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "newton.txt")
    text, rc = HEADER, 0
    jobs = [(["--shape", name], SHAPES[name][3]) for name in SHAPES] + [(["--kernel"], 180), (["--trees"], 180)]
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
