"""fit_prepared(weights=) against the same call without weights in one build; newton_leaves_prepared and objective_gradient alone; what
down-weighting mislabelled rows buys.

    shapes   = 2^20 x 128 (T = 100), 65 536 x 128 (T = 1000), 4096 x 16 (T = 200); D = 8, depth 6, n_bins 256, oblivious / L2 / Quantile, lr 0.1
    legs     = a fresh model, fit_prepared(ds, targets, T, objective=o, leaf_update=u[, weights=w]) for (o, u) in (rmse, gradient), (softmax, gradient),
               (softmax, newton); batch_size = n; w uniform in [0, 2) (mean 1), a device tensor.  Two runs of every leg must leave byte-equal files
               before anything is timed, and all-ones weights must leave the bytes of the call without the keyword.
    timing   = host clock around the call between two device synchronisations, medians of 10, the legs alternating in one process
    kernel   = newton_leaves_prepared and objective_gradient on device buffers at 2^20 x 128, D = 8, with and without weights
    curves   = the noisy linear rule of profiles/newton.txt (65 536 rows, F = 16, logistic D = 1, depth 3, lr 0.1, 16 384 clean validation rows) with
               30 % of the training labels flipped: the clean validation loss of an unweighted fit and of a fit with those rows at weight 0.05

    python3 scripts/weights_sweep.py [--out FILE]    # everything, each part in a child process of its own under a time limit; stops at the first
                                                     # failure; writes profiles/weights.txt (or FILE) when every part has run
    python3 scripts/weights_sweep.py --shape NAME    # one shape, in this process
    python3 scripts/weights_sweep.py --kernel        # the two stand-alone calls
    python3 scripts/weights_sweep.py --curves        # what weighting buys
    python3 scripts/weights_sweep.py --plain NAME [ROOT]   # only the calls without the new keywords, one JSON line each: the legs that an earlier build
                                                     # (its tree at ROOT) runs too, alternated process by process by the caller
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
LEGS = (("rmse", "gradient"), ("softmax", "gradient"), ("softmax", "newton"))
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
    score = xt @ w + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    lab = torch.argmax(score, dim=1).to(torch.int32).contiguous()
    real = score.contiguous()
    wt = (2.0 * torch.rand(rows, device="cuda:0", dtype=torch.float32)).contiguous()
    ones = torch.ones(rows, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ds = fresh().prepare_dataset(tup(xt))
    targets = {"rmse": tup(real), "softmax": tup(lab)}
    return np, fresh, ds, targets, tup(wt), tup(ones), timed, (rows, F, T), (xt, lab, real, wt, ones)


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def leg_kw(o, u):
    kw = {} if o == "rmse" else dict(objective=o)
    if u != "gradient":
        kw.update(leaf_update=u, leaf_l2=1.0)
    return kw


def run_plain(name, root):
    np, fresh, ds, targets, _w, _ones, timed, (rows, F, T), _keep = setup(name, root)
    for o in ("rmse", "softmax"):
        kw = leg_kw(o, "gradient")
        fresh().fit_prepared(ds, targets[o], T, **kw)
        ms = []
        for _ in range(REPS):
            m = fresh()
            ms.append(timed(lambda: m.fit_prepared(ds, targets[o], T, **kw)))
        print(json.dumps({"shape": name, "call": "fit_prepared(ds, y, T%s)" % ("" if o == "rmse" else ", objective='softmax'"), "median_ms": round(float(np.median(ms)), 3),
                          "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": REPS}), flush=True)
    return 0


def run(name):
    np, fresh, ds, targets, w, ones, timed, (rows, F, T), _keep = setup(name, ROOT)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, REPS))
    legs = [(o, u, wk) for o, u in LEGS for wk in ("none", "weights")]
    call = lambda m, o, u, wk: m.fit_prepared(ds, targets[o], T, **leg_kw(o, u), **({} if wk == "none" else dict(weights=w)))
    files = {}
    for o, u, wk in legs:
        a, b = fresh(), fresh()
        la, lb = call(a, o, u, wk), call(b, o, u, wk)
        files[(o, u, wk)] = file_bytes(a)
        same = files[(o, u, wk)] == file_bytes(b) and np.float32(la).tobytes() == np.float32(lb).tobytes()
        print("    %-8s %-8s %-8s two runs, %d trees: %s   loss on all rows %.7g" % (o, u, wk, a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", la))
        if not same:
            return 1
    for o, u in LEGS:
        one = fresh()
        one.fit_prepared(ds, targets[o], T, **leg_kw(o, u), weights=ones)
        if file_bytes(one) != files[(o, u, "none")] or files[(o, u, "weights")] == files[(o, u, "none")]:
            print("    all-ones weights are NOT the call without the keyword, or the weights left the unweighted model")
            return 1
    print("    all-ones weights leave the bytes of the call without the keyword; the weights leave another model")
    ms = {leg: [] for leg in legs}
    for _ in range(REPS):
        for o, u, wk in legs:
            m = fresh()
            ms[(o, u, wk)].append(timed(lambda: call(m, o, u, wk)))
    spread = max(max(v) - min(v) for v in ms.values())
    for o, u, wk in legs:
        print("    fit_prepared(objective=%-8s, leaf_update=%-8s, weights=%-7s)  call %s   %.3f ms per iteration" %
              (o, u, "w" if wk == "weights" else "None", fmt(ms[(o, u, wk)]), med(ms[(o, u, wk)]) / T))
    for o, u in LEGS:
        a, b = ms[(o, u, "weights")], ms[(o, u, "none")]
        diff = med(a) - med(b)
        print("    %s %s weighted / unweighted: %.4f   %+.3f ms, %+.5f ms per iteration (spread between repeats %.3f ms: %s)" %
              (o, u, med(a) / med(b), diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"), flush=True)
    return 0


def run_kernel():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n, F = 1 << 20, 128
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    print("stand-alone calls   %d x %d, D = %d, device buffers  [medians of %d, weighted and unweighted alternating, after two calls with equal bytes]" % (n, F, D, REPS))
    torch.manual_seed(7)
    xt = torch.randn(n, F, device="cuda:0", dtype=torch.float32)
    lab = torch.randint(0, D, (n,), device="cuda:0", dtype=torch.int32)
    real = torch.randn(n, D, device="cuda:0", dtype=torch.float32)
    wt = (2.0 * torch.rand(n, device="cuda:0", dtype=torch.float32)).contiguous()
    med = lambda a: float(np.median(a))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    m = make_model(gbrl_amd, np, F, D, n)
    ds = m.prepare_dataset(tup(xt))
    m.fit_prepared(ds, tup(lab), 1, objective="softmax")
    pred = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).cuda().repeat(n, 1).contiguous()
    # newton_leaves_prepared: the newton_leaves phase (memset, launch, read-back) and the call
    ra = m.newton_leaves_prepared(ds, tup(pred), tup(lab), "softmax", weights=tup(wt))
    rb = m.newton_leaves_prepared(ds, tup(pred), tup(lab), "softmax", weights=tup(wt))
    if ra["sums"].tobytes() != rb["sums"].tobytes() or ra["values"].tobytes() != rb["values"].tobytes():
        print("    newton_leaves_prepared(weights=): two calls DIFFER")
        return 1
    m.set_profiling(2)
    dev, call = {"none": [], "weights": []}, {"none": [], "weights": []}
    for _ in range(REPS):
        for wk in ("none", "weights"):
            kw = {} if wk == "none" else dict(weights=tup(wt))
            call[wk].append(timed(lambda: m.newton_leaves_prepared(ds, tup(pred), tup(lab), "softmax", **kw)))
            dev[wk].append(dict(m.last_phase_times())["newton_leaves"])
    m.set_profiling(0)
    for wk in ("none", "weights"):
        print("    newton_leaves_prepared softmax weights=%-7s newton_leaves phase %7.4f ms (min %7.4f max %7.4f)   call %7.3f ms (min %7.3f max %7.3f)" %
              ("w" if wk == "weights" else "None", med(dev[wk]), min(dev[wk]), max(dev[wk]), med(call[wk]), min(call[wk]), max(call[wk])))
    print("    weighted / unweighted: phase %.4f, call %.4f (the call with weights also runs the statistics kernel, its finishing sum and a 16-byte read-back)" %
          (med(dev["weights"]) / med(dev["none"]), med(call["weights"]) / med(call["none"])), flush=True)
    # objective_gradient: the call (device in, device out)
    for o, t in (("rmse", real), ("softmax", lab)):
        ga, la = m.objective_gradient(tup(pred), tup(t), o, weights=tup(wt))
        gb, lb = m.objective_gradient(tup(pred), tup(t), o, weights=tup(wt))
        if not torch.equal(torch.from_dlpack(ga), torch.from_dlpack(gb)) or np.float64(la).tobytes() != np.float64(lb).tobytes():
            print("    objective_gradient(weights=): two calls DIFFER")
            return 1
        del ga, gb
        call = {"none": [], "weights": []}
        for _ in range(REPS):
            for wk in ("none", "weights"):
                kw = {} if wk == "none" else dict(weights=tup(wt))
                call[wk].append(timed(lambda: m.objective_gradient(tup(pred), tup(t), o, **kw)))
        for wk in ("none", "weights"):
            print("    objective_gradient %-8s weights=%-7s call %7.3f ms (min %7.3f max %7.3f)" % (o, "w" if wk == "weights" else "None", med(call[wk]), min(call[wk]), max(call[wk])))
        print("    weighted / unweighted: call %.4f (with weights: the statistics kernel, its finishing sum and a 16-byte read-back in front of the launch)" %
              (med(call["weights"]) / med(call["none"])), flush=True)
    return 0


def run_curves():
    import numpy as np
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n, nv, F, T = 65536, 16384, 16, 100
    rng = np.random.default_rng(20251)
    X = rng.standard_normal((n + nv, F)).astype(np.float32)
    w = rng.standard_normal(F).astype(np.float32)
    y = ((X @ w + rng.standard_normal(n + nv).astype(np.float32)) > 0).astype(np.float32)
    flipped = rng.random(n) < 0.3
    noisy = np.where(flipped, 1.0 - y[:n], y[:n]).astype(np.float32)
    weights = np.where(flipped, 0.05, 1.0).astype(np.float32)
    print("what weighting buys   %d rows (%d clean validation rows), F = %d, logistic D = 1, depth 3, lr 0.1, newton leaves (leaf_l2 = 1), labels from a noisy linear rule, "
          "%d training labels flipped (30 %%)" % (n, nv, F, int(flipped.sum())))
    curves = {}
    for name, kw in (("unweighted", {}), ("flipped rows at weight 0.05", dict(weights=weights)), ("clean labels (the ceiling)", None)):
        m = make_model(gbrl_amd, np, F, 1, n, depth=3, bins=32)
        ds = m.prepare_dataset(X[:n])
        dsv = m.prepare_dataset(X[n:], reference=ds)
        tar = y[:n] if kw is None else noisy
        r = m.fit_prepared(ds, np.ascontiguousarray(tar), T, valid=dsv, valid_targets=np.ascontiguousarray(y[n:]), objective="logistic", leaf_update="newton", leaf_l2=1.0,
                           eval_metric="error", **(kw or {}))
        curves[name] = (np.asarray(r["valid_loss"]), np.asarray(r["valid_metric"]))
    for name, (loss, err) in curves.items():
        print("    %-28s clean valid_loss after 0 5 10 20 50 100 trees: %s   error rate after 100: %.4f   lowest loss %.6f at %d trees" %
              (name, " ".join("%.6f" % loss[k] for k in (0, 5, 10, 20, 50, 100)), err[100], loss.min(), int(loss.argmin())), flush=True)
    return 0


HEADER = """# python3 scripts/weights_sweep.py  -- one MI355X; each part in its own process; targets and weights are device tensors, the data set is prepared once
# legs = fit_prepared(ds, targets, T[, objective="softmax"][, leaf_update="newton", leaf_l2=1.0][, weights=w]) on a fresh model; rmse targets float32 [n, 8], softmax int32 labels [n];
#        w = 2 * uniform[0, 1) (mean 1), float32 [n]
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--kernel":
        return run_kernel()
    if len(sys.argv) == 2 and sys.argv[1] == "--curves":
        return run_curves()
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--plain":
        return run_plain(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "weights.txt")
    text, rc = HEADER, 0
    jobs = [(["--shape", name], SHAPES[name][3]) for name in SHAPES] + [(["--kernel"], 180), (["--curves"], 180)]
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
