"""The classifier metrics (eval_metric: error, auc): the cost of one evaluation on device buffers, and of fit_prepared watched by one.

    eval     = GBRL.eval_metric(pred, targets, "logistic", metric) on device buffers at 2^20 x 8 and 262 144 x 8, metric = error, auc: two calls
               with equal bytes first, then medians of 10; ms, and for auc the TB/s of the sort's traffic (16 n D bytes x 4 passes)
    fit      = fit_prepared(ds, y, 100, valid=dsv, valid_targets=yv, objective="logistic", eval_metric=e), e = None, "error", "auc", on a fresh
               model: 2^20 x 128 training rows, 262 144 validation rows, D = 8, depth 6, n_bins 256, batch_size = n.  Two runs of every leg must
               leave byte-equal files and curves -- and every leg the same file -- before anything is timed; medians of 10, the legs alternating
               in one process
    timing   = host clock around the call between two device synchronisations

    python3 scripts/metric_sweep.py [--parent ROOT] [--out FILE]   # both parts, each in a child process under a time limit; stops at the first
                                                      # failure; writes profiles/metric.txt (or FILE).  --parent ROOT: the tree of an earlier build;
                                                      # its fit_prepared(objective="logistic", valid=...) and this build's eval_metric=None leg
                                                      # are then timed alternating process by process, twice each
    python3 scripts/metric_sweep.py --eval | --fit    # one part, in this process
    python3 scripts/metric_sweep.py --plain [ROOT]    # the leg without eval_metric only, one JSON line
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, DEPTH, BINS = 8, 6, 256
ROWS, VROWS, F, T = 1 << 20, 262144, 128, 100
REPS = 10
LEGS = (None, "error", "auc")


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def setup_fit(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gbrl_amd

    def fresh():
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=ROWS, grow_policy="oblivious", verbose=0,
                          device="cuda", learner_name="sweep")
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(7)
    xt = torch.randn(ROWS + VROWS, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    y = ((xt @ w + 0.5 * torch.randn(ROWS + VROWS, D, device="cuda:0", dtype=torch.float32)) > 0.4).to(torch.float32)
    x, xv, yt, yv = xt[:ROWS].contiguous(), xt[ROWS:].contiguous(), y[:ROWS].contiguous(), y[ROWS:].contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    first = fresh()
    ds = first.prepare_dataset(tup(x))
    dsv = first.prepare_dataset(tup(xv), reference=ds)

    def fit(m, metric):
        kw = {} if metric is None else dict(eval_metric=metric)
        return m.fit_prepared(ds, tup(yt), T, valid=dsv, valid_targets=tup(yv), objective="logistic", **kw)
    return np, fresh, fit, timed, (x, xv, yt, yv)


def run_plain(root):
    np, fresh, fit, timed, _keep = setup_fit(root)
    fit(fresh(), None)
    ms = []
    for _ in range(REPS):
        m = fresh()
        ms.append(timed(lambda: fit(m, None)))
    print(json.dumps({"call": "fit_prepared(ds, y, %d, valid=dsv, valid_targets=yv, objective='logistic')" % T, "median_ms": round(float(np.median(ms)), 3),
                      "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": REPS}), flush=True)
    return 0


def run_fit():
    np, fresh, fit, timed, _keep = setup_fit(ROOT)
    med = lambda a: float(np.median(a))
    name = lambda e: "None" if e is None else "'%s'" % e
    print("fit_prepared  %d x %d, %d validation rows  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  logistic  [medians of %d, the legs "
          "alternating, after two runs of each]" % (ROWS, F, VROWS, DEPTH, D, BINS, T, REPS))
    files = {}
    for e in LEGS:
        a, b = fresh(), fresh()
        ra, rb = fit(a, e), fit(b, e)
        files[e] = file_bytes(a)
        same = files[e] == file_bytes(b) and all(np.asarray(ra[k]).tobytes() == np.asarray(rb[k]).tobytes() for k in ra if k != "eval_metric")
        tail = "" if e is None else "   valid_metric %.6f -> %.6f" % (ra["valid_metric"][0], ra["valid_metric"][-1])
        print("    eval_metric=%-7s two runs, %d trees: %s   valid_loss %.6f -> %.6f  best_n_trees %d%s" %
              (name(e), a.get_num_trees(), "byte-equal files and curves" if same else "DIFFERENT", ra["valid_loss"][0], ra["valid_loss"][-1], ra["best_n_trees"], tail))
        if not same:
            return 1
    if files["error"] != files[None] or files["auc"] != files[None]:
        print("    a metric changed the model file")
        return 1
    print("    the three legs leave the same model file")
    ms = {e: [] for e in LEGS}
    for _ in range(REPS):
        for e in LEGS:
            m = fresh()
            ms[e].append(timed(lambda: fit(m, e)))
    spread = max(max(v) - min(v) for v in ms.values())
    for e in LEGS:
        print("    fit_prepared(eval_metric=%-7s)  call %9.3f ms (min %9.3f max %9.3f)   %.3f ms per iteration" % (name(e), med(ms[e]), min(ms[e]), max(ms[e]), med(ms[e]) / T))
    for e in LEGS[1:]:
        diff = med(ms[e]) - med(ms[None])
        print("    %s / None: %.3f   %+.3f ms, %+.4f ms per evaluation (%d evaluations; spread between repeats %.3f ms: %s)" %
              (name(e), med(ms[e]) / med(ms[None]), diff, diff / (T + 1), T + 1, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"), flush=True)
    return 0


def run_eval():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import gbrl_amd
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    print("eval_metric   device buffers in, objective logistic, D = %d  [medians of %d, after two calls with equal bytes]" % (D, REPS))
    for n in (1 << 20, 262144):
        m = gbrl_amd.GBRL(input_dim=4, output_dim=D, policy_dim=D, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=n, grow_policy="oblivious", verbose=0,
                          device="cuda", learner_name="sweep")
        torch.manual_seed(8)
        p = (2 * torch.randn(n, D, device="cuda:0", dtype=torch.float32)).contiguous()
        y = ((p + 2 * torch.randn(n, D, device="cuda:0", dtype=torch.float32)) > 0.5).to(torch.float32).contiguous()
        for metric in ("error", "auc"):
            va, ca = m.eval_metric(tup(p), tup(y), "logistic", metric)
            vb, cb = m.eval_metric(tup(p), tup(y), "logistic", metric)
            if ca.tobytes() != cb.tobytes() or np.float64(va).tobytes() != np.float64(vb).tobytes():
                print("    n=%d %s: two calls DIFFER" % (n, metric))
                return 1
            ms = []
            for _ in range(REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.eval_metric(tup(p), tup(y), "logistic", metric)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            t = float(np.median(ms))
            if metric == "auc":
                moved = 16.0 * n * D * 4
                extra = "   sort traffic 16 n D x 4 passes = %.1f MB: %.3f TB/s of the whole call" % (moved / 1e6, moved / 1e12 / (t * 1e-3))
            else:
                moved = 8.0 * n * D
                extra = "   %.1f MB that must move: %.3f TB/s" % (moved / 1e6, moved / 1e12 / (t * 1e-3))
            print("    n=%-8d %-5s call %8.3f ms (min %8.3f max %8.3f)   value %.6f%s" % (n, metric, t, min(ms), max(ms), va, extra), flush=True)
    return 0


HEADER = """# python3 scripts/metric_sweep.py  -- one MI355X; each part in its own process; predictions and targets are device tensors
# eval_metric = the call on device buffers: zeroing the counters, the kernels, the read-back of the integers and the wait included
# fit legs = fit_prepared(ds, y, T, valid=dsv, valid_targets=yv, objective="logistic", eval_metric=e) on a fresh model, e = None, 'error', 'auc'
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread
"""


def main():
    argv = sys.argv[1:]
    if argv == ["--eval"]:
        return run_eval()
    if argv == ["--fit"]:
        return run_fit()
    if argv and argv[0] == "--plain" and len(argv) <= 2:
        return run_plain(os.path.abspath(argv[1]) if len(argv) == 2 else ROOT)
    parent = os.path.abspath(argv[argv.index("--parent") + 1]) if "--parent" in argv else None
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "metric.txt")
    me = os.path.abspath(__file__)
    jobs = [(["--eval"], 180, None), (["--fit"], 420, None)]
    if parent:
        jobs += [(["--plain", parent], 300, "previous commit  "), (["--plain"], 300, "this commit      ")] * 2
    text, rc, noted = HEADER, 0, False
    for args, limit, label in jobs:
        if label and not noted:
            text += "\n# the eval_metric=None leg against the previous commit's build: python3 scripts/metric_sweep.py --plain [ROOT], the two builds alternating process by process\n"
            noted = True
        child = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me] + args, stdout=subprocess.PIPE, text=True)
        lines = (label or "") + child.stdout if label else child.stdout
        print(lines, end="", flush=True)
        text += lines
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
