"""fit_prepared growing every tree on a one-side sample of its batch (goss = (0.1, 0.1), (0.2, 0.1)) against subsample at the same kept fraction
(0.2, 0.3) and against the full batch, the same build.

Targets are device tensors (a "cuda" model) and the data set is prepared once before the timing, so the times are the calls.
    legs     = a fresh model, fit_prepared(ds, targets, T, objective=o, seed=1, ...) for o = rmse (float32 [n, 8]) and softmax (int32 labels [n]):
               the full batch; subsample = 0.2, 0.3 (three sampler launches, the 4-byte read-back, the gather of the subset's code records); goss =
               (0.1, 0.1), (0.2, 0.1) (the score pass, three count passes, the tie pass, two scans, count and write: nine launches and a memset
               in place of the three, the same read-back and gather).  batch_size = n.
    Before the timing every leg is run twice and the two saved model files are compared byte for byte.
    call     = host clock around the call, between two device synchronisations.  The legs alternate in one process; medians of `REPS`, with
               min / max = the spread between repeats.
    phases   = the device time of one iteration's draw from the event pairs at profiling level 2 -- `goss_select` (scores, keys, the radix
               selection, the tie counts) and `sample_goss` (the tie scan, count, scan, write + gather, the 4-byte copy), or `sample_rows` -- the
               last iteration of a short profiled run, median of `PROFILED` runs; with them the other phases of that iteration.
    buys     = the noisy linear rule of profiles/newton.txt at 65 536 rows (logistic, D = 1, depth 3, 16 384 validation rows): the validation loss
               and error rate after 20 / 50 / 100 trees for the full batch, subsample = 0.3 and goss = (0.2, 0.1), with gradient and with Newton
               leaves.  Recorded, nothing asserted.

    python3 scripts/goss_sweep.py [--out FILE]        # every shape and `buys`, each in a child process of its own under a time limit; stops at the
                                                      # first failure; writes profiles/goss.txt (or FILE) when every part has run
    python3 scripts/goss_sweep.py --shape NAME        # one shape, in this process
    python3 scripts/goss_sweep.py --buys              # the quality table, in this process
    python3 scripts/goss_sweep.py --leg NAME plain|subsample [ROOT]   # only fit_prepared(ds, y, T) or fit_prepared(ds, y, T, subsample=0.5, seed=1),
                                                      # one JSON line: the legs that an earlier build (its tree at ROOT) runs too
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
    "65536x128_T1000": (65536, 128, 1000, 560),
    "4096x16_T200": (4096, 16, 200, 200),
}
# name, keywords, the subsample leg it is compared with
LEGS = (("full", {}, None), ("subsample=0.2", dict(subsample=0.2), None), ("goss=(0.1, 0.1)", dict(goss=(0.1, 0.1)), "subsample=0.2"),
        ("subsample=0.3", dict(subsample=0.3), None), ("goss=(0.2, 0.1)", dict(goss=(0.2, 0.1)), "subsample=0.3"))
REPS, PROFILED, SEED = 10, 5, 1


def setup(name, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, T, _ = SHAPES[name]

    def fresh():
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=rows, grow_policy="oblivious", verbose=0,
                          device="cuda", learner_name="sweep")
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(5)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    s = torch.tanh(xt @ w) + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    yt = s.contiguous()
    lt = torch.argmax(s, dim=1).to(torch.int32).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ds = fresh().prepare_dataset(tup(xt))
    return np, fresh, ds, {"rmse": tup(yt), "softmax": tup(lt)}, timed, (rows, F, T), (xt, yt, lt)


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def run_leg(name, which, root):
    np, fresh, ds, targets, timed, (rows, F, T), _keep = setup(name, root)
    kw = {} if which == "plain" else dict(subsample=0.5, seed=SEED)
    call = "fit_prepared(ds, y, T)" if which == "plain" else "fit_prepared(ds, y, T, subsample=0.5, seed=1)"
    fresh().fit_prepared(ds, targets["rmse"], T, **kw)
    ms = []
    for _ in range(REPS):
        m = fresh()
        ms.append(timed(lambda: m.fit_prepared(ds, targets["rmse"], T, **kw)))
    print(json.dumps({"shape": name, "call": call, "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                      "reps": REPS}), flush=True)
    return 0


def run(name):
    np, fresh, ds, targets, timed, (rows, F, T), _keep = setup(name, ROOT)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  seed=%d  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, SEED, REPS))
    for obj in ("rmse", "softmax"):
        y = targets[obj]
        kws = {leg: dict(kw, objective=obj, seed=SEED) for leg, kw, _ in LEGS}
        files = {}
        for leg, _, _ in LEGS:
            a, b = fresh(), fresh()
            la, lb = a.fit_prepared(ds, y, T, **kws[leg]), b.fit_prepared(ds, y, T, **kws[leg])
            files[leg] = file_bytes(a)
            same = files[leg] == file_bytes(b) and np.float32(la).tobytes() == np.float32(lb).tobytes()
            print("    %-8s %-16s two runs, %d trees: %s   loss on all rows %.7g" % (obj, leg, a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", la))
            if not same:
                return 1
        if len(set(files.values())) != len(files):
            print("    two legs left the same model: a sampled leg is not sampled")
            return 1
        ms = {leg: [] for leg, _, _ in LEGS}
        for _ in range(REPS):
            for leg, _, _ in LEGS:
                m = fresh()
                ms[leg].append(timed(lambda: m.fit_prepared(ds, y, T, **kws[leg])))
        spread = max(max(v) - min(v) for v in ms.values())
        for leg, _, _ in LEGS:
            print("    %-8s fit_prepared(%-16s)  call %s   %.3f ms per iteration   %.3f of the full batch" %
                  (obj, leg, fmt(ms[leg]), med(ms[leg]) / T, med(ms[leg]) / med(ms["full"])))
        for leg, _, against in LEGS:
            if against is None:
                continue
            diff = med(ms[leg]) - med(ms[against])
            print("    %-8s %s - %s: %+.3f ms, %+.4f ms per iteration: the price of the selection (spread between repeats %.3f ms: %s)" %
                  (obj, leg, against, diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"), flush=True)
        # the draw's own device time and the phases around it: the last iteration of a short profiled run
        for leg, _, _ in LEGS[1:]:
            seen = []
            for _ in range(PROFILED):
                m = fresh()
                m.set_profiling(2)
                m.fit_prepared(ds, y, 4, **kws[leg])
                seen.append(dict(m.last_phase_times()))
                m.set_profiling(0)
            names = ("continue_codes", "goss_select", "sample_goss", "sample_rows", "grad_stats", "gather_codes")
            print("    %-8s %-16s iteration 4, device ms from events, medians of %d:  %s" %
                  (obj, leg, PROFILED, "  ".join("%s %.4f" % (k, med([s[k] for s in seen])) for k in names if all(k in s for s in seen))), flush=True)
    return 0


def run_buys():
    import numpy as np
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n, nv, F, T = 65536, 16384, 16, 100
    rng = np.random.default_rng(20251)
    X = rng.standard_normal((n + nv, F)).astype(np.float32)
    w = rng.standard_normal(F).astype(np.float32)
    y = ((X @ w + rng.standard_normal(n + nv).astype(np.float32)) > 0).astype(np.float32)
    print("what it buys   %d rows (%d validation), F = %d, logistic D = 1, depth 3, lr 0.1, leaf_l2 = 1, labels from a noisy linear rule, seed = %d  [recorded, nothing asserted]" %
          (n, nv, F, SEED))
    print("    (a gradient leaf stores the MEAN of the amplified gradients over the kept rows, about 1 / (top + other) times the batch mean: goss = (0.2, 0.1) steps about")
    print("     3.3 times as far per tree as the other two legs; a newton leaf stores sum e g / (sum e h + leaf_l2), which the amplification leaves unbiased)")
    for rule in ("gradient", "newton"):
        for leg, kw in (("full", {}), ("subsample=0.3", dict(subsample=0.3)), ("goss=(0.2, 0.1)", dict(goss=(0.2, 0.1)))):
            m = gbrl_amd.GBRL(input_dim=F, output_dim=1, policy_dim=1, max_depth=3, min_data_in_leaf=0, n_bins=32, par_th=10, cv_beta=0.9, split_score_func="L2",
                              generator_type="Quantile", use_control_variates=False, batch_size=n, grow_policy="oblivious", verbose=0, device="cuda", learner_name="sweep")
            m.set_feature_weights(np.ones(F, np.float32))
            m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=1)
            m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
            ds = m.prepare_dataset(X[:n])
            dsv = m.prepare_dataset(X[n:], reference=ds)
            r = m.fit_prepared(ds, y[:n], T, valid=dsv, valid_targets=y[n:], objective="logistic", eval_metric="error", leaf_update=rule, leaf_l2=1.0, seed=SEED, **kw)
            print("    %-8s %-16s %s" % (rule, leg, "   ".join("after %3d trees: valid_loss %.6f error %.4f" % (k, r["valid_loss"][k], r["valid_metric"][k]) for k in (20, 50, 100))),
                  flush=True)
    return 0


HEADER = """# python3 scripts/goss_sweep.py  -- one MI355X; each shape in its own process; targets are device tensors, the data set is prepared once
# legs = fit_prepared(ds, targets, T, objective=o, seed=1, ...) on a fresh model: the full batch, subsample = 0.2 / 0.3, goss = (0.1, 0.1) / (0.2, 0.1) (the same kept fractions); batch_size = n
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
# goss_select = scores, keys, the radix selection and the tie counts; sample_goss = the tie scan, count, scan, write + gradient gather, the 4-byte copy; from the phases' event pairs
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--buys":
        return run_buys()
    if len(sys.argv) in (4, 5) and sys.argv[1] == "--leg" and sys.argv[3] in ("plain", "subsample"):
        return run_leg(sys.argv[2], sys.argv[3], os.path.abspath(sys.argv[4]) if len(sys.argv) == 5 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "goss.txt")
    text, rc = HEADER, 0
    jobs = [(["--shape", name], SHAPES[name][3]) for name in SHAPES] + [(["--buys"], 180)]
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
