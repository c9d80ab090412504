"""fit_prepared(objective="quantile") with gradient and with quantile leaves against rmse of the same build; quantile_leaves_prepared alone against
newton_leaves_prepared on the same rows; what quantile leaves buy on a heteroscedastic rule.

    shapes   = 2^20 x 128 (T = 100), 65 536 x 128 (T = 1000), 4096 x 16 (T = 200); D = 8, depth 6, n_bins 256, oblivious / L2 / Quantile, lr 0.1
    legs     = a fresh model, fit_prepared(ds, y, T) (rmse), fit_prepared(ds, y, T, objective="quantile", alpha=levels[, leaf_update="quantile"]);
               batch_size = n.  Two runs of every leg must leave byte-equal files before anything is timed.
    timing   = host clock around the call between two device synchronisations, medians of 10, the legs alternating in one process; the
               quantile_leaves phase (event pair around the memset, the launches and the read-back) from one more, profiled, run
    kernel   = quantile_leaves_prepared on device buffers at the three sizes, D = 8, one depth-6 tree: the select path and the general (sort) path
               (GBRL_HIP_CONTINUE_GENERIC=1), the quantile_leaves phase as the time; newton_leaves_prepared (logistic) on the same rows as the yardstick
    trees    = y = f(x) + sigma(x) * noise at 65 536 rows (F = 16, levels 0.1 / 0.5 / 0.9, depth 3, lr 0.1, 16 384 validation rows): the validation
               pinball loss of both leaf rules after k trees, the gradient trees it takes to reach quantile leaves' loss, the validation coverage

    python3 scripts/quantile_sweep.py [--out FILE]    # everything, each part in a child process of its own under a time limit; stops at the first
                                                      # failure; writes profiles/quantile.txt (or FILE) when every part has run
    python3 scripts/quantile_sweep.py --shape NAME    # one shape, in this process
    python3 scripts/quantile_sweep.py --kernel NAME   # quantile_leaves_prepared alone at one shape
    python3 scripts/quantile_sweep.py --trees         # what it buys
    python3 scripts/quantile_sweep.py --plain NAME [ROOT]   # only the calls without the new keywords (rmse, logistic), one JSON line each: the legs that an
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
    "2^20x128_T100": (1 << 20, 128, 100, 420),
    "65536x128_T1000": (65536, 128, 1000, 540),
    "4096x16_T200": (4096, 16, 200, 180),
}
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
    y = (xt @ w + (0.5 + xt[:, :1].abs()) * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)).contiguous()
    onehot = (y > 0).to(torch.float32).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ds = fresh().prepare_dataset(tup(xt))
    return np, torch, fresh, ds, tup, timed, (rows, F, T), (xt, y, onehot)


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def run_plain(name, root):
    np, torch, fresh, ds, tup, timed, (rows, F, T), (xt, y, onehot) = setup(name, root)
    for call, t, kw in (("fit_prepared(ds, y, T)", y, {}), ("fit_prepared(ds, y, T, objective='logistic')", onehot, dict(objective="logistic"))):
        fresh().fit_prepared(ds, tup(t), T, **kw)
        ms = []
        for _ in range(REPS):
            m = fresh()
            ms.append(timed(lambda: m.fit_prepared(ds, tup(t), T, **kw)))
        print(json.dumps({"shape": name, "call": call, "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                          "reps": REPS}), flush=True)
    return 0


def levels(np):
    return np.linspace(0.1, 0.9, D).astype(np.float32)


def run(name):
    np, torch, fresh, ds, tup, timed, (rows, F, T), (xt, y, onehot) = setup(name, ROOT)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    a = levels(np)
    legs = {"rmse": {}, "quantile/gradient": dict(objective="quantile", alpha=a), "quantile/quantile": dict(objective="quantile", alpha=a, leaf_update="quantile")}
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  levels %s  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, " ".join("%.2f" % v for v in a), REPS))
    files = {}
    for leg, kw in legs.items():
        p, q = fresh(), fresh()
        lp, lq = p.fit_prepared(ds, tup(y), T, **kw), q.fit_prepared(ds, tup(y), T, **kw)
        files[leg] = file_bytes(p)
        same = files[leg] == file_bytes(q) and np.float32(lp).tobytes() == np.float32(lq).tobytes()
        print("    %-18s two runs, %d trees: %s   loss on all rows %.7g" % (leg, p.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", lp))
        if not same:
            return 1
    ms = {leg: [] for leg in legs}
    for _ in range(REPS):
        for leg, kw in legs.items():
            m = fresh()
            ms[leg].append(timed(lambda: m.fit_prepared(ds, tup(y), T, **kw)))
    spread = max(max(v) - min(v) for v in ms.values())
    for leg in legs:
        print("    %-18s call %s   %.4f ms per iteration" % (leg, fmt(ms[leg]), med(ms[leg]) / T))
    m = fresh()
    m.set_profiling(2)
    m.fit_prepared(ds, tup(y), T, **legs["quantile/quantile"])
    ph = dict(m.last_phase_times())
    for leg in ("quantile/gradient", "quantile/quantile"):
        diff = med(ms[leg]) - med(ms["rmse"])
        print("    %s / rmse: %.3f   %+.3f ms, %+.4f ms per iteration (spread between repeats %.3f ms: %s)" %
              (leg, med(ms[leg]) / med(ms["rmse"]), diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"))
    print("    quantile_leaves phase of the last iteration %.4f ms, select path: %s" % (ph.get("quantile_leaves", float("nan")), "yes" if ph.get("quantile_select") == 1.0 else "no"))
    for leg in ("rmse", "quantile/gradient"):   # where an iteration's time goes: the phases of the last one
        m = fresh()
        m.set_profiling(2)
        m.fit_prepared(ds, tup(y), T, **legs[leg])
        print("    phases of the last iteration, %-18s %s" % (leg, "  ".join("%s %.4f" % (k, v) for k, v in dict(m.last_phase_times()).items())), flush=True)
    return 0


def run_kernel(name):
    np, torch, fresh, ds, tup, timed, (rows, F, T), (xt, y, onehot) = setup(name, ROOT)
    a = levels(np)
    print("quantile_leaves_prepared   %d x %d, D = %d, one depth-%d tree, device buffers  [medians of %d, after two calls with equal bytes]" % (rows, F, D, DEPTH, REPS))
    m = fresh()
    m.fit_prepared(ds, tup(y), 1, objective="quantile", alpha=a)
    pred = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).cuda().repeat(rows, 1).contiguous()
    walk = rows * (((F + 15) // 16) * 32 + 8 * D)            # the code records, the prediction and the targets in
    select = walk + rows * D * 4 + rows * 4 + 4 * (rows * D * 4 + rows * 4 * D)   # keys and leaf ids out; four count passes over the keys and (per column) the leaf ids
    for generic in ("0", "1"):
        os.environ["GBRL_HIP_CONTINUE_GENERIC"] = generic
        ra = m.quantile_leaves_prepared(ds, tup(pred), tup(y), a)
        rb = m.quantile_leaves_prepared(ds, tup(pred), tup(y), a)
        if any(ra[k].tobytes() != rb[k].tobytes() for k in ra):
            print("    generic=%s: two calls DIFFER" % generic)
            return 1
        if generic == "0":
            first = ra
        elif any(ra[k].tobytes() != first[k].tobytes() for k in ra):
            print("    the two paths DIFFER")
            return 1
        m.set_profiling(2)
        dev, call = [], []
        for _ in range(REPS):
            call.append(timed(lambda: m.quantile_leaves_prepared(ds, tup(pred), tup(y), a)))
            ph = dict(m.last_phase_times())
            dev.append(ph["quantile_leaves"])
        m.set_profiling(0)
        sel = ph["quantile_select"] == 1.0
        print("    %-8s quantile_leaves phase %8.4f ms (min %8.4f max %8.4f)   call %8.3f ms%s   rows placed %d, leaves %d" %
              ("select" if sel else "general", float(np.median(dev)), min(dev), max(dev), float(np.median(call)),
               "   %.1f MB supposed to move = %.2f TB/s" % (select / 1e6, select / 1e9 / float(np.median(dev))) if sel else "", int(ra["counts"].sum()), len(ra["counts"])),
              flush=True)
    os.environ.pop("GBRL_HIP_CONTINUE_GENERIC", None)
    print("    the two paths returned the same bytes")
    # the yardstick: the Newton sums of a logistic model on the same rows
    n = fresh()
    n.fit_prepared(ds, tup(onehot), 1, objective="logistic")
    npred = torch.from_numpy(np.asarray(n.get_bias(), np.float32)).cuda().repeat(rows, 1).contiguous()
    n.newton_leaves_prepared(ds, tup(npred), tup(onehot), "logistic")
    n.set_profiling(2)
    dev = []
    for _ in range(REPS):
        n.newton_leaves_prepared(ds, tup(npred), tup(onehot), "logistic")
        dev.append(dict(n.last_phase_times())["newton_leaves"])
    n.set_profiling(0)
    print("    yardstick: newton_leaves phase (logistic, streaming kernel) %8.4f ms (min %8.4f max %8.4f)" % (float(np.median(dev)), min(dev), max(dev)), flush=True)
    return 0


def run_trees():
    import numpy as np
    sys.path.insert(0, ROOT)
    import gbrl_amd
    n, nv, F, Tg, Tq = 65536, 16384, 16, 600, 100
    rng = np.random.default_rng(20252)
    X = rng.standard_normal((n + nv, F)).astype(np.float32)
    w = rng.standard_normal(F).astype(np.float32)
    y1 = (np.sin(X[:, 0]) + 0.5 * (X @ w) / np.sqrt(F) + (0.25 + np.abs(X[:, 1])) * rng.standard_normal(n + nv)).astype(np.float32)
    a = np.array([0.1, 0.5, 0.9], np.float32)
    Y = np.ascontiguousarray(np.tile(y1[:, None], (1, 3)))
    print("what it buys   %d rows (%d validation), F = %d, y = f(x) + sigma(x) * noise, levels 0.1 / 0.5 / 0.9 (D = 3), depth 3, lr 0.1" % (n, nv, F))
    curves, cover = {}, {}
    for rule, T in (("gradient", Tg), ("quantile", Tq)):
        m = make_model(gbrl_amd, np, F, 3, n, depth=3, bins=32)
        ds = m.prepare_dataset(X[:n])
        dsv = m.prepare_dataset(X[n:], reference=ds)
        curves[rule] = np.asarray(m.fit_prepared(ds, Y[:n], T, valid=dsv, valid_targets=Y[n:], objective="quantile", alpha=a, leaf_update=rule)["valid_loss"])
        P = m.predict(X[n:], None, 0, 100)
        if not isinstance(P, np.ndarray):   # (a model that delivers on the device hands out a DLPack capsule)
            import torch
            P = torch.from_dlpack(P).cpu().numpy()
        P = P.reshape(nv, 3)
        cover[rule] = (Y[n:] <= P).mean(axis=0)
    for k in (10, 20, 50, 100):
        reach = np.nonzero(curves["gradient"] <= curves["quantile"][k])[0]
        print("    quantile leaves after %3d trees: valid pinball loss %.6f   gradient leaves reach it after %s trees (gradient after %3d trees: %.6f)" %
              (k, curves["quantile"][k], str(int(reach[0])) if reach.size else "more than %d" % Tg, k, curves["gradient"][k]), flush=True)
    for rule in ("gradient", "quantile"):
        print("    validation coverage mean(y <= p_d) after 100 trees, %-8s leaves: %s   (levels 0.100 0.500 0.900)" % (rule, " ".join("%.3f" % c for c in cover[rule])))
    return 0


HEADER = """# python3 scripts/quantile_sweep.py  -- one MI355X; each part in its own process; targets are device tensors, the data set is prepared once
# legs = fit_prepared(ds, y, T[, objective="quantile", alpha=levels[, leaf_update="quantile"]]) on a fresh model, y float32 [n, 8]
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
# quantile_leaves phase = an event pair around the memset of the result block, the launches and the enqueue of the read-back, in a profiled run of its own
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) == 3 and sys.argv[1] == "--kernel":
        return run_kernel(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--trees":
        return run_trees()
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--plain":
        return run_plain(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "quantile.txt")
    text, rc = HEADER, 0
    jobs = [(["--kernel", name], 180) for name in SHAPES] + [(["--shape", name], SHAPES[name][3]) for name in SHAPES] + [(["--trees"], 240)]
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
