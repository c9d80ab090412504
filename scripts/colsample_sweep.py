"""fit_prepared growing every tree on a sample of the columns (colsample = 0.5, 0.25) against the call on all columns (colsample = 1.0), the same build.

Targets are device tensors (a "cuda" model) and the data set is prepared once before the timing, so the times are the calls.
    legs     = a fresh model, fit_prepared(ds, y, T, colsample=q, seed=1) for q in 1.0, 0.5, 0.25; batch_size = n.  colsample = 1.0 runs the loop
               without column sampling (no plan, no gather); a column-sampled iteration draws k columns on the host, uploads the gather plan,
               re-packs the code records of those columns into ceil(k / 16) groups (gather_cols.hip), gathers their thresholds, and grows on k
               features instead of F.
    Before the timing every leg is run twice and the two saved model files are compared byte for byte.
    call     = host clock around the call, between two device synchronisations.  The legs alternate in one process; medians of `REPS`, with
               min / max = the spread between repeats.
    gather   = the device time of one iteration's `gather_cols` phase (plan upload, the code gather, the threshold gather) from the phase's event
               pair at profiling level 2 -- an upper bound of the code gather kernel alone -- against the bytes that kernel must move: 32 bytes per
               row and touched source group read, 32 per row and output group written.  The last iteration of a short profiled run, median of
               `PROFILED` runs; with it the other phases of that iteration.

    python3 scripts/colsample_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                      # failure; writes profiles/colsample.txt (or FILE) when every shape has run
    python3 scripts/colsample_sweep.py --shape NAME   # one shape, in this process
    python3 scripts/colsample_sweep.py --plain NAME [ROOT]   # only fit_prepared(ds, y, T) without the keywords, one JSON line: the leg that an
                                                      # earlier build (its tree at ROOT) runs too
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
FRACTIONS = (1.0, 0.5, 0.25)
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
    yt = (torch.tanh(xt @ w) + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ds = fresh().prepare_dataset(tup(xt))
    return np, fresh, ds, tup(yt), timed, (rows, F, T), (xt, yt)


def file_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.gbrl_model")
        assert m.save(p) == 0
        with open(p, "rb") as f:
            return f.read()


def run_plain(name, root):
    np, fresh, ds, y, timed, (rows, F, T), _keep = setup(name, root)
    fresh().fit_prepared(ds, y, T)
    ms = []
    for _ in range(REPS):
        m = fresh()
        ms.append(timed(lambda: m.fit_prepared(ds, y, T)))
    print(json.dumps({"shape": name, "call": "fit_prepared(ds, y, T)", "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
                      "max_ms": round(max(ms), 3), "reps": REPS}), flush=True)
    return 0


def run(name):
    np, fresh, ds, y, timed, (rows, F, T), _keep = setup(name, ROOT)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    kw = lambda q: dict(colsample=q, seed=SEED)
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  seed=%d  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, SEED, REPS))
    # two runs per leg: the same bytes; 1.0 is the call without the keywords
    files = {}
    for q in FRACTIONS:
        a, b = fresh(), fresh()
        la, lb = a.fit_prepared(ds, y, T, **kw(q)), b.fit_prepared(ds, y, T, **kw(q))
        files[q] = file_bytes(a)
        same = files[q] == file_bytes(b) and np.float32(la).tobytes() == np.float32(lb).tobytes()
        print("    colsample %.2f (%3d of %d columns per tree): two runs, %d trees: %s   loss on all rows %.7g" %
              (q, ds.sample_cols(q, seed=SEED, draw=0).size, F, a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", la))
        if not same:
            return 1
    plain = fresh()
    plain.fit_prepared(ds, y, T)
    if file_bytes(plain) != files[1.0] or files[0.5] == files[1.0] or files[0.25] == files[0.5]:
        print("    colsample 1.00 is NOT the call without the keywords, or a sampled leg is not sampled")
        return 1
    print("    colsample 1.00 leaves the bytes of fit_prepared(ds, y, T); the sampled legs leave other models")
    ms = {q: [] for q in FRACTIONS}
    for _ in range(REPS):
        for q in FRACTIONS:
            m = fresh()
            ms[q].append(timed(lambda: m.fit_prepared(ds, y, T, **kw(q))))
    spread = max(max(v) - min(v) for v in ms.values())
    for q in FRACTIONS:
        print("    fit_prepared(colsample=%.2f)  call %s   %.3f ms per iteration" % (q, fmt(ms[q]), med(ms[q]) / T))
    for q in FRACTIONS[1:]:
        diff = med(ms[q]) - med(ms[1.0])
        print("    %.2f / 1.00: %.3f   %+.3f ms, %+.4f ms per iteration (spread between repeats %.3f ms: %s)" %
              (q, med(ms[q]) / med(ms[1.0]), diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"), flush=True)
    # the gather's own device time against its bytes, and the phases around it: the last iteration of a short profiled run
    for q in FRACTIONS:
        seen = []
        for _ in range(PROFILED):
            m = fresh()
            m.set_profiling(2)
            m.fit_prepared(ds, y, 4, **kw(q))
            seen.append(dict(m.last_phase_times()))
            m.set_profiling(0)
        names = sorted({k for s in seen for k in s}, key=lambda k: -med([s.get(k, 0.0) for s in seen]))[:6]
        text = "  ".join("%s %.4f" % (k, med([s.get(k, float("nan")) for s in seen])) for k in names)
        if q < 1.0:
            cols = ds.sample_cols(q, seed=SEED, draw=3)
            touched, out_groups = len({int(c) // 16 for c in cols}), (cols.size + 15) // 16
            moved = 32 * rows * (touched + out_groups)
            g = med([s.get("gather_cols", float("nan")) for s in seen])
            print("    colsample %.2f, iteration 4 (draw 3: %d columns in %d of %d source groups -> %d groups): gather_cols %.4f ms for %.1f MB that must move = %.0f GB/s" %
                  (q, cols.size, touched, (F + 15) // 16, out_groups, g, moved / 1e6, moved / 1e6 / g if g > 0 else float("nan")))
        print("    colsample %.2f, iteration 4, device ms from events, medians of %d, the six longest phases:  %s" % (q, PROFILED, text), flush=True)
    return 0


HEADER = """# python3 scripts/colsample_sweep.py  -- one MI355X; each shape in its own process; targets are device tensors, the data set is prepared once
# legs = fit_prepared(ds, y, T, colsample=q, seed=1) on a fresh model, q = 1.0 (no column sampling: no plan, no gather), 0.5, 0.25; batch_size = n
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
# gather_cols = one iteration's plan upload + code gather + threshold gather on the device, from the phase's event pair (an upper bound of the code gather kernel)
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--plain":
        return run_plain(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "colsample.txt")
    text, rc = HEADER, 0
    for name in SHAPES:
        child = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][3]), sys.executable, os.path.abspath(__file__), "--shape", name],
                               stdout=subprocess.PIPE, text=True)
        print(child.stdout, end="", flush=True)
        text += child.stdout
        rc = child.returncode
        if rc != 0:
            print("%s: exit status %d -- stopping" % (name, rc), flush=True)
            break
    if rc == 0:
        with open(out_path, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
