"""fit_prepared growing every tree on a sample of its batch (subsample = 0.5, 0.25) against the unsampled call (subsample = 1.0), the same build.

Targets are device tensors (a "cuda" model) and the data set is prepared once before the timing, so the times are the calls.
    legs     = a fresh model, fit_prepared(ds, y, T, subsample=p, seed=1) for p in 1.0, 0.5, 0.25; batch_size = n.  subsample = 1.0 runs the
               unsampled loop (no sampler launch, no gather); a sampled iteration adds the three sampler launches with the gradient gather, a
               4-byte read-back the host waits for, and the gather of the subset's code records that step_prepared(rows) does, and grows on m
               rows instead of n.
    Before the timing every leg is run twice and the two saved model files are compared byte for byte.
    call     = host clock around the call, between two device synchronisations.  The legs alternate in one process; medians of `REPS`, with
               min / max = the spread between repeats.
    sampler  = the device time of one iteration's sampler (count, scan, write + gather, the 4-byte copy) from the event pair of the
               `sample_rows` phase at profiling level 2: the last iteration of a short profiled run, median of `PROFILED` runs; with it the
               other phases of that iteration and the rows it grew on.

    python3 scripts/subsample_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                      # failure; writes profiles/subsample.txt (or FILE) when every shape has run
    python3 scripts/subsample_sweep.py --shape NAME   # one shape, in this process
    python3 scripts/subsample_sweep.py --plain NAME [ROOT]   # only fit_prepared(ds, y, T) without the keywords, one JSON line: the leg that an
                                                      # earlier build (its tree at ROOT) runs too -- profiles/fit_prepared.txt's parent / pr method
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
    kw = lambda p: dict(subsample=p, seed=SEED)
    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  seed=%d  [medians of %d, the legs alternating, after two runs of each]" %
          (name, rows, F, DEPTH, D, BINS, T, SEED, REPS))
    # two runs per leg: the same bytes; 1.0 is the call without the keywords
    files = {}
    for p in FRACTIONS:
        a, b = fresh(), fresh()
        la, lb = a.fit_prepared(ds, y, T, **kw(p)), b.fit_prepared(ds, y, T, **kw(p))
        files[p] = file_bytes(a)
        same = files[p] == file_bytes(b) and np.float32(la).tobytes() == np.float32(lb).tobytes()
        print("    subsample %.2f: two runs, %d trees: %s   loss on all rows %.7g" % (p, a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", la))
        if not same:
            return 1
    plain = fresh()
    plain.fit_prepared(ds, y, T)
    if file_bytes(plain) != files[1.0] or files[0.5] == files[1.0] or files[0.25] == files[0.5]:
        print("    subsample 1.00 is NOT the call without the keywords, or a sampled leg is not sampled")
        return 1
    print("    subsample 1.00 leaves the bytes of fit_prepared(ds, y, T); the sampled legs leave other models")
    ms = {p: [] for p in FRACTIONS}
    for _ in range(REPS):
        for p in FRACTIONS:
            m = fresh()
            ms[p].append(timed(lambda: m.fit_prepared(ds, y, T, **kw(p))))
    spread = max(max(v) - min(v) for v in ms.values())
    for p in FRACTIONS:
        print("    fit_prepared(subsample=%.2f)  call %s   %.3f ms per iteration" % (p, fmt(ms[p]), med(ms[p]) / T))
    for p in FRACTIONS[1:]:
        diff = med(ms[p]) - med(ms[1.0])
        print("    %.2f / 1.00: %.3f   %+.3f ms, %+.4f ms per iteration (spread between repeats %.3f ms: %s)" %
              (p, med(ms[p]) / med(ms[1.0]), diff, diff / T, spread, "beyond the spread" if abs(diff) > spread else "NOT beyond the spread"), flush=True)
    # the sampler's own device time and the phases around it: the last iteration of a short profiled run
    for p in FRACTIONS[1:]:
        seen = []
        for _ in range(PROFILED):
            m = fresh()
            m.set_profiling(2)
            m.fit_prepared(ds, y, 4, **kw(p))
            seen.append(dict(m.last_phase_times()))
            m.set_profiling(0)
        names = ("continue_codes", "sample_rows", "grad_stats", "gather_codes")
        kept = ds_sample_count(ds, p, 3)
        print("    subsample %.2f, iteration 4 (draw 3 keeps %d of %d rows), device ms from events, medians of %d:  %s" %
              (p, kept, rows, PROFILED, "  ".join("%s %.4f" % (k, med([s.get(k, float("nan")) for s in seen])) for k in names)), flush=True)
    return 0


def ds_sample_count(ds, p, draw):
    import torch
    return int(torch.from_dlpack(ds.sample_rows(p, seed=SEED, draw=draw)).numel())


HEADER = """# python3 scripts/subsample_sweep.py  -- one MI355X; each shape in its own process; targets are device tensors, the data set is prepared once
# legs = fit_prepared(ds, y, T, subsample=p, seed=1) on a fresh model, p = 1.0 (the unsampled loop: no sampler launch), 0.5, 0.25; batch_size = n
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
# sample_rows = one iteration's sampler on the device (count, scan, write + gradient gather, the 4-byte copy), from the phase's event pair
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--plain":
        return run_plain(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else ROOT)
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "subsample.txt")
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
