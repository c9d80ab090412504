"""Cost of one step() whose batch holds more distinct categorical cells than Fc * n_bins candidates (the mean-gradient ranking, cat_rank.hip).

    python scripts/cat_rank_sweep.py [--steps 12] [--parent DIR] [--out profiles/cat_rank.txt]

The shape is BASELINE configs[4]'s minibatch pushed into the overflow regime: 4096 rows, 192 numeric and 64 categorical columns, n_bins = 32,
tokens drawn from 100 000 values (about 4 000 distinct per column against 32 kept).  --parent DIR: a directory that holds ANOTHER build of the
gbrl_amd package (e.g. the parent commit's); the same inputs are timed there in a child process and both figures are written.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, FC, D, BINS, TOKENS = 4096, 192, 64, 8, 32, 100000


def measure(steps):
    import gbrl_amd
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, F), dtype=np.float32)
    toks = np.array([("v%06d" % i).encode() for i in range(TOKENS)], dtype="S128")
    Xc = np.ascontiguousarray(toks[rng.integers(0, TOKENS, size=(N, FC))])
    G = rng.standard_normal((N, D), dtype=np.float32)
    m = gbrl_amd.GBRL(input_dim=F + FC, output_dim=D, policy_dim=D, max_depth=6, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Uniform", use_control_variates=False, batch_size=N, grow_policy="oblivious",
                      verbose=0, device="cpu", learner_name="cat_rank_sweep")
    m.set_feature_weights(np.ones(F + FC, np.float32))
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_mapping(np.arange(F + FC, dtype=np.int32), np.array([True] * F + [False] * FC, dtype=bool))
    for _ in range(3):
        m.step(X, Xc, G.copy())
    ts = []
    for _ in range(steps):
        g = G.copy()
        t0 = time.perf_counter()
        m.step(X, Xc, g)
        ts.append((time.perf_counter() - t0) * 1e3)
    m.set_profiling(2)
    m.step(X, Xc, G.copy())
    ph = dict(m.last_phase_times())
    distinct = int(sum(len(np.unique(Xc[:, f])) for f in range(FC)))
    return dict(step_ms_median=float(np.median(ts)), step_ms_min=float(np.min(ts)), steps=steps, cat_rank_ms=ph.get("cat_rank"),
                distinct_cells=distinct, kept=FC * BINS, trees=int(m.get_num_trees()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cat_rank.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.steps)))
        return
    sys.path.insert(0, ROOT)
    new = measure(a.steps)
    old = None
    if a.parent:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps)], capture_output=True, text=True,
                             env=dict(os.environ, PYTHONPATH=os.path.abspath(a.parent)), timeout=900)
        lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if lines:
            old = json.loads(lines[-1][7:])
        else:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
    fmt = lambda v: "unmeasured" if v is None else "%.3f ms" % v
    txt = ["step() with more distinct categorical cells than Fc * n_bins: %d rows, %d numeric + %d categorical columns, n_bins %d, output_dim %d," % (N, F, FC, BINS, D),
           "tokens drawn from %d values: %d distinct (feature, cell) pairs against %d kept.  Host arrays in, wall clock of one step()," % (TOKENS, new["distinct_cells"], new["kept"]),
           "median (min) of %d steps after 3 warm-up steps, one MI355X." % new["steps"], "",
           "this build, ranking on the device : %s (%s)" % (fmt(new["step_ms_median"]), fmt(new["step_ms_min"])),
           "parent commit, ranking on the host: %s (%s)" % ((fmt(old["step_ms_median"]), fmt(old["step_ms_min"])) if old else ("unmeasured", "unmeasured")),
           "cat_rank phase (device events, one profiled step: norms, keys, sort, chains, publish launch): %s" % fmt(new["cat_rank_ms"]), ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(txt))
    print("\n".join(txt))


if __name__ == "__main__":
    main()
