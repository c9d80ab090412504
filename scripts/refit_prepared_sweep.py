"""refit_leaves_prepared -- the leaf values of a tree range fitted again on a prepared data set, one enqueue and one wait -- against what a user can do
without it, on the same build:

    newton   the loop newton_leaves_prepared(ds, P, y, tree=t) -> predict_continue_prepared(ds, P, t, t + 1) over the range (a wait, a read-back of
             the sums, the value rule on the host and a re-upload of the mirror slice per tree).  The loop is the yardstick.
    rmse     refit_leaves(X, None, Y) on the float matrix behind the data set.

Rows, targets and the held prediction are device tensors (a "cuda" model), so the times are the calls, not PCIe copies.  Per shape a logistic and an
rmse model are fitted with fit_prepared; every repetition refits a fresh clone of it (made outside the clock), the two legs of a pair alternating in
one process.  Before anything is timed the two legs' model bytes are compared: they must be equal.  call = host clock around the call(s), each
ending in a stream synchronise; medians of `reps`, with min / max = the spread between repeats.

    python3 scripts/refit_prepared_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                           # failure; writes profiles/refit_prepared.txt (or FILE) when every shape has run
    python3 scripts/refit_prepared_sweep.py --shape NAME   # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, DEPTH, BINS = 8, 6, 256
# name: rows, columns, trees, repetitions, time limit of the child (s)
SHAPES = {"2^20x128_t100": (1 << 20, 128, 100, 10, 500), "65536x128_t1000": (65536, 128, 1000, 10, 500), "4096x16_t200": (4096, 16, 200, 10, 200)}


def run(name):
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, trees, reps, _ = SHAPES[name]

    def fresh():
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=BINS, split_score_func="L2", generator_type="Quantile",
                          grow_policy="oblivious", device="cuda", batch_size=rows)
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(5)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    s = torch.tanh(xt @ w) + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    yr, yl = s.contiguous(), (s > 0).to(torch.float32).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    values = lambda m: np.asarray(m.get_ensemble_data()["values"], np.float32).tobytes()

    def clock(fn, m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(m)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def pair(m0, new, old):
        """the bytes first, then `reps` alternating repetitions on fresh clones; returns the two lists of times (ms)"""
        a, b = gbrl_amd.GBRL(m0), gbrl_amd.GBRL(m0)
        new(a), old(b)
        assert values(a) == values(b), "%s: the two legs leave different model bytes" % name
        ta, tb = [], []
        for _ in range(reps):
            ta.append(clock(new, gbrl_amd.GBRL(m0)))
            tb.append(clock(old, gbrl_amd.GBRL(m0)))
        return ta, tb

    def line(what, t):
        t = sorted(t)
        return "%-34s %9.2f ms  (min %9.2f  max %9.2f)" % (what, t[len(t) // 2], t[0], t[-1])

    out = ["== %s: %d x %d, D = %d, depth %d, %d bins, %d trees, medians of %d ==" % (name, rows, F, D, DEPTH, BINS, trees, reps)]
    # ---- newton: one call against the public loop
    ml = fresh()
    ds = ml.prepare_dataset(tup(xt))
    ml.fit_prepared(ds, tup(yl), trees, objective="logistic")
    bias = torch.tensor(np.asarray(ml.get_bias(), np.float32), device="cuda:0").reshape(1, D).repeat(rows, 1).contiguous()

    def newton_loop(m):
        P = bias.clone()
        for t in range(trees):
            m.newton_leaves_prepared(ds, tup(P), tup(yl), "logistic", leaf_l2=1.0, tree=t)
            m.predict_continue_prepared(ds, tup(P), t, t + 1)   # (a device base is continued in place)

    ta, tb = pair(ml, lambda m: m.refit_leaves_prepared(ds, tup(yl), objective="logistic", leaf_update="newton", leaf_l2=1.0), newton_loop)
    out += [line("newton  refit_leaves_prepared", ta), line("newton  the loop, per range", tb),
            "newton  loop / call = %.2f   per tree: %.3f ms against %.3f ms" % (sorted(tb)[reps // 2] / sorted(ta)[reps // 2], sorted(ta)[reps // 2] / trees, sorted(tb)[reps // 2] / trees)]
    # ---- rmse gradient: the codes against the float matrix
    mr = fresh()
    dsr = mr.prepare_dataset(tup(xt))
    mr.fit_prepared(dsr, tup(yr), trees)
    ta, tb = pair(mr, lambda m: m.refit_leaves_prepared(dsr, tup(yr)), lambda m: m.refit_leaves(tup(xt), None, tup(yr)))
    out += [line("rmse    refit_leaves_prepared", ta), line("rmse    refit_leaves (float rows)", tb),
            "rmse    refit_leaves / refit_leaves_prepared = %.2f" % (sorted(tb)[reps // 2] / sorted(ta)[reps // 2])]
    print("\n".join(out), flush=True)


def main():
    if "--shape" in sys.argv:
        return run(sys.argv[sys.argv.index("--shape") + 1])
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "refit_prepared.txt")
    text = ["# scripts/refit_prepared_sweep.py: refit_leaves_prepared against the newton loop and against refit_leaves (see the script's docstring)"]
    for name, shape in SHAPES.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name], capture_output=True, text=True, timeout=shape[-1])
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit("shape %s failed (exit %d): stopping" % (name, r.returncode))
        text.append(r.stdout.rstrip())
    with open(dest, "w") as f:
        f.write("\n\n".join(text) + "\n")


if __name__ == "__main__":
    main()
