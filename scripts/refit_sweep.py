"""refit_leaves -- the leaf values of a fitted ensemble fitted again, the structure kept -- against fit() of the same number of trees on the
same data (the same build: fit is unchanged), and its kernel time per tree against ONE predict_continue call over a single tree on the same
rows, which is the floor for "walk the rows once and touch the prediction once".

Rows, targets and the held prediction are device tensors (a "cuda" model), so the times are the calls, not PCIe copies.  Per shape: a fresh
model is fitted `reps` times (fit legs), the last one is refitted `reps` times over all its trees with decay_rate = 0 (on the fitted data: the
values keep their bits, which is checked and reported), and predict_continue runs over the tree [0, 1).
    call    = host clock around the call (each ends in a stream synchronise).  refit_leaves: one enqueue for the whole range, one wait, then the
              values are written to the host model; the device mirror is uploaded again by the NEXT call that needs it, so that cost is not in
              this column (the predict_continue leg that follows pays it once; its first repetition is a warm-up).
    kernel  = the library's HIP-event bracket (set_profiling(1)): last_phase_times()["refit"] covers the prefix prediction, every accumulate /
              finalize / apply launch and the loss kernels; ["predict"] is k_continue.
Medians, with min / max = the spread between repeats.

    python3 scripts/refit_sweep.py [--out FILE]    # every shape, each in a child process of its own under a time limit; stops at the first failure;
                                                   # writes profiles/refit.txt (or FILE) when every shape has run
    python3 scripts/refit_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

F, D = 128, 8
# name: rows, policy, depth, trees, repetitions, time limit of the child (s)
SHAPES = {
    "obl15_2^20": (1 << 20, "oblivious", 6, 15, 10, 300),
    "obl100_2^20": (1 << 20, "oblivious", 6, 100, 10, 400),
    "grd10_2^20": (1 << 20, "greedy", 6, 10, 10, 300),
    "obl1000_65536": (65536, "oblivious", 6, 1000, 10, 500),
    "obl15_d1_2^20": (1 << 20, "oblivious", 1, 15, 10, 300),
}


def run(name):
    import numpy as np
    import torch
    import cases as K
    import gbrl_amd
    rows, policy, depth, trees, reps, _ = SHAPES[name]
    case = dict(name="rf", seed=11, N=4096, F=F, Fc=0, D=D, depth=depth, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
                policy=policy, trees=trees, batch_size=rows)

    def fresh():
        m = gbrl_amd.GBRL(**K.ctor_kwargs(case, device="cuda"))
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(5)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    yt = (torch.tanh(xt @ w) + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    xa, ya = tup(xt), tup(yt)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))

    fit_ms = []
    m = None
    for i in range(1 + reps):
        m = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.fit(xa, None, ya, trees, shuffle=False)
        dt = time.perf_counter() - t0
        if i >= 1:
            fit_ms.append(dt * 1e3)
    T = m.get_num_trees()
    assert T == trees
    e = m.get_ensemble_data()
    n_leaves = int(np.asarray(e["values"]).shape[0])
    fitted = np.asarray(e["values"], np.float32).tobytes()

    m.set_profiling(1)
    refit_ms, refit_kern, losses = [], [], []
    for i in range(2 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = m.refit_leaves(xa, None, ya, 0, T, 0.0)
        dt = time.perf_counter() - t0
        if i >= 2:
            refit_ms.append(dt * 1e3)
            refit_kern.append(float(m.last_phase_times().get("refit", float("nan"))))
            losses.append(loss)
    same = np.asarray(m.get_ensemble_data()["values"], np.float32).tobytes() == fitted
    staged = float(np.asarray(m.staged_loss(xa, None, ya, stops=[T]))[0])

    bias = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).to("cuda:0")
    cache = bias.repeat(rows, 1).contiguous()
    ca = tup(cache)
    cont_ms, cont_kern = [], []
    for i in range(2 + reps):
        cache.copy_(bias.repeat(rows, 1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.predict_continue(xa, None, ca, 0, 1)
        dt = time.perf_counter() - t0
        del out
        if i >= 2:
            cont_ms.append(dt * 1e3)
            cont_kern.append(float(m.last_phase_times().get("predict", float("nan"))))

    print("%-14s %8d x %d  %-9s d%d  %4d trees  %6d leaves  D=%d  [%d reps]" % (name, rows, F, policy, depth, T, n_leaves, D, reps))
    print("    refit on the fitted data: values %s; returned loss %s staged_loss; %d distinct losses over the repetitions" %
          ("keep their bits" if same else "CHANGED", "==" if losses[-1] == staged else "!=", len(set(losses))))
    print("    fit(%d trees)          call %s   = %7.3f ms per tree" % (T, fmt(fit_ms), med(fit_ms) / T))
    print("    refit_leaves(0, %d)    call %s   kernel %s   = %7.3f ms per tree (kernel)" % (T, fmt(refit_ms), fmt(refit_kern), med(refit_kern) / T))
    print("    predict_continue(0, 1)  call %s   kernel %s" % (fmt(cont_ms), fmt(cont_kern)))
    print("    refit / fit: call %.3f     refit kernel per tree / predict_continue kernel over one tree: %.2f" %
          (med(refit_ms) / med(fit_ms), (med(refit_kern) / T) / med(cont_kern)), flush=True)


HEADER = """# python3 scripts/refit_sweep.py  -- one MI355X; each shape in its own process; rows, targets and the held prediction are device tensors
# fit = fit() of a fresh model, one batch that holds the whole data set, unshuffled; refit_leaves = all trees of that model on the same data, decay_rate 0
# predict_continue(0, 1) = one tree over the same rows: the floor for "walk the rows once and touch the prediction once"
# call = host clock around the call (ends in a stream synchronise); kernel = HIP events around the kernels (set_profiling(1)); medians over the repetitions, min / max = the spread
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "refit.txt")
    text, rc = HEADER, 0
    for name in SHAPES:
        child = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][5]), sys.executable, os.path.abspath(__file__), "--shape", name],
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
