"""predict_leaves_prepared / leaf_counts_prepared -- where the rows of a data set land -- against the existing kernels, in the same run of the same
build: predict_leaves / leaf_counts on the float matrix behind the data set, and predict_continue_prepared over the same range of the same data set.

The trees are grown by step_prepared on a 4096-row data set; the timed data set is bound to it (prepare_dataset(X, reference=)), so its codes mean the
same thresholds.  The float matrix, the held prediction and the leaf matrices are device tensors (a "cuda" model); the count vectors return to the host,
which is part of those calls.  Before timing the outputs are compared: the two leaf matrices, the two count vectors, and bincount of the matrix.
Per shape: 2 warm-up rounds, then `reps` timed rounds, the legs alternating within a round.
    call    = host clock around the call (it returns after the stream has been synchronised).
    kernel  = the library's HIP-event bracket around the traversal kernels (set_profiling(1), last_phase_times()["predict"]); for the count calls the
              counter memset and one launch per run of trees whose leaves fit the chunk.
Medians, with min / max = the spread between repeats.

    python3 scripts/leaves_prepared_sweep.py [--out FILE]    # every shape, each in a child process of its own under a time limit; stops at the first
                                                             # failure; writes profiles/leaves_prepared.txt (or FILE) when every shape has run
    python3 scripts/leaves_prepared_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

F, D, DEPTH = 128, 8, 6
# name: rows, policy, trees, repetitions, time limit of the child (s)  (profiles/leaves.txt's four)
SHAPES = {
    "obl15_2^20": (1 << 20, "oblivious", 15, 10, 300),
    "grd10_2^20": (1 << 20, "greedy", 10, 10, 300),
    "obl100_2^20": (1 << 20, "oblivious", 100, 10, 300),
    "obl1000_65536": (65536, "oblivious", 1000, 10, 400),
}


def run(name):
    import numpy as np
    import torch
    import cases as K
    import gbrl_amd
    rows, policy, trees, reps, _ = SHAPES[name]
    case = dict(name="lv", seed=11, N=4096, F=F, Fc=0, D=D, depth=DEPTH, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
                policy=policy, trees=trees)
    X, _, G, _ = K.make_inputs(case)
    rng = np.random.default_rng(3)
    Gs = [np.ascontiguousarray(G + 0.5 * rng.standard_normal(G.shape).astype(np.float32)) for _ in range(16)]      # different trees
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case, device="cuda"))
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    train = m.prepare_dataset(X)
    for t in range(trees):
        m.step_prepared(train, Gs[t % len(Gs)])
    T = m.get_num_trees()
    assert T == trees
    n_leaves = int(np.asarray(m.get_ensemble_data()["values"]).shape[0])
    group, chunk, lds = gbrl_amd.GBRL.leaves_prepared_geometry((F + 15) // 16)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    arg = tup(xt)
    ds = m.prepare_dataset(arg, reference=train)
    bias = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).to("cuda:0")
    cache = bias.repeat(rows, 1).contiguous()
    carg = tup(cache)
    legs = {"leaves_prepared": lambda: m.predict_leaves_prepared(ds, 0, T),
            "leaves": lambda: m.predict_leaves(arg, None, 0, T),
            "counts_prepared": lambda: m.leaf_counts_prepared(ds, 0, T),
            "counts": lambda: m.leaf_counts(arg, None, 0, T),
            "continue_prepared": lambda: m.predict_continue_prepared(ds, carg, 0, T)}
    # the new calls agree with the old ones and with each other: checked before anything is timed
    lp, lf = torch.from_dlpack(legs["leaves_prepared"]()), torch.from_dlpack(legs["leaves"]())
    assert torch.equal(lp, lf), "predict_leaves_prepared differs from predict_leaves"
    binc = torch.bincount(lp.reshape(-1).long(), minlength=n_leaves).cpu().numpy().astype(np.int64)
    del lp, lf
    c1, c2, c3 = legs["counts_prepared"](), legs["counts_prepared"](), legs["counts"]()
    assert np.array_equal(c1, c3) and np.array_equal(c1, binc) and c1.tobytes() == c2.tobytes(), "leaf_counts_prepared differs"
    m.set_profiling(1)
    call = {k: [] for k in legs}
    kern = {k: [] for k in legs}
    for i in range(2 + reps):
        for k, fn in legs.items():
            if k == "continue_prepared":
                cache.copy_(bias.repeat(rows, 1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            del out
            if i >= 2:
                call[k].append(dt * 1e3)
                kern[k].append(float(m.last_phase_times().get("predict", float("nan"))))
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    print("%-14s %8d x %d  %-9s d%d  %4d trees  %6d leaves  D=%d  [%d reps]  plan: %d trees per group, chunk %d counters, %d bytes of LDS" %
          (name, rows, F, policy, DEPTH, T, n_leaves, D, reps, group, chunk, lds))
    print("    outputs before timing: predict_leaves_prepared == predict_leaves; leaf_counts_prepared == leaf_counts == bincount; two calls: same bytes")
    label = {"leaves_prepared": "predict_leaves_prepared", "leaves": "predict_leaves", "counts_prepared": "leaf_counts_prepared", "counts": "leaf_counts",
             "continue_prepared": "predict_continue_prepared"}
    for k in legs:
        print("    %-26s call %s   kernel %s" % (label[k], fmt(call[k]), fmt(kern[k])))
    ratio = lambda a, b: "call %.2f  kernel %.2f" % (med(call[a]) / med(call[b]), med(kern[a]) / med(kern[b]))
    print("    predict_leaves_prepared / predict_leaves: %s     / predict_continue_prepared: %s" % (ratio("leaves_prepared", "leaves"), ratio("leaves_prepared", "continue_prepared")))
    print("    leaf_counts_prepared / leaf_counts:       %s     / predict_continue_prepared: %s" % (ratio("counts_prepared", "counts"), ratio("counts_prepared", "continue_prepared")),
          flush=True)


HEADER = """# python3 scripts/leaves_prepared_sweep.py  -- one MI355X; each shape in its own process; the float matrix, the held prediction and the leaf matrices are device tensors
# predict_leaves_prepared / leaf_counts_prepared = the new calls on a bound data set (k_leaves_codes; memset + one k_leaf_counts_codes launch per run of trees);
# predict_leaves / leaf_counts = the float kernels on the matrix the data set was made from; predict_continue_prepared = the chain over the same range of the same data set
# call = host clock around the call (ends in a stream synchronise); kernel = HIP events around the traversal kernels (set_profiling(1)); medians over the repetitions, min / max = the spread
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "leaves_prepared.txt")
    text, rc = HEADER, 0
    for name in SHAPES:
        child = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][4]), sys.executable, os.path.abspath(__file__), "--shape", name],
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
