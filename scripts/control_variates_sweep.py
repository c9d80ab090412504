"""control_variates / control_variates_prepared against the existing chain calls, in the same run of the same build: predict_continue over [0, T) on the
float matrix and predict_continue_prepared on the data set bound to it -- the same routing with an fma chain, so the ratio shows what the
three-rounding chain, the statistics passes and the second result cost.  A third pair times the continued call (momentum=, start_tree_idx = T - 1: one
new tree) against the full one: that ratio is the reason for momentum=.

The trees are grown by step_prepared on a 4096-row data set; the timed data set is bound to it (prepare_dataset(X, reference=)).  Observations,
gradients, momentum and results are device tensors (a "cuda" model).  Before timing: the float and the data set form return the same bytes, and the
continued call returns the same bytes in both forms (that a real continuation gives the bytes of the full call is
tests/test_gpu_control_variates.py's).  Per shape: 2 warm-up rounds, then `reps` timed rounds, the legs alternating within a round.
    call    = host clock around the call (it returns after the stream has been synchronised).
    kernel  = the library's HIP-event bracket around the call's launches (set_profiling(1); phase "control_variates": walk, fold, moments, apply; phase
              "predict": the chain kernel).
Medians, with min / max = the spread between repeats.

    python3 scripts/control_variates_sweep.py [--out FILE]    # every shape, each in a child process of its own under a time limit; stops at the first
                                                              # failure; writes profiles/control_variates.txt (or FILE) when every shape has run
    python3 scripts/control_variates_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

D, DEPTH = 8, 6
# name: rows, features, policy, trees, repetitions, time limit of the child (s)
SHAPES = {
    "obl15_2^20": (1 << 20, 128, "oblivious", 15, 10, 300),
    "grd10_2^20": (1 << 20, 128, "greedy", 10, 10, 300),
    "obl100_2^20": (1 << 20, 128, "oblivious", 100, 10, 300),
    "obl1000_65536": (65536, 128, "oblivious", 1000, 10, 400),
    "obl200_4096x16": (4096, 16, "oblivious", 200, 10, 300),
}


def run(name):
    import numpy as np
    import torch
    import cases as K
    import gbrl_amd
    rows, F, policy, trees, reps, _ = SHAPES[name]
    case = dict(name="cv", seed=11, N=4096, F=F, Fc=0, D=D, depth=DEPTH, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
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
    plan = gbrl_amd.gbrl_cpp.control_variates_geometry(rows, (F + 15) // 16, True, D)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    gt = torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    arg, garg = tup(xt), tup(gt)
    ds = m.prepare_dataset(arg, reference=train)
    bias = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).to("cuda:0")
    cache = bias.repeat(rows, 1).contiguous()
    carg = tup(cache)
    full = m.control_variates(arg, None, garg)
    full_g, full_m = torch.from_dlpack(full["grads"]), torch.from_dlpack(full["momentum"])
    prep = m.control_variates_prepared(ds, garg)
    assert torch.equal(torch.from_dlpack(prep["grads"]), full_g) and torch.equal(torch.from_dlpack(prep["momentum"]), full_m), "the data set form differs"
    # the continued call is timed on the full call's own momentum: one tree walked over held averages, the work of a real continuation (whose bytes
    # tests/test_gpu_control_variates.py checks against the full call)
    held = tup(full_m)
    cont = m.control_variates(arg, None, garg, momentum=held, start_tree_idx=T - 1)
    cont2 = m.control_variates_prepared(ds, garg, momentum=held, start_tree_idx=T - 1)
    assert torch.equal(torch.from_dlpack(cont["grads"]), torch.from_dlpack(cont2["grads"])), "the continued forms differ"
    del full, prep, cont, cont2
    legs = {"cv": lambda: m.control_variates(arg, None, garg),
            "continue": lambda: m.predict_continue(arg, None, carg, 0, T),
            "cv_prepared": lambda: m.control_variates_prepared(ds, garg),
            "continue_prepared": lambda: m.predict_continue_prepared(ds, carg, 0, T),
            "cv_one_tree": lambda: m.control_variates(arg, None, garg, momentum=held, start_tree_idx=T - 1),
            "cv_prepared_one_tree": lambda: m.control_variates_prepared(ds, garg, momentum=held, start_tree_idx=T - 1)}
    m.set_profiling(1)
    call = {k: [] for k in legs}
    kern = {k: [] for k in legs}
    for i in range(2 + reps):
        for k, fn in legs.items():
            if k.startswith("continue"):
                cache.copy_(bias.repeat(rows, 1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            del out
            if i >= 2:
                ph = m.last_phase_times()
                call[k].append(dt * 1e3)
                kern[k].append(float(ph.get("control_variates" if k.startswith("cv") else "predict", float("nan"))))
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))
    print("%-15s %8d x %-3d %-9s d%d  %4d trees  D=%d  [%d reps]  plan: %s" % (name, rows, F, policy, DEPTH, T, D, reps, plan))
    print("    outputs before timing: control_variates_prepared == control_variates (grads, momentum); the continued forms agree")
    label = {"cv": "control_variates", "continue": "predict_continue", "cv_prepared": "control_variates_prepared", "continue_prepared": "predict_continue_prepared",
             "cv_one_tree": "control_variates, 1 new tree", "cv_prepared_one_tree": "control_variates_prepared, 1 new"}
    for k in legs:
        print("    %-32s call %s   kernel %s" % (label[k], fmt(call[k]), fmt(kern[k])))
    ratio = lambda a, b: "call %.2f  kernel %.2f" % (med(call[a]) / med(call[b]), med(kern[a]) / med(kern[b]))
    print("    control_variates / predict_continue: %s     prepared / predict_continue_prepared: %s" % (ratio("cv", "continue"), ratio("cv_prepared", "continue_prepared")))
    print("    one new tree / full call:            %s     prepared: %s" % (ratio("cv_one_tree", "cv"), ratio("cv_prepared_one_tree", "cv_prepared")), flush=True)


HEADER = """# python3 scripts/control_variates_sweep.py  -- one MI355X; each shape in its own process; observations, gradients, momentum and results are device tensors
# control_variates(_prepared) = walk + fold + moments + apply over the trees [0, T); "1 new tree" = momentum= with start_tree_idx = T - 1
# predict_continue(_prepared) = the fma chain over [0, T) on the same rows of the same model: the yardstick
# call = host clock around the call (ends in a stream synchronise); kernel = HIP events around the launches (set_profiling(1)); medians over the repetitions, min / max = the spread
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "control_variates.txt")
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
