"""predict() of a model with a Linear learning-rate schedule against a Const twin with the same trees, in the same process.

The Const twin runs the kernels a Const-only model has always run (kern::predict does not look at the rate table for it), so its time is
the baseline; the Linear model runs predict_sched.hip.  Rows are device tensors, the result stays on the device (DLPack): the time is
the call, not a PCIe copy.  Per shape: warm-up calls, then `reps` timed calls of each model, interleaved; median, min and max are printed,
and the ratio of the medians.

    python3 scripts/sched_predict_sweep.py                 # every shape, each in a child process of its own under a time limit;
                                                           # stops at the first shape that fails
    python3 scripts/sched_predict_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

# name: rows, features, policy, depth, trees, outputs, repetitions, time limit of the child (s), the kernels kern::predict dispatches to
# (Linear model / Const twin; `scripts/sched_predict_sweep.py --shape NAME` under `rocprofv3 --kernel-trace --stats` shows them)
SHAPES = {
    "obl15": (1 << 20, 128, "oblivious", 6, 15, 8, 30, 240, "k_sched_stream / k_predict_reg"),
    "grd10": (1 << 20, 128, "greedy", 6, 10, 8, 30, 240, "k_sched_stream / k_predict_grd_stream"),
    "obl1000": (1 << 20, 128, "oblivious", 6, 1000, 8, 8, 420, "k_sched_stream / k_predict_reg"),
    # 4096 rows x 2000 trees is inside the 128 .. 2048-tree window in which kern::predict spreads the trees of a small batch over block
    # columns: tree slices + combine on both sides, NOT the chain pair
    "slices2000": (4096, 16, "greedy", 4, 2000, 8, 50, 420, "k_sched_stream (32 tree slices) + k_predict_combine / k_predict_obl2 (slices) + combine"),
    # the chain pair: up to 1024 rows from 128 trees on, up to 8192 rows beyond 2048 trees
    "relay1024": (1024, 16, "greedy", 4, 2000, 8, 50, 420, "k_leaf_slots + k_sched_relay / k_leaf_slots + k_chain_relay"),
    "relay4096": (4096, 16, "greedy", 4, 2500, 8, 50, 420, "k_leaf_slots + k_sched_relay / k_leaf_slots + k_chain_relay"),
}


def run(name):
    import numpy as np
    import torch
    import cases as K
    import gbrl_amd
    rows, F, policy, depth, trees, D, reps, _, path = SHAPES[name]
    case = dict(name="sw", seed=11, N=4096, F=F, Fc=0, D=D, depth=depth, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
                policy=policy, trees=trees)
    X, _, G, _ = K.make_inputs(case)
    rng = np.random.default_rng(3)
    Gs = [np.ascontiguousarray(G + 0.5 * rng.standard_normal(G.shape).astype(np.float32)) for _ in range(16)]      # different trees
    lin = [dict(algo="SGD", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=D - 1, stop_lr=0.01, T=max(2, trees // 2)),
           dict(algo="SGD", scheduler="Const", init_lr=0.01, start_idx=D - 1, stop_idx=D)]
    con = [dict(lin[0], scheduler="Const"), lin[1]]
    models = []
    for opts in (lin, con):
        m = gbrl_amd.GBRL(**K.ctor_kwargs(case, device="cuda"))
        m.set_feature_weights(np.ones(F, np.float32))
        for o in opts:
            m.set_optimizer(**o)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        for t in range(trees):
            m.step(X, None, Gs[t % len(Gs)])      # step never reads the optimizer: both models grow the same trees
        assert m.get_num_trees() == trees
        models.append(m)
    el, ec = models[0].get_ensemble_data(), models[1].get_ensemble_data()
    assert all(np.array_equal(np.asarray(el[k]), np.asarray(ec[k])) for k in K.ENSEMBLE_KEYS), "the twins differ"
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    arg = (xt.data_ptr(), tuple(xt.shape), str(xt.dtype), "cuda")
    times = ([], [])
    for i in range(3 + reps):
        for k, m in enumerate(models):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.predict(arg, None, 0, 0)      # returns after the stream has been synchronised
            dt = time.perf_counter() - t0
            del out
            if i >= 3:
                times[k].append(dt * 1e6)
    med = [float(np.median(t)) for t in times]
    print("%-10s %8d x %-3d  %-9s d%d  %4d trees  D=%d   Linear %9.1f us (min %9.1f max %9.1f)   Const %9.1f us (min %9.1f max %9.1f)   ratio %.3f   [%d reps]   %s"
          % (name, rows, F, policy, depth, trees, D, med[0], min(times[0]), max(times[0]), med[1], min(times[1]), max(times[1]), med[0] / med[1], reps, path), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    for name in SHAPES:
        rc = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][7]), sys.executable, os.path.abspath(__file__), "--shape", name]).returncode
        if rc != 0:
            print("%s: exit status %d -- stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
