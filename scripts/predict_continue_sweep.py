"""predict_continue(cache, T-1, T) -- one new tree applied to a held prediction -- against predict(X, T-1, T) over the same single tree and
against predict(X, 0, T), the whole walk a caller without a cache pays, in the same process.

Rows and cache are device tensors; predict's result stays on the device (DLPack) and predict_continue updates the cache in place, so the
times are the calls, not PCIe copies.  Per shape: warm-up calls, then `reps` timed calls of each of the three, interleaved.  Two clocks:
`call` = host clock around the call (it returns after the stream has been synchronised), `kernel` = the library's HIP-event bracket around the
traversal kernel (set_profiling(1), last_phase_times()["predict"]).  Medians, with min / max = the spread.  (a) = continue / predict of the one
tree: the new call moves 4 n D more bytes (it reads the cache), so a streaming kernel sits near (4F + 8D) / (4F + 4D); (b) = predict of the
whole ensemble / continue: the saving; (c) = n (4F + 8D) bytes over the kernel time.

    python3 scripts/predict_continue_sweep.py                 # every shape, each in a child process of its own under a time limit;
                                                              # stops at the first shape that fails
    python3 scripts/predict_continue_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

F, D, DEPTH = 128, 8, 6
# name: rows, policy, trees, repetitions, time limit of the child (s)
SHAPES = {}
for _pol, _trees in (("oblivious", 100), ("oblivious", 1000), ("greedy", 100)):
    for _rows in (4096, 65536, 1 << 20):
        SHAPES["%s%d_%d" % (_pol[:3], _trees, _rows)] = (_rows, _pol, _trees, 30, 300)


def run(name):
    import numpy as np
    import torch
    import cases as K
    import gbrl_amd
    rows, policy, trees, reps, _ = SHAPES[name]
    case = dict(name="pc", seed=11, N=4096, F=F, Fc=0, D=D, depth=DEPTH, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
                policy=policy, trees=trees)
    X, _, G, _ = K.make_inputs(case)
    rng = np.random.default_rng(3)
    Gs = [np.ascontiguousarray(G + 0.5 * rng.standard_normal(G.shape).astype(np.float32)) for _ in range(16)]      # different trees
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case, device="cuda"))
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    for t in range(trees):
        m.step(X, None, Gs[t % len(Gs)])
    T = m.get_num_trees()
    assert T == trees
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    arg = (xt.data_ptr(), tuple(xt.shape), str(xt.dtype), "cuda")
    held = torch.from_dlpack(m.predict(arg, None, 0, T - 1)).clone()     # the prediction over [0, T-1): what the caller's cache holds
    cache = held.clone()
    carg = (cache.data_ptr(), tuple(cache.shape), str(cache.dtype), "cuda")
    # the feature computes what the whole walk computes (same kernels' chain at these sizes or within predict's 1e-5: reported, not assumed)
    m.predict_continue(arg, None, carg, T - 1, T)
    whole = torch.from_dlpack(m.predict(arg, None, 0, T))
    max_diff = float((cache - whole).abs().max())
    same_bits = bool(torch.equal(cache, whole))
    m.set_profiling(1)
    legs = {"continue": lambda: m.predict_continue(arg, None, carg, T - 1, T),
            "predict1": lambda: m.predict(arg, None, T - 1, T),
            "predictT": lambda: m.predict(arg, None, 0, T)}
    call = {k: [] for k in legs}
    kern = {k: [] for k in legs}
    for i in range(3 + reps):
        for k, fn in legs.items():
            if k == "continue":
                cache.copy_(held)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            del out
            if i >= 3:
                call[k].append(dt * 1e6)
                kern[k].append(float(m.last_phase_times().get("predict", float("nan"))) * 1e3)
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.1f us (min %9.1f max %9.1f)" % (med(a), min(a), max(a))
    bytes_moved = rows * (4 * F + 8 * D)
    print("%-16s %8d x %d  %-9s d%d  %4d trees  D=%d  [%d reps]  continue == predict(0, T): %s (max abs diff %.3g)" %
          (name, rows, F, policy, DEPTH, T, D, reps, "bitwise" if same_bits else "NOT bitwise", max_diff))
    for k in legs:
        print("    %-9s call %s   kernel %s" % (k, fmt(call[k]), fmt(kern[k])))
    print("    (a) continue / predict(T-1, T): call %.3f  kernel %.3f   [streaming bound (4F + 8D) / (4F + 4D) = %.3f]" %
          (med(call["continue"]) / med(call["predict1"]), med(kern["continue"]) / med(kern["predict1"]), (4 * F + 8 * D) / (4 * F + 4 * D)))
    print("    (b) predict(0, T) / continue:   call %.1f  kernel %.1f" %
          (med(call["predictT"]) / med(call["continue"]), med(kern["predictT"]) / med(kern["continue"])))
    print("    (c) continue: %.1f MB in the kernel's median time = %.2f TB/s" % (bytes_moved / 1e6, bytes_moved / (med(kern["continue"]) * 1e-6) / 1e12), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    for name in SHAPES:
        rc = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][4]), sys.executable, os.path.abspath(__file__), "--shape", name]).returncode
        if rc != 0:
            print("%s: exit status %d -- stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
