"""staged_loss / predict_staged -- every ensemble prefix in one walk -- against what a caller can do without them: a loop of predict_continue over
consecutive stops on a device-resident held prediction, with a device-side loss after each stop.

Rows, targets and the held prediction are device tensors, so the times are the calls, not PCIe copies.  Per shape: warm-up rounds, then `reps`
timed rounds of each leg, interleaved.
    staged   = one staged_loss(X, None, Y, stops) call: host clock around the call (it returns after the stream has been synchronised and the
               len(stops) doubles have arrived).
    loop     = cache <- tiled bias; for consecutive stops (a, b): predict_continue(X, None, cache, a, b) in place, then
               S = ((cache - Y).double() ** 2).sum() on the device and a device synchronise (the next in-place update must not overtake the
               loss that reads the cache; a loop on a loss threshold reads the value here anyway); host clock around the whole loop.
               The loss is the plain torch expression, several kernels with float64 temporaries, not a fused one: the ratio is the call
               against the loop as a user would write it, not kernel against kernel.
    predict  = one predict_staged(X, None, stops) call of a "cuda" model (the [stages, n, D] result stays on the device).
    kernel   = the library's HIP-event bracket around the staged kernels (set_profiling(1), last_phase_times()["predict"]): k_staged (+ k_staged_finish).
Medians, with min / max = the spread between repeats.  Bytes: what the algorithm needs, computed from the shape -- loss mode n (4F + 4D) +
16 stages ceil(n / 64) (the partials written and read once), predict mode n (4F + 4D stages) -- over the kernel's median time; hardware
counters are not collected here.  The staged losses are compared with the loop's (same predictions bit for bit, another summation order).

    python3 scripts/staged_sweep.py                 # every shape, each in a child process of its own under a time limit; stops at the first failure
    python3 scripts/staged_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

F, D, DEPTH = 128, 8, 6
# name: rows, policy, trees, every k-th tree is a stop, repetitions, time limit of the child (s)
SHAPES = {
    "obl100_every_2^20": (1 << 20, "oblivious", 100, 1, 10, 400),
    "obl1000_every10th_65536": (65536, "oblivious", 1000, 10, 10, 400),
    "grd10_every_2^20": (1 << 20, "greedy", 10, 1, 10, 400),
}


def run(name):
    import numpy as np
    import torch
    import cases as K
    import gbrl_amd
    rows, policy, trees, every, reps, _ = SHAPES[name]
    case = dict(name="st", seed=11, N=4096, F=F, Fc=0, D=D, depth=DEPTH, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
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
    stops = list(range(every, T + 1, every))
    S = len(stops)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    yt = torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    arg, yarg = tup(xt), tup(yt)
    bias = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).to("cuda:0")
    cache = bias.repeat(rows, 1).contiguous()
    carg = tup(cache)

    def loop():
        cache.copy_(bias.repeat(rows, 1))
        out, a = [], 0
        for b in stops:
            m.predict_continue(arg, None, carg, a, b)
            out.append(((cache - yt).double() ** 2).sum())
            torch.cuda.synchronize()
            a = b
        return np.sqrt(0.5 * torch.stack(out).cpu().numpy() / rows)

    legs = {"staged": lambda: m.staged_loss(arg, None, yarg, stops), "loop": loop, "predict": lambda: m.predict_staged(arg, None, stops)}
    # the feature computes what the loop computes: reported, not assumed
    ls, ll = legs["staged"](), legs["loop"]()
    rel = float(np.max(np.abs(ls - ll) / ll))
    last = torch.from_dlpack(legs["predict"]())[-1]
    same_bits = bool(torch.equal(last, cache))
    del last
    same_bytes = legs["staged"]().tobytes() == ls.tobytes()
    m.set_profiling(1)
    call = {k: [] for k in legs}
    kern = {k: [] for k in legs}
    for i in range(2 + reps):
        for k, fn in legs.items():
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
    nb = (rows + 63) // 64
    loss_bytes = rows * (4 * F + 4 * D) + 16 * S * nb
    pred_bytes = rows * (4 * F + 4 * D * S)
    print("%-24s %8d x %d  %-9s d%d  %4d trees  D=%d  %d stages (every %d)  [%d reps]" % (name, rows, F, policy, DEPTH, T, D, S, every, reps))
    print("    staged_loss vs the loop's losses: max rel diff %.3g; two staged_loss calls: %s; predict_staged[-1] vs the loop's final cache: %s" %
          (rel, "same bytes" if same_bytes else "DIFFERENT bytes", "bitwise" if same_bits else "NOT bitwise"))
    print("    staged   call %s   kernel %s" % (fmt(call["staged"]), fmt(kern["staged"])))
    print("    loop     call %s   (%d predict_continue calls + %d device losses)" % (fmt(call["loop"]), S, S))
    print("    predict  call %s   kernel %s" % (fmt(call["predict"]), fmt(kern["predict"])))
    print("    loop / staged_loss: %.2f" % (med(call["loop"]) / med(call["staged"])))
    print("    staged_loss kernels:    %8.1f MB needed, %.3f TB/s over the kernel's median time" %
          (loss_bytes / 1e6, loss_bytes / (med(kern["staged"]) * 1e-3) / 1e12))
    print("    predict_staged kernel:  %8.1f MB needed, %.3f TB/s over the kernel's median time" %
          (pred_bytes / 1e6, pred_bytes / (med(kern["predict"]) * 1e-3) / 1e12), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    for name in SHAPES:
        rc = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][5]), sys.executable, os.path.abspath(__file__), "--shape", name]).returncode
        if rc != 0:
            print("%s: exit status %d -- stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
