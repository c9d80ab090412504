"""staged_loss_prepared -- every ensemble prefix on a prepared data set in one walk -- against the loop it replaces: predict_continue_prepared over
consecutive stops on a device-resident held prediction plus objective_gradient for the loss of each stop.

The shapes are those of profiles/staged.txt (scripts/staged_sweep.py): 2^20 x 128 with 100 trees and a stop at every tree, 65 536 x 128 with 1000
trees and a stop at every 10th; D = 8, depth 6.  The model is grown by fit_prepared on 4096 rows; the evaluated rows are another data set on its
thresholds (prepare_dataset(X, reference=ds)), binned once outside the timed region.  Targets and the held prediction are device tensors.
    staged   = one staged_loss_prepared(dsv, Y, stops, objective) call: host clock around the call (it returns after the stream has been
               synchronised and the len(stops) doubles have arrived).
    loop     = cache <- tiled bias (one device copy of a matrix tiled beforehand); for consecutive stops (a, b): predict_continue_prepared(dsv, cache, a, b) in place, then
               objective_gradient(cache, Y, objective)[1], which ends in a synchronise and returns the loss; host clock around the whole loop.
    predict  = one predict_staged_prepared(dsv, stops) call of a "cuda" model (rmse leg only; the [stages, n, D] result stays on the device).
    kernel   = the library's HIP-event bracket around the staged kernels (set_profiling(1), last_phase_times()["predict"]).
Legs alternate in one process; 2 warm-up rounds, then `reps` timed ones; medians with min / max = the spread between repeats, and the ratio's
spread from the per-round ratios.  The staged losses are compared with the loop's (same row losses, same reduction: equal bytes are expected).

    python3 scripts/staged_prepared_sweep.py                 # every shape, each in a child process of its own under a time limit; stops at the first failure
    python3 scripts/staged_prepared_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, D, DEPTH, NFIT = 128, 8, 6, 4096
# name: rows, trees, every k-th tree is a stop, objective, repetitions, time limit of the child (s)
SHAPES = {
    "rmse100_every_2^20": (1 << 20, 100, 1, "rmse", 10, 400),
    "logistic100_every_2^20": (1 << 20, 100, 1, "logistic", 10, 400),
    "rmse1000_every10th_65536": (65536, 1000, 10, "rmse", 10, 500),
    "logistic1000_every10th_65536": (65536, 1000, 10, "logistic", 10, 500),
}


def run(name):
    import numpy as np
    import torch
    import gbrl_amd
    rows, trees, every, objective, reps, _ = SHAPES[name]
    rng = np.random.default_rng(11)
    X = rng.standard_normal((NFIT, F)).astype(np.float32)
    S0 = X[:, :D] + 0.5 * rng.standard_normal((NFIT, D)).astype(np.float32)
    Y = np.ascontiguousarray((S0 > 0).astype(np.float32) if objective == "logistic" else S0)
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=64, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cuda", batch_size=NFIT)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, Y, trees, objective=objective)
    T = m.get_num_trees()
    assert T == trees
    stops = list(range(every, T + 1, every))
    S = len(stops)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    yt = (torch.rand(rows, D, device="cuda:0") > 0.5).float() if objective == "logistic" else torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    dsv = m.prepare_dataset(tup(xt), reference=ds)
    del xt
    yarg = tup(yt)
    bias = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).to("cuda:0")
    tiled = bias.repeat(rows, 1).contiguous()
    cache = tiled.clone()
    carg = tup(cache)

    def loop():
        cache.copy_(tiled)   # (the held prediction starts at the bias: one device copy, no allocation, inside the timed region)
        out, a = [], 0
        for b in stops:
            m.predict_continue_prepared(dsv, carg, a, b)
            out.append(m.objective_gradient(carg, yarg, objective)[1])
            a = b
        return np.asarray(out, np.float64)

    legs = {"staged": lambda: m.staged_loss_prepared(dsv, yarg, stops, objective)["loss"], "loop": loop}
    if objective == "rmse":
        legs["predict"] = lambda: m.predict_staged_prepared(dsv, stops)
    ls, ll = legs["staged"](), legs["loop"]()
    rel = float(np.max(np.abs(ls - ll) / ll))
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
    ratios = [l / s for l, s in zip(call["loop"], call["staged"])]
    G, nb = (F + 15) // 16, (rows + 63) // 64
    loss_bytes = rows * (32 * G + 4 * D) + 16 * S * nb
    print("%-30s %8d x %d  oblivious d%d  %4d trees  D=%d  %-8s %d stages (every %d)  [%d reps]" % (name, rows, F, DEPTH, T, D, objective, S, every, reps))
    print("    staged_loss_prepared vs the loop's losses: max rel diff %.3g (%s); two staged calls: %s" %
          (rel, "same bytes" if ls.tobytes() == ll.tobytes() else "different bytes", "same bytes" if same_bytes else "DIFFERENT bytes"))
    print("    staged   call %s   kernel %s" % (fmt(call["staged"]), fmt(kern["staged"])))
    print("    loop     call %s   (%d predict_continue_prepared calls + %d objective_gradient calls)" % (fmt(call["loop"]), S, S))
    if "predict" in legs:
        print("    predict  call %s   kernel %s" % (fmt(call["predict"]), fmt(kern["predict"])))
    print("    loop / staged_loss_prepared: %.2f (per-round ratios min %.2f max %.2f)" % (med(call["loop"]) / med(call["staged"]), min(ratios), max(ratios)))
    print("    staged kernels: %8.1f MB needed, %.3f TB/s over the kernel's median time" % (loss_bytes / 1e6, loss_bytes / (med(kern["staged"]) * 1e-3) / 1e12),
          flush=True)


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
