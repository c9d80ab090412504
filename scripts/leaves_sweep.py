"""predict_leaves / leaf_counts -- where a row lands -- against predict_continue over the same tree range on the same rows: the same walk plus the
value gather and the chain, measured in the same run of the same build.

Rows, the held prediction and the leaf matrix are device tensors (a "cuda" model: predict_leaves returns its [n, T] int32 capsule on the device,
a fresh allocation per call), so the times are the calls, not PCIe copies; leaf_counts returns its n_leaves int64 to the host, which is part of the
call.  Per shape: warm-up rounds, then `reps` timed rounds of each leg, interleaved.
    call    = host clock around the call (it returns after the stream has been synchronised).
    kernel  = the library's HIP-event bracket around the traversal kernels (set_profiling(1), last_phase_times()["predict"]): k_leaves; the
              counter memset + every k_leaf_counts launch (one per run of trees whose leaves fit GBRL.leaf_counts_chunk() counters); k_continue.
Medians, with min / max = the spread between repeats.  Byte floors, from the shape (no hardware counters): predict_leaves n (4F + 4T); leaf_counts
4nF per tree chunk; predict_continue n (4F + 8D) -- each over the device-to-device copy rate measured in the same process (a 512 MiB float32
tensor copied by torch: 2 x 512 MiB moved per copy).  The leaf matrix is compared with the counts (bincount on the device) before timing.

    python3 scripts/leaves_sweep.py [--out FILE]    # every shape, each in a child process of its own under a time limit; stops at the first failure;
                                                    # writes profiles/leaves.txt (or FILE) when every shape has run
    python3 scripts/leaves_sweep.py --shape NAME    # one shape, in this process
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
    for t in range(trees):
        m.step(X, None, Gs[t % len(Gs)])
    T = m.get_num_trees()
    assert T == trees
    e = m.get_ensemble_data()
    ti = np.asarray(e["tree_indices"])
    n_leaves = int(np.asarray(e["values"]).shape[0])
    chunk = gbrl_amd.GBRL.leaf_counts_chunk()
    # the runs leaf_counts cuts the range into (kern::leaf_counts: whole trees, at most `chunk` leaves each)
    first = np.append(ti, n_leaves)
    chunks, a = 0, 0
    while a < T:
        b = a
        while b < T and first[b + 1] - first[a] <= chunk:
            b += 1
        a = max(b, a + 1)
        chunks += 1
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    arg = tup(xt)
    bias = torch.from_numpy(np.asarray(m.get_bias(), np.float32)).to("cuda:0")
    cache = bias.repeat(rows, 1).contiguous()
    carg = tup(cache)
    # the copy rate of this process
    src = torch.empty(128 << 20, device="cuda:0", dtype=torch.float32)
    dst = torch.empty_like(src)
    copy_us = []
    for i in range(13):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        if i >= 3:
            copy_us.append((time.perf_counter() - t0) * 1e6)
    copy_rate = 2 * src.numel() * 4 / (float(np.median(copy_us)) * 1e-6)      # bytes per second
    del src, dst
    legs = {"leaves": lambda: m.predict_leaves(arg, None, 0, T),
            "counts": lambda: m.leaf_counts(arg, None, 0, T),
            "continue": lambda: m.predict_continue(arg, None, carg, 0, T)}
    # the two calls agree with each other: reported, not assumed
    lv = torch.from_dlpack(legs["leaves"]())
    binc = torch.bincount(lv.reshape(-1).long(), minlength=n_leaves).cpu().numpy().astype(np.int64)
    del lv
    c1, c2 = legs["counts"](), legs["counts"]()
    agree = bool(np.array_equal(binc, c1))
    same_bytes = c1.tobytes() == c2.tobytes()
    m.set_profiling(1)
    call = {k: [] for k in legs}
    kern = {k: [] for k in legs}
    for i in range(2 + reps):
        for k, fn in legs.items():
            if k == "continue":
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
    floor = {"leaves": rows * (4 * F + 4 * T), "counts": 4 * rows * F * chunks, "continue": rows * (4 * F + 8 * D)}
    print("%-14s %8d x %d  %-9s d%d  %4d trees  %6d leaves  D=%d  [%d reps]  copy rate %.2f TB/s  leaf_counts: %d chunk(s) of <= %d counters" %
          (name, rows, F, policy, DEPTH, T, n_leaves, D, reps, copy_rate / 1e12, chunks, chunk))
    print("    leaf_counts == bincount(predict_leaves): %s; two leaf_counts calls: %s" % ("equal" if agree else "DIFFERENT", "same bytes" if same_bytes else "DIFFERENT bytes"))
    for k, label in (("leaves", "predict_leaves"), ("counts", "leaf_counts"), ("continue", "predict_continue")):
        fl = floor[k] / copy_rate * 1e3
        print("    %-16s call %s   kernel %s   floor %8.1f MB = %7.3f ms: kernel / floor %6.2f" %
              (label, fmt(call[k]), fmt(kern[k]), floor[k] / 1e6, fl, med(kern[k]) / fl))
    print("    predict_leaves / predict_continue: call %.2f  kernel %.2f     leaf_counts / predict_continue: call %.2f  kernel %.2f" %
          (med(call["leaves"]) / med(call["continue"]), med(kern["leaves"]) / med(kern["continue"]),
           med(call["counts"]) / med(call["continue"]), med(kern["counts"]) / med(kern["continue"])), flush=True)


HEADER = """# python3 scripts/leaves_sweep.py  -- one MI355X; each shape in its own process; rows, the held prediction and the leaf matrix are device tensors
# predict_leaves = the [n, T] int32 matrix of a "cuda" model (k_leaves); leaf_counts = int64 [n_leaves] on the host (memset + one k_leaf_counts launch per tree chunk);
# predict_continue = the yardstick over the same range on the same rows (k_continue: the same walk plus the value gather and the chain); medians over the repetitions, min / max = the spread
# call = host clock around the call (ends in a stream synchronise); kernel = HIP events around the traversal kernels (set_profiling(1)); floor = bytes from the shape over the copy rate of the same process
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "leaves.txt")
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
