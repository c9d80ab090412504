"""tree_gram_prepared -- the Gram matrix of the per-tree outputs over a data set -- against the loop it replaces, in the same run of the same build:
predict_leaves_prepared, a torch gather of the float32 leaf values, and a float64 matmul on the device, over row chunks small enough that the
[rows, T * D] float64 intermediate stays under 1 GiB.

The trees are grown by step_prepared on a 4096-row data set; the timed data set is bound to it.  Before timing the two results are compared within the
tests' bound, (rows * D + 8) * 2^-53 * sum |v_t v_u| per entry with the right-hand sums computed from the gathered values, and GBRL_HIP_GRAM_GENERIC=1
against the streaming kernel within the same bound at a row subset.  Per shape: 2 warm-up rounds, then `reps` timed
rounds, the legs alternating within a round.
    call    = host clock around the call (it ends in a stream synchronise; the yardstick synchronises after its last matmul).
    kernel  = the library's HIP-event bracket around k_tree_gram + k_gram_reduce (set_profiling(1), last_phase_times()["predict"]).
    of peak = rows * D * T * (T + 1) useful float64 flops (the upper triangle) per kernel second, over 78.6 TFLOP/s (MI355X float64 matrix peak).
Medians, with min / max = the spread between repeats.

    python3 scripts/tree_gram_sweep.py [--out FILE]    # every shape, each in a child process under a time limit; stops at the first failure
    python3 scripts/tree_gram_sweep.py --shape NAME    # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

F, D, DEPTH, PEAK = 128, 8, 6, 78.6e12
# name: rows, policy, trees, repetitions, time limit of the child (s)  (the family's four)
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
    case = dict(name="gram", seed=11, N=4096, F=F, Fc=0, D=D, depth=DEPTH, n_bins=64, score="Cosine" if policy == "greedy" else "L2", gen="Quantile",
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
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    yt = torch.randn(rows, D, device="cuda:0", dtype=torch.float32)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    ds = m.prepare_dataset(tup(xt), reference=train)
    values = torch.from_numpy(np.asarray(m.get_ensemble_data()["values"], np.float32).reshape(-1, D)).to("cuda:0")
    chunk = max(64, min(rows, (1 << 30) // (8 * T * D)))
    plan = gbrl_amd.gbrl_cpp.tree_gram_geometry(rows, T, D, (F + 15) // 16)

    def yardstick(caps=False):
        """the Gram and the moments; caps: also sum |v_t v_u| and sum |v_t y|, the right-hand sides of the bound (the check before timing only)"""
        gram = torch.zeros(T, T, device="cuda:0", dtype=torch.float64)
        mom = torch.zeros(T, device="cuda:0", dtype=torch.float64)
        cap, capm = torch.zeros_like(gram), torch.zeros_like(mom)
        for r0 in range(0, rows, chunk):
            idx = torch.arange(r0, min(rows, r0 + chunk), device="cuda:0", dtype=torch.int32)
            L = torch.from_dlpack(m.predict_leaves_prepared(ds, 0, T, rows=tup(idx))).long()
            V = values[L].double()                                  # [c, T, D]
            A = V.permute(1, 0, 2).reshape(T, -1)                   # [T, c * D]
            y = yt[r0:r0 + len(idx)].double().reshape(-1)
            gram += A @ A.t()
            mom += A @ y
            if caps:
                cap += A.abs() @ A.abs().t()
                capm += A.abs() @ y.abs()
        torch.cuda.synchronize()
        out = (gram.cpu().numpy(), mom.cpu().numpy())
        return out + (cap.cpu().numpy(), capm.cpu().numpy()) if caps else out

    legs = {"tree_gram_prepared": lambda: m.tree_gram_prepared(ds, tup(yt)), "leaves + gather + matmul": yardstick}
    # before timing: both results within the tests' bound of the yardstick, the right-hand sums computed from the gathered values
    bound = lambda n: (n * D + 8) * 2.0 ** -53
    r, (g0, m0, cap, capm) = legs["tree_gram_prepared"](), yardstick(caps=True)
    assert r["route"] == "stream" and (np.abs(r["gram"] - g0) <= bound(rows) * cap).all(), "the Gram matrices differ"
    assert (np.abs(r["moment"] - m0) <= bound(rows) * capm).all(), "the moments differ"
    worst = max((np.abs(r["gram"] - g0) / np.maximum(bound(rows) * cap, 1e-300)).max(), (np.abs(r["moment"] - m0) / np.maximum(bound(rows) * capm, 1e-300)).max())
    sub = torch.arange(0, 4096, device="cuda:0", dtype=torch.int32)
    a = m.tree_gram_prepared(ds, rows=tup(sub))
    os.environ["GBRL_HIP_GRAM_GENERIC"] = "1"
    b = m.tree_gram_prepared(ds, rows=tup(sub))
    del os.environ["GBRL_HIP_GRAM_GENERIC"]
    Ls = torch.from_dlpack(m.predict_leaves_prepared(ds, 0, T, rows=tup(sub))).long()
    As = values[Ls].double().abs().permute(1, 0, 2).reshape(T, -1)
    caps_sub = (As @ As.t()).cpu().numpy()
    assert b["route"] == "general" and (np.abs(a["gram"] - b["gram"]) <= bound(4096) * caps_sub).all(), "the two kernels differ"
    m.set_profiling(1)
    call = {k: [] for k in legs}
    kern = []
    for i in range(2 + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            del out
            if i >= 2:
                call[k].append(dt * 1e3)
                if k == "tree_gram_prepared":
                    kern.append(float(m.last_phase_times().get("predict", float("nan"))))
    med = lambda v: float(np.median(v))
    fmt = lambda v: "%9.3f ms (min %9.3f max %9.3f)" % (med(v), min(v), max(v))
    print("%-14s %8d x %d  %-9s d%d  %4d trees  D=%d  [%d reps]  plan: %d pairs x %d row blocks, %.1f MiB scratch, %d bytes of LDS; yardstick in chunks of %d rows" %
          (name, rows, F, policy, DEPTH, T, D, reps, plan["pairs"], plan["row_blocks"], plan["scratch_bytes"] / 2 ** 20, plan["lds_bytes"], chunk))
    print("    outputs before timing: |tree_gram_prepared - yardstick| <= (rows * D + 8) * 2^-53 * sum |v_t v_u| per entry, Gram and moments (worst %.3f of it); "
          "GBRL_HIP_GRAM_GENERIC=1 against the streaming kernel likewise on 4096 rows" % worst)
    print("    %-26s call %s   kernel %s" % ("tree_gram_prepared", fmt(call["tree_gram_prepared"]), fmt(kern)))
    print("    %-26s call %s" % ("leaves + gather + matmul", fmt(call["leaves + gather + matmul"])))
    flops = float(rows) * D * T * (T + 1)
    print("    tree_gram_prepared / yardstick: call %.3f     useful float64 rate %.2f TFLOP/s = %.4f of peak" %
          (med(call["tree_gram_prepared"]) / med(call["leaves + gather + matmul"]), flops / (med(kern) * 1e-3) / 1e12, flops / (med(kern) * 1e-3) / PEAK), flush=True)


HEADER = """# python3 scripts/tree_gram_sweep.py  -- one MI355X; each shape in its own process; the data set, the targets and the yardstick's tensors are on the device
# tree_gram_prepared = k_tree_gram (row walk -> float64 operands in LDS -> v_mfma_f64_16x16x4_f64) + k_gram_reduce, the tiles read back and mirrored on the host
# yardstick = predict_leaves_prepared(rows=chunk) + values[leaves] + float64 matmul per row chunk (intermediate under 1 GiB)
# call = host clock around the call; kernel = HIP events around the two launches (set_profiling(1)); medians over the repetitions, min / max = the spread
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run(sys.argv[2])
        return 0
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "tree_gram.txt")
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
