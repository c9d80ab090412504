"""step_prepared on a prepared data set against step on the same observations (the same build), prepare_dataset itself, and a row subset
against a step on the gathered matrix.

Observations, gradients and row indices are device tensors (a "cuda" model), so the times are the calls, not PCIe copies.  Per shape two equal
fresh models are stepped ALTERNATELY in one process -- one with step(obs, None, grads), the other with step_prepared(ds, grads) on a data set
prepared once -- with the same gradients, so both grow the same trees (checked: the ensembles' bytes are compared at the end).
    call    = host clock around the call, between two device synchronisations.
    prepare = prepare_dataset(obs) of a fresh data set (it waits for its stream before it returns), the data set dropped again.
    subset  = step_prepared(ds, grads[m], rows) with m of the n rows (a random choice without replacement, ascending) against step on the
              gathered [m, F] matrix.  The two grow DIFFERENT trees (the data set's thresholds against the subset's own quantiles): only
              the times are compared.
Medians of `reps` after `warm` warm-up rounds, with min / max = the spread between repeats.

    python3 scripts/prepared_step_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                          # failure; writes profiles/prepared_step.txt (or FILE) when every shape has run
    python3 scripts/prepared_step_sweep.py --shape NAME   # one shape, in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

D, DEPTH, BINS = 8, 6, 256
AC_OPTS = [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=7), dict(algo="SGD", scheduler="Const", init_lr=0.01, start_idx=7, stop_idx=8)]
ONE_OPT = [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)]
# name: rows, features, policy, score, optimisers, subset rows (0: none), time limit of the child (s)
SHAPES = {
    "cfg2_2^20x128": (1 << 20, 128, "oblivious", "L2", ONE_OPT, 0, 300),        # BASELINE.md configs[1]
    "cfg3_2^20x128": (1 << 20, 128, "greedy", "Cosine", AC_OPTS, 0, 300),       # BASELINE.md configs[2]
    "cfg2_4096x16": (4096, 16, "oblivious", "L2", ONE_OPT, 0, 120),
    "cfg3_4096x16": (4096, 16, "greedy", "Cosine", AC_OPTS, 0, 120),
    "cfg2_subset_2^18_of_2^20": (1 << 20, 128, "oblivious", "L2", ONE_OPT, 1 << 18, 300),
}
REPS, WARM = 10, 3


def run(name):
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, policy, score, opts, sub, _ = SHAPES[name]

    def fresh():
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func=score, generator_type="Quantile", use_control_variates=False, batch_size=rows, grow_policy=policy, verbose=0,
                          device="cuda", learner_name="sweep")
        m.set_feature_weights(np.ones(F, np.float32))
        for o in opts:
            m.set_optimizer(**o)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(5)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    gt = (torch.tanh(xt @ w) + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%8.3f ms (min %8.3f max %8.3f)" % (med(a), min(a), max(a))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    a, b = fresh(), fresh()
    prep_ms = []
    for i in range(WARM + REPS):
        dt = timed(lambda: b.prepare_dataset(tup(xt)))                 # (the returned data set is dropped inside the timed region)
        if i >= WARM:
            prep_ms.append(dt)
    ds = b.prepare_dataset(tup(xt))
    print("%-26s %8d x %d  %-9s %-6s d%d  D=%d  n_bins=%d  [%d reps after %d]" % (name, rows, F, policy, score, DEPTH, D, BINS, REPS, WARM))
    print("    prepare_dataset           call %s   holds %.1f MiB" % (fmt(prep_ms), ds.nbytes / 2.0 ** 20))
    if sub == 0:
        step_ms, prepared_ms = [], []
        for i in range(WARM + REPS):                                    # the two legs alternate
            dt_a = timed(lambda: a.step(tup(xt), None, tup(gt)))
            dt_b = timed(lambda: b.step_prepared(ds, tup(gt)))
            if i >= WARM:
                step_ms.append(dt_a)
                prepared_ms.append(dt_b)
        ea, eb = a.get_ensemble_data(), b.get_ensemble_data()
        same = all(np.asarray(ea[k]).tobytes() == np.asarray(eb[k]).tobytes() for k in ea if hasattr(ea[k], "shape"))
        print("    the two models after %d trees: %s" % (a.get_num_trees(), "the same bytes" if same else "DIFFERENT"))
        print("    step(obs, None, grads)    call %s" % fmt(step_ms))
        print("    step_prepared(ds, grads)  call %s" % fmt(prepared_ms))
        saved, spread = med(step_ms) - med(prepared_ms), max(max(step_ms) - min(step_ms), max(prepared_ms) - min(prepared_ms))
        pays = "prepare_dataset pays for itself after %.1f steps" % (med(prep_ms) / saved) if saved > spread else \
            "no saving beyond the spread between repeats (%.3f ms)" % spread
        print("    step_prepared / step: %.3f   saved per step %.3f ms   %s" % (med(prepared_ms) / med(step_ms), saved, pays), flush=True)
        return 0 if same else 1
    idx = torch.sort(torch.randperm(rows, device="cuda:0")[:sub]).values.to(torch.int32).contiguous()
    xs = xt[idx.long()].contiguous()
    gs = gt[idx.long()].contiguous()
    step_ms, prepared_ms = [], []
    for i in range(WARM + REPS):
        dt_a = timed(lambda: a.step(tup(xs), None, tup(gs)))
        dt_b = timed(lambda: b.step_prepared(ds, tup(gs), rows=tup(idx)))
        if i >= WARM:
            step_ms.append(dt_a)
            prepared_ms.append(dt_b)
    print("    step(obs[rows], None, grads)     %d rows   call %s" % (sub, fmt(step_ms)))
    print("    step_prepared(ds, grads, rows)   %d rows   call %s" % (sub, fmt(prepared_ms)))
    print("    step_prepared / step: %.3f   saved per step %.3f ms" % (med(prepared_ms) / med(step_ms), med(step_ms) - med(prepared_ms)), flush=True)
    return 0


HEADER = """# python3 scripts/prepared_step_sweep.py  -- one MI355X; each shape in its own process; observations, gradients and row indices are device tensors
# step = step(obs, None, grads); step_prepared = the same gradients on a data set prepared once from the same observations; the two legs alternate in one process
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "prepared_step.txt")
    text, rc = HEADER, 0
    for name in SHAPES:
        child = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][6]), sys.executable, os.path.abspath(__file__), "--shape", name],
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
