"""A data set bound to another one's thresholds against a data set of its own, and fit_prepared with a validation set against the call without one.

Observations and targets are device tensors (a "cuda" model), so the times are the calls, not PCIe copies.
    (a) own   = prepare_dataset(obs): key transpose, radix selection of the quantiles, class codes.
        bound = prepare_dataset(obs, reference=ds): ONE pass over obs against ds's threshold keys (kern::bin_like), plus the copies of the
                thresholds.  The same rows in both legs; before the timing the bound set's records are compared with ds.codes() byte for byte (a data
                set bound to itself holds its own codes).  bytes = what the bound call must move: 4 n F read + 32 n ceil(F / 16) written.
    (b) plain = a fresh model, fit_prepared(ds, y, T);  valid = a fresh model, fit_prepared(ds, y, T, valid=dsv, valid_targets=yv) with n / 4
                validation rows bound to ds, record only (early_stopping_rounds = 0).  The yardstick for the added time is T x one
                predict_continue_prepared(dsv, base, T - 1, T) call, timed in the same process.  Both legs leave byte-equal model files (checked).
    call = host clock around the call, between two device synchronisations.  The legs alternate in one process; medians of `REPS`, with
    min / max = the spread between repeats.

    python3 scripts/dataset_like_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                         # failure; writes profiles/dataset_like.txt (or FILE) when every shape has run
    python3 scripts/dataset_like_sweep.py --shape NAME   # one shape, in this process
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, DEPTH, BINS = 8, 6, 256
# name: rows, features, iterations of the fit comparison (0: none), time limit of the child (s)
SHAPES = {
    "2^20x128": (1 << 20, 128, 100, 420),
    "65536x128": (65536, 128, 0, 200),
    "4096x16": (4096, 16, 0, 200),
}
REPS = 10


def run(name):
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, T, _ = SHAPES[name]

    def fresh():
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, min_data_in_leaf=0, n_bins=BINS, par_th=10, cv_beta=0.9,
                          split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=rows, grow_policy="oblivious", verbose=0,
                          device="cuda", learner_name="sweep")
        m.set_feature_weights(np.ones(F, np.float32))
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    torch.manual_seed(5)
    xt = torch.randn(rows, F, device="cuda:0", dtype=torch.float32)
    w = torch.randn(F, D, device="cuda:0", dtype=torch.float32) / 8
    yt = (torch.tanh(xt @ w) + 0.3 * torch.randn(rows, D, device="cuda:0", dtype=torch.float32)).contiguous()
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    med = lambda a: float(np.median(a))
    fmt = lambda a: "%9.3f ms (min %9.3f max %9.3f)" % (med(a), min(a), max(a))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def file_bytes(m):
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "m.gbrl_model")
            assert m.save(p) == 0
            with open(p, "rb") as f:
                return f.read()

    print("%-10s %8d x %d  n_bins=%d  [medians of %d, the legs alternating, after one warm-up of each]" % (name, rows, F, BINS, REPS))
    m = fresh()
    ds = m.prepare_dataset(tup(xt))
    bound = m.prepare_dataset(tup(xt), reference=ds)
    same = bound.codes().tobytes() == ds.codes().tobytes() and bound.thresholds().tobytes() == ds.thresholds().tobytes()
    print("    a data set bound to itself: %s   own holds %.1f MiB, bound %.1f MiB" %
          ("byte-equal records and thresholds" if same else "DIFFERENT", ds.nbytes / 2.0 ** 20, bound.nbytes / 2.0 ** 20))
    if not same:
        return 1
    del bound
    own_ms, like_ms = [], []
    for _ in range(REPS):
        own_ms.append(timed(lambda: m.prepare_dataset(tup(xt))))
        like_ms.append(timed(lambda: m.prepare_dataset(tup(xt), reference=ds)))
    moved = 4.0 * rows * F + 32.0 * rows * ((F + 15) // 16)
    spread = max(max(own_ms) - min(own_ms), max(like_ms) - min(like_ms))
    saved = med(own_ms) - med(like_ms)
    print("    prepare_dataset(obs)                call %s" % fmt(own_ms))
    print("    prepare_dataset(obs, reference=ds)  call %s   %.1f MiB moved: %.0f GB/s over the whole call" %
          (fmt(like_ms), moved / 2.0 ** 20, moved / (med(like_ms) * 1e-3) / 1e9))
    print("    bound / own: %.3f   saved %.3f ms (spread between repeats %.3f ms: %s)" %
          (med(like_ms) / med(own_ms), saved, spread, "beyond the spread" if abs(saved) > spread else "NOT beyond the spread"), flush=True)
    # the kernel alone, by the engine's own event pair around the launch
    m.set_profiling(2)
    k_ms = []
    for _ in range(REPS):
        m.prepare_dataset(tup(xt), reference=ds)
        k_ms.append(float(m.last_phase_times().get("bin_like", float("nan"))))
    m.set_profiling(0)
    print("    kern::bin_like alone (event pair)   %s   %.0f GB/s" % (fmt(k_ms), moved / (med(k_ms) * 1e-3) / 1e9), flush=True)
    if T == 0:
        return 0
    # ---- (b) fit_prepared with a validation set of n / 4 rows
    nv = rows // 4
    xv = torch.randn(nv, F, device="cuda:0", dtype=torch.float32)
    yv = (torch.tanh(xv @ w) + 0.3 * torch.randn(nv, D, device="cuda:0", dtype=torch.float32)).contiguous()
    dsv = m.prepare_dataset(tup(xv), reference=ds)
    a, b = fresh(), fresh()
    loss_a = a.fit_prepared(ds, tup(yt), T)
    r = b.fit_prepared(ds, tup(yt), T, valid=dsv, valid_targets=tup(yv))
    same = file_bytes(a) == file_bytes(b) and np.float32(loss_a).tobytes() == np.float32(r["loss"]).tobytes()
    want = np.asarray(b.staged_loss(tup(xv), None, tup(yv), stops=[0, T // 2, T]), np.float64)
    curve_ok = want.tobytes() == r["valid_loss"][[0, T // 2, T]].tobytes()
    print("    fit_prepared, T = %d, %d validation rows: %s; valid_loss[0, T/2, T] %s staged_loss   valid_loss %.7g -> %.7g, best_n_trees %d" %
          (T, nv, "byte-equal model files and loss" if same else "DIFFERENT MODELS", "==" if curve_ok else "!=", r["valid_loss"][0], r["valid_loss"][T],
           r["best_n_trees"]))
    if not (same and curve_ok):
        return 1
    plain_ms, valid_ms, cont_ms = [], [], []
    base = torch.zeros(nv, D, device="cuda:0", dtype=torch.float32)
    b.predict_continue_prepared(dsv, tup(base), T - 1, T)
    for _ in range(REPS):
        ma, mb = fresh(), fresh()
        plain_ms.append(timed(lambda: ma.fit_prepared(ds, tup(yt), T)))
        valid_ms.append(timed(lambda: mb.fit_prepared(ds, tup(yt), T, valid=dsv, valid_targets=tup(yv))))
        cont_ms.append(timed(lambda: b.predict_continue_prepared(dsv, tup(base), T - 1, T)))
    spread = max(max(plain_ms) - min(plain_ms), max(valid_ms) - min(valid_ms))
    added = med(valid_ms) - med(plain_ms)
    print("    fit_prepared(ds, y, T)                      call %s" % fmt(plain_ms))
    print("    fit_prepared(ds, y, T, valid=dsv, ...)      call %s" % fmt(valid_ms))
    print("    predict_continue_prepared(dsv, [T - 1, T))  call %s   T x that = %.3f ms" % (fmt(cont_ms), T * med(cont_ms)))
    print("    valid / plain: %.3f   added %.3f ms = %.3f ms per iteration (spread between repeats %.3f ms: %s)" %
          (med(valid_ms) / med(plain_ms), added, added / T, spread, "beyond the spread" if added > spread else "NOT beyond the spread"), flush=True)
    return 0


HEADER = """# python3 scripts/dataset_like_sweep.py  -- one MI355X; each shape in its own process; observations and targets are device tensors
# own = prepare_dataset(obs); bound = prepare_dataset(obs, reference=ds) on the same rows; valid = fit_prepared with n / 4 validation rows bound to ds, record only
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "dataset_like.txt")
    text, rc = HEADER, 0
    for name in SHAPES:
        child = subprocess.run(["timeout", "-k", "10", str(SHAPES[name][3]), sys.executable, os.path.abspath(__file__), "--shape", name],
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
