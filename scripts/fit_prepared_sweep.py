"""fit_prepared on a prepared data set against fit on the same observations, and predict_continue_prepared against predict_continue (the same build).

Observations, targets and the held prediction are device tensors (a "cuda" model), so the times are the calls, not PCIe copies.
    (a) fit      = a fresh model, fit(obs, None, y, T, shuffle=False): every iteration predicts the batch from the bias through all trees, subtracts
                   the targets and steps (transpose, candidates' thresholds reused, binning, growth).
        prepared = a fresh model, fit_prepared(ds, y, T) on a data set prepared ONCE before the timing (prepare_dataset is timed on its own line):
                   the running prediction is held and advanced by the one new tree, the gradient comes out of the same launch, the step grows on
                   the held codes.  batch_size = n in both legs.
        Before the timing both legs are run once (the warm-up of the shape) and their saved model files are compared byte for byte.
    (b) continue = predict_continue(obs, None, base, a, b) in place on a device base; prepared = predict_continue_prepared(ds, base, a, b), for
                   one tree ([T - 1, T)) and for 100 ([0, 100)) of the model (a) left.
    call = host clock around the call, between two device synchronisations.  The two legs alternate in one process; medians of `REPS`, with
    min / max = the spread between repeats.

    python3 scripts/fit_prepared_sweep.py [--out FILE]   # every shape, each in a child process of its own under a time limit; stops at the first
                                                         # failure; writes profiles/fit_prepared.txt (or FILE) when every shape has run
    python3 scripts/fit_prepared_sweep.py --shape NAME   # one shape, in this process
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, DEPTH, BINS = 8, 6, 256
# name: rows, features, iterations, also time the continue calls, time limit of the child (s)
SHAPES = {
    "2^20x128_T100": (1 << 20, 128, 100, True, 420),
    "65536x128_T1000": (65536, 128, 1000, False, 420),
    "4096x16_T200": (4096, 16, 200, False, 200),      # nothing is saved in binning here, only the quadratic predict
}
REPS = 10


def run(name):
    import numpy as np
    import torch
    import gbrl_amd
    rows, F, T, cont, _ = SHAPES[name]

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

    print("%-18s %8d x %d  oblivious L2 d%d  D=%d  n_bins=%d  T=%d  batch_size=n  [medians of %d, the legs alternating, after one warm-up of each]" %
          (name, rows, F, DEPTH, D, BINS, T, REPS))
    prep_ms = [timed(lambda: fresh().prepare_dataset(tup(xt))) for _ in range(4)][1:]
    ds = fresh().prepare_dataset(tup(xt))
    print("    prepare_dataset (once, not in the times below)  call %s   holds %.1f MiB" % (fmt(prep_ms), ds.nbytes / 2.0 ** 20))
    # warm-up of both legs, and the check that they leave the same model
    a, b = fresh(), fresh()
    loss_a = a.fit(tup(xt), None, tup(yt), T, False, "MultiRMSE")
    loss_b = b.fit_prepared(ds, tup(yt), T)
    same = file_bytes(a) == file_bytes(b) and np.float32(loss_a).tobytes() == np.float32(loss_b).tobytes()
    print("    the two models after %d trees: %s   loss %.7g / %.7g" % (a.get_num_trees(), "byte-equal model files" if same else "DIFFERENT", loss_a, loss_b))
    if not same:
        return 1
    fit_ms, prepared_ms = [], []
    for _ in range(REPS):
        ma, mb = fresh(), fresh()
        fit_ms.append(timed(lambda: ma.fit(tup(xt), None, tup(yt), T, False, "MultiRMSE")))
        prepared_ms.append(timed(lambda: mb.fit_prepared(ds, tup(yt), T)))
    spread = max(max(fit_ms) - min(fit_ms), max(prepared_ms) - min(prepared_ms))
    print("    fit(obs, None, y, T)      call %s   %.3f ms per iteration" % (fmt(fit_ms), med(fit_ms) / T))
    print("    fit_prepared(ds, y, T)    call %s   %.3f ms per iteration" % (fmt(prepared_ms), med(prepared_ms) / T))
    saved = med(fit_ms) - med(prepared_ms)
    print("    fit_prepared / fit: %.3f   saved %.3f ms (spread between repeats %.3f ms: %s)" %
          (med(prepared_ms) / med(fit_ms), saved, spread, "beyond the spread" if saved > spread else "NOT beyond the spread"), flush=True)
    if cont:
        m = b
        for lo, hi in ((T - 1, T), (0, min(T, 100))):
            base = torch.zeros(rows, D, device="cuda:0", dtype=torch.float32)
            m.predict_continue(tup(xt), None, tup(base), lo, hi)
            m.predict_continue_prepared(ds, tup(base), lo, hi)
            p1 = torch.zeros_like(base)
            p2 = torch.zeros_like(base)
            m.predict_continue(tup(xt), None, tup(p1), lo, hi)
            m.predict_continue_prepared(ds, tup(p2), lo, hi)
            if not torch.equal(p1.view(torch.int32), p2.view(torch.int32)):
                print("    continue [%d, %d): DIFFERENT bits" % (lo, hi))
                return 1
            c_ms, cp_ms = [], []
            for _ in range(REPS):
                base.zero_()
                c_ms.append(timed(lambda: m.predict_continue(tup(xt), None, tup(base), lo, hi)))
                base.zero_()
                cp_ms.append(timed(lambda: m.predict_continue_prepared(ds, tup(base), lo, hi)))
            sp = max(max(c_ms) - min(c_ms), max(cp_ms) - min(cp_ms))
            print("    predict_continue(obs, ...)        [%3d, %3d)  call %s" % (lo, hi, fmt(c_ms)))
            print("    predict_continue_prepared(ds, ...) [%3d, %3d)  call %s   prepared / obs: %.3f (spread %.3f ms), the same bits" %
                  (lo, hi, fmt(cp_ms), med(cp_ms) / med(c_ms), sp), flush=True)
    return 0


HEADER = """# python3 scripts/fit_prepared_sweep.py  -- one MI355X; each shape in its own process; observations, targets and held predictions are device tensors
# fit = fit(obs, None, y, T, shuffle=False) on a fresh model; fit_prepared = fit_prepared(ds, y, T) on a fresh model and a data set prepared once; batch_size = n
# call = host clock around the call, between two device synchronisations; medians over the repetitions, min / max = the spread; the legs alternate in one process
"""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        return run(sys.argv[2])
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "fit_prepared.txt")
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
