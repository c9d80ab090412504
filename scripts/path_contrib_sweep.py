"""Measurements of path_importance_prepared (profiles/path_contrib.txt).

    python scripts/path_contrib_sweep.py [--reps 10] [--leg-budget 40] [--no-shap] > profiles/path_contrib.txt

D = 8, depth 6, 256 bins, oblivious / L2 at 2^20 x 128 with 10 and 100 trees, 65 536 x 128 with 1000 trees and 4096 x 16 with 100 trees.  Per shape,
in ONE process, legs alternating, medians of --reps runs with (min .. max):
  path        path_importance_prepared(ds): the call, and its kernel phase `path_rows` alone under set_profiling(2)
  continue    one predict_continue_prepared call over the same rows and trees, device base in place: the walk the kernel is built on
  shap        shap_importance_prepared(ds) on the same model and rows: the exact attribution, the time to beat
Before anything is timed the streaming kernel's sums are compared byte for byte with the one-thread-per-row kernel's (GBRL_HIP_PATH_GENERIC=1).  A leg
whose runs would pass --leg-budget seconds is repeated fewer times and the count is printed.  Also printed: the used features, the slots per pass
and the feature passes of the streaming kernel's plan.
bench.py is not part of this script: the flagship workload is compared by running `python bench.py --gpus 1 --steps 10 --warmup 2` from a checkout
of the previous commit and from this one in turn, one process each, three a side, and reading the trees/s of the JSON lines."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
import cases as K  # noqa: E402
import gbrl_amd  # noqa: E402

f32 = np.float32
D, DEPTH, BINS = 8, 6, 256
DEV = torch.device("cuda:0")
LEG_BUDGET_S = 40.0


def arg(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(legs, reps):
    times = {k: [] for k in legs}
    count = {}
    for k, fn in legs.items():                      # warm-up, and what one run of the leg costs
        count[k] = max(1, min(reps, int(LEG_BUDGET_S * 1e3 / max(timed(fn), 1e-3))))
    for i in range(reps):
        for k, fn in legs.items():
            if i < count[k]:
                times[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v), len(v)) for k, v in times.items()}


def fitted(n, F, T, n_fit=65536):
    """a model of T trees grown on the first min(n, n_fit) rows, and all n rows bound to its thresholds"""
    rng = np.random.default_rng(n + F + T)
    X = rng.standard_normal((n, F), dtype=f32)
    W = rng.standard_normal((F, D)).astype(f32)
    k = min(n, n_fit)
    Y = np.tanh(X[:k] @ W) + 0.3 * rng.standard_normal((k, D), dtype=f32)
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=BINS, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cpu", batch_size=k)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    ds_fit = m.prepare_dataset(X[:k])
    m.fit_prepared(ds_fit, Y, T)
    m.set_profiling(2)
    ds = ds_fit if k == n else m.prepare_dataset(X, reference=ds_fit)
    return m, ds


def shape(n, F, T, reps, with_shap):
    m, ds = fitted(n, F, T)
    e = m.get_ensemble_data()
    used = len(set(np.asarray(e["feature_indices"])[np.arange(DEPTH)[None, :] < np.asarray(e["depths"])[:, None]].tolist()))
    plan = gbrl_amd.gbrl_cpp.path_geometry(used, F, D)
    a = m.path_importance_prepared(ds)
    os.environ["GBRL_HIP_PATH_GENERIC"] = "1"
    b = m.path_importance_prepared(ds)
    os.environ.pop("GBRL_HIP_PATH_GENERIC")
    assert a["passes"] == plan["passes"] and b["passes"] == 0 and all(a[k].tobytes() == b[k].tobytes() for k in ("sum", "sum_abs", "expected")), "the two kernels differ"
    kernel = []
    base, norm, offset = K.poly_vectors(DEPTH)
    out = torch.from_numpy(np.tile(np.asarray(e["bias"], f32), (n, 1))).to(DEV)
    legs = {"path": lambda: (m.path_importance_prepared(ds), kernel.append(dict(m.last_phase_times()).get("path_rows", float("nan")))),
            "continue": lambda: m.predict_continue_prepared(ds, arg(out), 0, T)}
    if with_shap:
        legs["shap"] = lambda: m.shap_importance_prepared(ds, norm, base, offset)
    med = alternate(legs, reps)
    kernel = kernel[1:]                             # (the first entry is the warm-up's)
    fmt = lambda v: "%10.3f (%10.3f .. %10.3f, %2d runs)" % v
    p, c = med["path"], med["continue"]
    print("%-14s %5d trees   used %3d  slots %2d  passes %d   path_importance_prepared %s   kernel phase %10.3f (%10.3f .. %10.3f)   predict_continue_prepared %s   path / continue %6.1fx"
          % ("%d x %d" % (n, F), T, used, plan["slots"], plan["passes"], fmt(p), statistics.median(kernel), min(kernel), max(kernel), fmt(c), p[0] / c[0]), end="")
    if with_shap:
        print("   shap_importance_prepared %s   shap / path %7.1fx" % (fmt(med["shap"]), med["shap"][0] / p[0]), end="")
    print(flush=True)


def main():
    global LEG_BUDGET_S
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg-budget", type=float, default=LEG_BUDGET_S)
    ap.add_argument("--no-shap", action="store_true")
    ap.add_argument("--rows-log2", type=int, default=20)
    args = ap.parse_args()
    LEG_BUDGET_S = args.leg_budget
    print("== path_importance_prepared (D = %d, depth %d, %d bins, oblivious / L2; ms, median (min .. max) of up to %d alternating runs in one process; %s)"
          % (D, DEPTH, BINS, args.reps, torch.cuda.get_device_name(0)))
    for n, F, T in ((1 << args.rows_log2, 128, 10), (1 << args.rows_log2, 128, 100), (65536, 128, 1000), (4096, 16, 100)):
        shape(n, F, T, args.reps, not args.no_shap)


if __name__ == "__main__":
    main()
