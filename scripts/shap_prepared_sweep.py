"""Measurements of shap_prepared and shap_importance_prepared (profiles/shap_prepared.txt).

    python scripts/shap_prepared_sweep.py [--matrix] [--importance] [--reps 10] [--rows-log2 20] [--leg-budget 60] > profiles/shap_prepared.txt

  matrix form      shap_prepared(ds) against ensemble_shap(X) on the same rows, 65 536 x 128 with 100 trees and 4096 x 16 with 100 trees: the call
                   times (both deliver the matrix to the host), and beside them the kernel time of each form -- the `shap` phase of
                   last_phase_times() under set_profiling(2): k_shap alone, between two events, without the memset in front of it.
  importance form  shap_importance_prepared(ds) at 2^rows-log2 x 128 with 100 and with 10 trees against the only alternative there is without it: a
                   loop over ensemble_shap on slices of X of the default chunk size, each slice reduced on the host with gbrl_cpp.shap_sums_host's
                   rule restated in NumPy (tiles of 64 rows, float64) -- the loop needs X, which a user of fit_prepared no longer has.  Both legs
                   are first timed on one chunk of rows; when the row count asked for would not fit --leg-budget seconds a leg, the largest power
                   of two that does is measured instead, and the line says so.
D = 8, depth 6, 256 bins, oblivious / L2.  Medians of --reps with their spread (min .. max); the legs alternate inside one process; a leg whose runs
would pass the budget is repeated fewer times and the count is printed; before anything is timed the two forms are compared byte for byte.
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
cpp = gbrl_amd.gbrl_cpp


def model(F, batch_size):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=BINS, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device="cpu", batch_size=batch_size)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


LEG_BUDGET_S = 60.0                            # --leg-budget: a leg whose runs would take longer in all than this is repeated fewer times


def alternate(legs, reps):
    warm = sum(timed(fn) for fn in legs.values())          # warm-up, and what one round of the legs costs
    reps = max(1, min(reps, int(LEG_BUDGET_S * 1e3 / max(warm, 1e-3))))
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v), reps) for k, v in times.items()}


def fitted(n, F, T, n_fit=65536):
    """a model of T trees grown on the first min(n, n_fit) rows, and all n rows bound to its thresholds"""
    rng = np.random.default_rng(n + F + T)
    X = rng.standard_normal((n, F), dtype=f32)
    W = rng.standard_normal((F, D)).astype(f32)
    k = min(n, n_fit)
    Y = np.tanh(X[:k] @ W) + 0.3 * rng.standard_normal((k, D), dtype=f32)
    m = model(F, k)
    ds_fit = m.prepare_dataset(X[:k])
    m.fit_prepared(ds_fit, Y, T)
    m.set_profiling(2)
    ds = ds_fit if k == n else m.prepare_dataset(X, reference=ds_fit)
    base, norm, offset = K.poly_vectors(DEPTH)
    return m, ds, X, (norm, base, offset)


def phase(m, name):
    return dict(m.last_phase_times()).get(name, float("nan"))


def matrix_form(n, F, T, reps):
    m, ds, X, poly = fitted(n, F, T)
    a, b = np.asarray(m.shap_prepared(ds, *poly)), np.asarray(m.ensemble_shap(X, None, *poly))
    assert a.tobytes() == b.tobytes(), "the two forms differ"
    kf, kc = [], []
    legs = {"ensemble_shap": lambda: (m.ensemble_shap(X, None, *poly), kf.append(phase(m, "shap"))),
            "shap_prepared": lambda: (m.shap_prepared(ds, *poly), kc.append(phase(m, "shap")))}
    med = alternate(legs, reps)
    e, p = med["ensemble_shap"], med["shap_prepared"]
    kf, kc = kf[1:], kc[1:]                    # (the first entry is the warm-up's)
    spread = lambda v: "%10.3f (%10.3f .. %10.3f)" % (statistics.median(v), min(v), max(v))
    print("%-14s %4d trees   call: ensemble_shap %10.3f (%10.3f .. %10.3f)   shap_prepared %10.3f (%10.3f .. %10.3f)   %5.2fx   |   kernel: float form %s   codes form %s   %5.3fx   %d runs" % (
        "%d x %d" % (n, F), T, e[0], e[1], e[2], p[0], p[1], p[2], p[0] / e[0], spread(kf), spread(kc), statistics.median(kc) / statistics.median(kf), p[3]), flush=True)


def host_loop(m, X, poly, chunk):
    """mean |SHAP| without the data-set call: ensemble_shap on slices, reduced on the host by the tile rule"""
    F = X.shape[1]
    part, part_abs = [], []
    for p0 in range(0, X.shape[0], chunk):
        phi = np.asarray(m.ensemble_shap(X[p0:p0 + chunk], None, *poly)).astype(np.float64)
        tiles = phi.shape[0] // 64
        head = phi[:tiles * 64].reshape(tiles, 64, F, D)
        part.append(head.sum(axis=1)); part_abs.append(np.abs(head).sum(axis=1))
        if tiles * 64 < phi.shape[0]:
            part.append(phi[tiles * 64:].sum(axis=0, keepdims=True)); part_abs.append(np.abs(phi[tiles * 64:]).sum(axis=0, keepdims=True))
    return np.concatenate(part).sum(axis=0), np.concatenate(part_abs).sum(axis=0)


def importance_form(n, F, T, reps, loop_reps):
    chunk = cpp.shap_geometry(F, D)["default_chunk_rows"]
    asked = n
    if n > chunk:                              # one chunk of rows first: what the row count asked for would cost
        m, ds, X, poly = fitted(chunk, F, T)
        timed(lambda: m.shap_importance_prepared(ds, *poly))          # (warm-up)
        per_chunk = max(timed(lambda: m.shap_importance_prepared(ds, *poly)), timed(lambda: host_loop(m, X, poly, chunk)))
        while n > chunk and per_chunk * (n // chunk) * 3 > LEG_BUDGET_S * 1e3:      # (a checked run, a warm-up and at least one timed run)
            n //= 2
        del m, ds, X
    m, ds, X, poly = fitted(n, F, T)
    r1, r2 = m.shap_importance_prepared(ds, *poly), m.shap_importance_prepared(ds, *poly, chunk_rows=4 * chunk)
    assert r1["sum_abs"].tobytes() == r2["sum_abs"].tobytes() and r1["sum"].tobytes() == r2["sum"].tobytes(), "chunk_rows changes the bytes"
    got = []
    first = timed(lambda: got.append(host_loop(m, X, poly, chunk)))
    s, a = got[0]
    rel = float(np.abs(a - r1["sum_abs"]).max() / np.abs(r1["sum_abs"]).max())
    assert rel < 1e-9, rel                     # (NumPy adds pairwise inside a tile: the same number up to float64 rounding, not the same bytes)
    kernel = []
    call = alternate({"importance": lambda: (m.shap_importance_prepared(ds, *poly), kernel.append(phase(m, "shap")))}, reps)["importance"]
    if first > LEG_BUDGET_S * 1e3 / 2:         # too slow to repeat inside the budget: the checked run is the measurement
        loop = (first, first, first, 1)
    else:
        loop = alternate({"loop": lambda: host_loop(m, X, poly, chunk)}, loop_reps)["loop"]
    kern = kernel[1:]
    if n != asked:
        print("(%d rows would not fit %.0f s a leg at %.1f ms a chunk of %d rows: measured at %d rows)" % (asked, LEG_BUDGET_S, per_chunk, chunk, n))
    print("%-14s %4d trees   shap_importance_prepared %10.3f (%10.3f .. %10.3f, %d runs), device phase %10.3f (%10.3f .. %10.3f)   ensemble_shap loop + host sums %10.3f (%10.3f .. %10.3f, %d runs)   %5.2fx"
          % ("%d x %d" % (n, F), T, call[0], call[1], call[2], call[3], statistics.median(kern), min(kern), max(kern), loop[0], loop[1], loop[2], loop[3], loop[0] / call[0]), flush=True)


def main():
    global LEG_BUDGET_S
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="store_true")
    ap.add_argument("--importance", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-reps", type=int, default=10, help="runs of the host loop (the slow leg)")
    ap.add_argument("--rows-log2", type=int, default=20)
    ap.add_argument("--leg-budget", type=float, default=LEG_BUDGET_S, help="seconds one leg may take in all")
    ap.add_argument("--trees", type=int, nargs="*", default=[100, 10])
    a = ap.parse_args()
    LEG_BUDGET_S = a.leg_budget
    both = not (a.matrix or a.importance)
    print("== SHAP values on a prepared data set (D = %d, depth %d, %d bins, oblivious / L2; ms, median of %d (min .. max); legs alternate in one process) ==" % (D, DEPTH, BINS, a.reps))
    if a.matrix or both:
        print("-- matrix form: the call, matrix delivered to the host; ratio = shap_prepared / ensemble_shap")
        matrix_form(65536, 128, 100, a.reps)
        matrix_form(4096, 16, 100, a.reps)
    if a.importance or both:
        print("-- importance form: against a loop over ensemble_shap slices reduced on the host; ratio = loop / call")
        for T in a.trees:
            importance_form(1 << a.rows_log2, 128, T, a.reps, a.loop_reps)


if __name__ == "__main__":
    main()
