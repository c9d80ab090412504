"""Measurements of shap_interaction_importance_prepared (profiles/shap_interactions.txt).

    python scripts/shap_interactions_sweep.py [--reps 10] [--leg-budget 40] > profiles/shap_interactions.txt

D = 1, depth 6, 256 bins: 65 536 x 128 with 15 oblivious trees, 65 536 x 128 with 10 greedy trees, 4096 x 16 with 200 oblivious trees.  Per shape, in ONE
process, legs alternating, medians of --reps runs with (min .. max):
  interactions   shap_interaction_importance_prepared(ds): the call, and its kernel phase `shapx_rows` (summed over the chunks) under set_profiling(2)
  shap           shap_importance_prepared(ds) on the same model and rows, and its kernel phase `shap`: the quadratic explainer beside the cubic one
  general        the interactions call under GBRL_HIP_SHAPX_GENERIC=1: the one-thread-per-row kernel, what a shape the plan declines pays
Before anything is timed the streaming kernel's matrix of the first 512 rows is compared byte for byte with the one-thread-per-row kernel's
(GBRL_HIP_SHAPX_GENERIC=1).  Also printed: K, the largest number of distinct features in a tree and on a path, and the rows a block owns."""
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
D, DEPTH, BINS = 1, 6, 256
LEG_BUDGET_S = 40.0


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


def fitted(n, F, T, policy):
    rng = np.random.default_rng(n + F + T)
    X = rng.standard_normal((n, F), dtype=f32)
    y = np.tanh(X @ rng.standard_normal(F).astype(f32)) + 0.3 * rng.standard_normal(n, dtype=f32)
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=BINS, split_score_func="L2" if policy == "oblivious" else "Cosine",
                      generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=n)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, f32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    ds = m.prepare_dataset(X)
    m.fit_prepared(ds, y, T)
    m.set_profiling(2)
    return m, ds


def phase(m, name):
    return m.last_phase_times().get(name, float("nan"))   # (the engine sums the phases of one name: here the chunks' launches)


def shape(n, F, T, policy, reps):
    m, ds = fitted(n, F, T, policy)
    e = m.get_ensemble_data()
    ti, dep, fi = np.asarray(e["tree_indices"]), np.asarray(e["depths"]), np.asarray(e["feature_indices"])
    per_path = max(len(set(fi[s, :dep[s]].tolist())) for s in range(len(dep)))
    rows_of = (lambda t: [t]) if policy == "oblivious" else (lambda t: range(ti[t], ti[t + 1] if t + 1 < len(ti) else len(dep)))
    per_tree = max(len({f for s in rows_of(t) for f in fi[s, :dep[s]].tolist()}) for t in range(len(ti)))
    some = np.arange(min(n, 512), dtype=np.int32)
    a = m.shap_interactions_prepared(ds, rows=some)
    os.environ["GBRL_HIP_SHAPX_GENERIC"] = "1"
    b = m.shap_interactions_prepared(ds, rows=some)
    os.environ.pop("GBRL_HIP_SHAPX_GENERIC")
    assert np.asarray(a["values"]).tobytes() == np.asarray(b["values"]).tobytes(), "the two kernels differ"
    used = len(a["features"])
    plan = gbrl_amd.gbrl_cpp.shap_interactions_geometry(used, per_tree, per_path, F, D)
    base, norm, offset = K.poly_vectors(DEPTH)
    kx, ks = [], []
    kg = []

    def general():
        os.environ["GBRL_HIP_SHAPX_GENERIC"] = "1"
        try:
            r = m.shap_interaction_importance_prepared(ds)
        finally:
            os.environ.pop("GBRL_HIP_SHAPX_GENERIC")
        assert r["block_rows"] == 0
        kg.append(phase(m, "shapx_rows"))

    def interactions():
        assert m.shap_interaction_importance_prepared(ds)["block_rows"] == plan["block_rows"] > 0
        kx.append(phase(m, "shapx_rows"))

    legs = {"interactions": interactions, "shap": lambda: (m.shap_importance_prepared(ds, norm, base, offset), ks.append(phase(m, "shap"))), "general": general}
    med = alternate(legs, reps)
    kx, ks, kg = kx[1:], ks[1:], kg[1:]             # (the first entry is the warm-up's)
    fmt = lambda v: "%10.3f (%10.3f .. %10.3f, %2d runs)" % v
    print("%-12s %4d %-9s trees   K %3d  per tree %2d  per path %d  block rows %2d   shap_interaction_importance_prepared %s   kernel phase %10.3f (%10.3f .. %10.3f)   "
          "shap_importance_prepared %s   kernel phase %10.3f (%10.3f .. %10.3f)   kernel ratio interactions / shap %7.2fx   "
          "one-thread-per-row kernel: call %s   kernel phase %10.3f (%10.3f .. %10.3f)"
          % ("%d x %d" % (n, F), T, policy, used, per_tree, per_path, plan["block_rows"], fmt(med["interactions"]), statistics.median(kx), min(kx), max(kx),
             fmt(med["shap"]), statistics.median(ks), min(ks), max(ks), statistics.median(kx) / statistics.median(ks),
             fmt(med["general"]), statistics.median(kg), min(kg), max(kg)), flush=True)


def main():
    global LEG_BUDGET_S
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg-budget", type=float, default=LEG_BUDGET_S)
    args = ap.parse_args()
    LEG_BUDGET_S = args.leg_budget
    print("== shap_interaction_importance_prepared (D = %d, depth %d, %d bins; ms, median (min .. max) of up to %d alternating runs in one process; %s)"
          % (D, DEPTH, BINS, args.reps, torch.cuda.get_device_name(0)))
    for n, F, T, policy in ((65536, 128, 15, "oblivious"), (65536, 128, 10, "greedy"), (4096, 16, 200, "oblivious")):
        shape(n, F, T, policy, args.reps)


if __name__ == "__main__":
    main()
