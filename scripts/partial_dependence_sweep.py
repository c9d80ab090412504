"""Measurements of partial_dependence_prepared (profiles/partial_dependence.txt): the time per launched variant against ONE
predict_continue_prepared call over the same rows and trees in the same process -- a variant is that call's walk plus up to two 2-byte LDS writes
per row and D wave sums, minus the base read and (without ICE) the output store.  A permutation_importance_prepared launch at the same shape runs
beside it: a permutation variant gathers its code from another row, a partial-dependence variant does not.

    python scripts/partial_dependence_sweep.py > profiles/partial_dependence.txt

Medians of 10 with their spread (min .. max); the legs alternate inside one process; two runs of every partial-dependence leg are byte-equal before
anything is timed.  Targets and base live on the device; the ICE rows are delivered to the host (NumPy), and that copy is inside the ice legs."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gbrl_amd  # noqa: E402

f32 = np.float32
DEV = torch.device("cuda:0")
REPS = 10
D = 8


def arg(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def model(F, batch_size):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=6, n_bins=256, split_score_func="L2", generator_type="Quantile",
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


def alternate(legs, reps=REPS):
    """legs: {name: fn}; every repetition runs every leg once, in order; returns {name: (median, min, max) ms}"""
    for fn in legs.values():
        fn()                                   # warm-up
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def same(a, b, ice):
    ok = a["baseline"].tobytes() == b["baseline"].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a["pd"], b["pd"]))
    return ok and (not ice or all(x.tobytes() == y.tobytes() for x, y in zip(a["ice"], b["ice"])))


def shape(n, F, tree_counts, ice_legs):
    rng = np.random.default_rng(n + F)
    X = rng.standard_normal((n, F), dtype=f32)
    W = rng.standard_normal((F, D)).astype(f32)
    Y = np.tanh(X @ W) + 0.3 * rng.standard_normal((n, D), dtype=f32)
    m = model(F, n)
    ds = m.prepare_dataset(X)
    del X
    m.fit_prepared(ds, Y, max(tree_counts))
    y = torch.from_numpy(Y).to(DEV)
    base0 = torch.from_numpy(np.tile(np.asarray(m.get_ensemble_data()["bias"], f32), (n, 1))).to(DEV)
    thr = ds.thresholds()
    for T in tree_counts:
        breaks = sorted(((len(m.partial_dependence_codes(thr, c, T)), c) for c in range(F)), reverse=True)
        tested = [(k, c) for k, c in breaks if k > 1]
        (k1, c1) = tested[0]                                   # the column with the most breaks
        (ka, ca), (kb, cb) = tested[-1], tested[-2]            # the pair with the fewest cells among the tested columns
        legs, counts = {}, {}

        def leg(name, features, ice):
            fn = lambda: m.partial_dependence_prepared(ds, features, n_trees=T, ice=ice)
            a, b = fn(), fn()
            assert same(a, b, ice), name
            legs[name] = fn
            counts[name] = 1 + sum(int(np.prod(p.shape[:-1])) for p in a["pd"])      # the baseline and every cell: all tested, all launched

        leg("column", [c1], False)
        leg("pair", [(ca, cb)], False)
        if ice_legs:
            leg("column ice", [c1], True)
            leg("pair ice", [(ca, cb)], True)
        n_cols = min(len(tested), 9)
        n_rep = 63 // n_cols
        cols = sorted(c for _, c in tested[:n_cols])
        legs["perm"] = lambda: m.permutation_importance_prepared(ds, arg(y), n_repeats=n_rep, seed=1, cols=cols, n_trees=T)
        counts["perm"] = 1 + n_cols * n_rep
        out = base0.clone()
        legs["continue"] = lambda: m.predict_continue_prepared(ds, arg(out), 0, T)
        med = alternate(legs)
        c = med["continue"]
        print("%-14s %5d   %-12s %31s   predict_continue_prepared: %9.3f (%8.3f .. %8.3f) ms" % ("%d x %d" % (n, F), T, "", "", c[0], c[1], c[2]))
        for name in legs:
            if name == "continue":
                continue
            p, v = med[name], counts[name]
            what = {"column": "column %d, %d cells" % (c1, k1), "pair": "columns (%d, %d), %d x %d cells" % (ca, cb, ka, kb), "perm": "%d columns x %d repeats" % (n_cols, n_rep)}
            print("%-14s %5d   %-12s %4d var   %9.3f (%8.3f .. %8.3f)   %9.4f ms / var   %6.2fx   %s" % (
                "", T, name, v, p[0], p[1], p[2], p[0] / v, p[0] / v / c[0], what.get(name.split(" ")[0], "")))


def main():
    print("== partial_dependence_prepared, time per launched variant against one predict_continue_prepared call (D = %d, depth 6, 256 bins, oblivious / L2;" % D)
    print("   a variant = the baseline or a cell; base and targets on the device, ICE rows to the host; median of %d (min .. max), ms; ratio = ms / var over the call) ==" % REPS)
    shape(1 << 20, 128, (100,), ice_legs=False)
    shape(65536, 128, (1000, 100), ice_legs=True)


if __name__ == "__main__":
    main()
