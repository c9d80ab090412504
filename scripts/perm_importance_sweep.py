"""Measurements of permutation_importance_prepared (profiles/perm_importance.txt): the time per (column, repeat) variant against ONE
predict_continue_prepared call over the same rows and trees in the same process -- a variant is that call's walk plus a 2-byte gather per row, minus
the base read and the output store.

    python scripts/perm_importance_sweep.py > profiles/perm_importance.txt

Medians of 10 with their spread (min .. max); the two legs alternate inside one process; two runs of every leg are byte-equal before anything is
timed.  Targets and base live on the device, so that no leg times an upload of theirs."""
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


def used_columns(m, n_trees):
    e = m.get_ensemble_data()
    depths, fidx = np.asarray(e["depths"])[:n_trees], np.asarray(e["feature_indices"])[:n_trees]
    live = np.arange(fidx.shape[1])[None, :] < depths[:, None]
    return sorted(set(int(f) for f in fidx[live]))


def shape(n, F, tree_counts):
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
    geo = gbrl_amd.gbrl_cpp.permutation_geometry()
    for T in tree_counts:
        used = used_columns(m, T)
        # one launch exactly: the baseline and launch_variants - 1 shuffled variants, all on columns the walk reads
        n_cols = min(len(used), 9)
        n_repeats = (geo["launch_variants"] - 1) // n_cols
        cols = used[:n_cols]
        variants = 1 + n_cols * n_repeats
        perm = lambda: m.permutation_importance_prepared(ds, arg(y), n_repeats=n_repeats, seed=1, cols=cols, n_trees=T)
        a, b = perm(), perm()
        assert a["loss"].tobytes() == b["loss"].tobytes() and np.float64(a["baseline"]).tobytes() == np.float64(b["baseline"]).tobytes()
        outs = []
        for _ in range(2):
            o = base0.clone()
            m.predict_continue_prepared(ds, arg(o), 0, T)
            outs.append(o)
        assert torch.equal(outs[0], outs[1])
        out = base0.clone()
        med = alternate({"perm": perm, "continue": lambda: m.predict_continue_prepared(ds, arg(out), 0, T)})
        p, c = med["perm"], med["continue"]
        print("%-14s %5d %4d x %-2d %4d   %9.3f (%8.3f .. %8.3f)   %9.4f   %9.3f (%8.3f .. %8.3f)   %6.2fx   %s" % (
            "%d x %d" % (n, F), T, n_cols, n_repeats, variants, p[0], p[1], p[2], p[0] / variants, c[0], c[1], c[2], p[0] / variants / c[0],
            "mean importance of the columns %s: %s" % (cols[:3], np.array2string(a["mean"][:3], precision=4))))


def main():
    print("== permutation_importance_prepared, time per variant against one predict_continue_prepared call (D = %d, depth 6, 256 bins, oblivious / L2, rmse;" % D)
    print("   one launch: the baseline + 63 shuffled variants on columns the trees use; targets and base on the device; median of %d (min .. max), ms) ==" % REPS)
    print("%-14s %5s %9s %4s   %31s   %9s   %31s   %7s" % ("rows x cols", "trees", "cols x rep", "var", "the call, ms", "ms / var", "predict_continue_prepared, ms", "ratio"))
    shape(1 << 20, 128, (100, 1))
    shape(65536, 128, (1000, 100, 1))
    shape(4096, 16, (100,))


if __name__ == "__main__":
    main()
