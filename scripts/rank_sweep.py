"""Measurements of the ranking objectives (profiles/rank.txt): rank_gradient alone, fit_prepared per iteration, what lambdarank buys, and -- with
--legs -- the legs this change must not move (run once per process by a driver that alternates this build and the parent's).

    python scripts/rank_sweep.py > profiles/rank.txt
    python scripts/rank_sweep.py --legs           # one process of the unchanged legs: prints one line of medians

Medians of 10; the legs of a table alternate inside one process; two runs of every leg are byte-equal before anything is timed."""
import argparse
import json
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


def arg(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


def model(F, D=1, depth=6, n_bins=256, batch_size=1 << 21, device="cuda"):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func="L2", generator_type="Quantile",
                      grow_policy="oblivious", device=device, batch_size=batch_size)
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
    """legs: {name: fn}; every repetition runs every leg once, in order; returns {name: median ms}"""
    for fn in legs.values():
        fn()                                   # warm-up
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def ranking_data(n_queries, size, F, seed, labels_max=4):
    rng = np.random.default_rng(seed)
    n = n_queries * size
    X = rng.standard_normal((n, F)).astype(f32)
    z = X[:, 0] + 0.5 * X[:, 1] + 0.5 * rng.standard_normal(n)
    y = np.clip(np.floor((z + 2.0) * (labels_max + 1) / 4.0), 0, labels_max).astype(np.int32)
    return X, y, np.full(n_queries, size, np.int32)


def kernel_cost():
    print("== rank_gradient alone (device tuples in, grad + hess + loss + ndcg + positions out; median of %d, ms) ==" % REPS)
    print("yardstick: objective_gradient(pred, y, 'logistic') at D = 1 on the same row count, same process, legs alternating")
    print("%-22s %-11s %9s %12s %14s   %s" % ("shape", "objective", "ms", "pairs", "pairs/s", "share of the call by phase (set_profiling(2), median of %d)" % REPS))
    m = model(4, device="cuda")
    for n_queries, size in ((1 << 19, 2), (8192, 128), (64, 1024)):
        n = n_queries * size
        rng = np.random.default_rng(size)
        s = torch.from_numpy((rng.standard_normal(n) * 2).astype(f32)).to(DEV)
        y = torch.from_numpy(rng.integers(0, 5 if size > 2 else 2, n).astype(np.int32)).to(DEV)
        yf = torch.from_numpy(rng.integers(0, 2, n).astype(f32)).to(DEV)
        group = np.full(n_queries, size, np.int32)
        legs, pairs = {}, {}
        for obj in ("pairwise", "lambdarank"):
            a = m.rank_gradient(arg(s), arg(y), group, obj)
            b = m.rank_gradient(arg(s), arg(y), group, obj)
            for k in ("grad", "hess", "positions"):
                assert torch.equal(torch.from_dlpack(a[k]), torch.from_dlpack(b[k])), (obj, k)
            assert a["ndcg"].tobytes() == b["ndcg"].tobytes() and np.float64(a["loss"]).tobytes() == np.float64(b["loss"]).tobytes()
            pairs[obj] = a["pairs"]
            legs[obj] = (lambda o: lambda: m.rank_gradient(arg(s), arg(y), group, o))(obj)
        legs["logistic"] = lambda: m.objective_gradient(arg(s), arg(yf), "logistic")
        med = alternate(legs)
        for obj in ("pairwise", "lambdarank"):
            m.set_profiling(2)
            ph = {}
            for _ in range(REPS):
                m.rank_gradient(arg(s), arg(y), group, obj)
                for k, v in m.last_phase_times().items():
                    ph.setdefault(k, []).append(v)
            m.set_profiling(0)
            ph = {k: statistics.median(v) for k, v in ph.items() if k.startswith("rank_")}
            tot = sum(ph.values())
            share = "  ".join("%s %.3f ms (%.0f%%)" % (k[5:], v, 100.0 * v / tot) for k, v in ph.items())
            print("%-22s %-11s %9.3f %12d %14.3e   %s" % ("%d x %d" % (n_queries, size), obj, med[obj], pairs[obj], pairs[obj] / (med[obj] * 1e-3), share))
        print("%-22s %-11s %9.3f" % ("%d x %d" % (n_queries, size), "logistic", med["logistic"]))
    print("(rank_queries is the label pass with its uploads and its wait, once per call; a fit pays it once, not per iteration)")


def fit_cost():
    print()
    print("== fit_prepared per iteration (F = 128, depth 6, 256 bins, oblivious / L2; %d iterations a run from a fresh model, median of %d runs, ms per iteration) ==" % (5, REPS))
    print("yardstick: the logistic fit at D = 1 on the same data set (targets y > 1)")
    T = 5
    for n_queries, size in ((1 << 19, 2), (8192, 128)):
        X, y, group = ranking_data(n_queries, size, 128, seed=size, labels_max=4 if size > 2 else 1)
        yl = (y > (1 if size > 2 else 0)).astype(f32)
        Xd = torch.from_numpy(X).to(DEV)
        yd, yld = torch.from_numpy(y).to(DEV), torch.from_numpy(yl).to(DEV)
        holder = model(128)
        ds = holder.prepare_dataset(arg(Xd))
        kinds = {}
        for obj in ("pairwise", "lambdarank", "logistic"):
            for leaf in ("gradient", "newton"):
                kw = dict(objective=obj, leaf_update=leaf)
                if obj != "logistic":
                    kw["group"] = group
                tar = yld if obj == "logistic" else yd
                files = []
                for _ in range(2):
                    mm = model(128)
                    mm.fit_prepared(ds, arg(tar), 2, **kw)
                    files.append(np.asarray(mm.get_ensemble_data()["values"]).tobytes())
                assert files[0] == files[1], (obj, leaf)
                kinds["%s/%s" % (obj, leaf)] = (lambda kw_, tar_: lambda: model(128).fit_prepared(ds, arg(tar_), T, **kw_))(kw, tar)
        med = alternate(kinds)
        for k, v in med.items():
            base = med["logistic/" + k.split("/")[1]]
            print("%-22s %-22s %9.3f ms / iteration   %.2fx the logistic fit" % ("%d x %d" % (n_queries, size), k, v / T, v / base))
        del ds, holder


def what_it_buys():
    print()
    print("== what it buys: validation NDCG@10 against trees (relevance 0..4 a noisy monotone function of two features; 2048 + 512 queries of 32 rows, F = 16,")
    print("   depth 4, lr 0.1): lambdarank (ndcg_at = 10) with newton leaves, and an rmse fit on the labels, the same trees counted ==")
    F = 16
    X, y, group = ranking_data(2048, 32, F, seed=1)
    Xv, yv, gv = ranking_data(512, 32, F, seed=2)
    stops = [1, 2, 5, 10, 20, 50, 100]
    rows = {}
    for name in ("lambdarank", "rmse"):
        m = model(F, depth=4, device="cpu")
        ds = m.prepare_dataset(X)
        dsv = m.prepare_dataset(Xv, reference=ds)
        out, done = [], 0
        for t in stops:
            if name == "lambdarank":
                m.fit_prepared(ds, y, t - done, objective="lambdarank", group=group, ndcg_at=10, leaf_update="newton")
            else:
                m.fit_prepared(ds, y.astype(f32), t - done)
            done = t
            base = np.full(len(yv), m.get_bias()[0], f32)
            P = np.asarray(m.predict_continue_prepared(dsv, base, 0, t))
            out.append(1.0 - m.rank_gradient(np.ascontiguousarray(P), yv, gv, "lambdarank", 10)["loss"])
        rows[name] = out
    base = 1.0 - model(F, device="cpu").rank_gradient(np.zeros(len(yv), f32), yv, gv, "lambdarank", 10)["loss"]
    print("trees       " + "".join("%9d" % t for t in stops) + "    (all scores equal: %.4f)" % base)
    for name, out in rows.items():
        print("%-12s" % name + "".join("%9.4f" % v for v in out))


def unchanged_legs():
    """one process: medians of the legs that exist in the parent commit too"""
    N, F = 1 << 20, 128
    rng = np.random.default_rng(0)
    X = torch.from_numpy(rng.standard_normal((N, F)).astype(f32)).to(DEV)
    y8 = torch.from_numpy(rng.standard_normal((N, 8)).astype(f32)).to(DEV)
    y1 = torch.from_numpy((rng.random(N) < 0.3).astype(f32)).to(DEV)
    h8, h1 = model(F, 8), model(F, 1)
    ds8, ds1 = h8.prepare_dataset(arg(X)), h1.prepare_dataset(arg(X))
    T = 5
    legs = {"fit_prepared_rmse_D8": lambda: model(F, 8).fit_prepared(ds8, arg(y8), T),
            "fit_prepared_logistic_newton_D1": lambda: model(F, 1).fit_prepared(ds1, arg(y1), T, objective="logistic", leaf_update="newton")}
    med = alternate(legs)
    print(json.dumps({k: round(v / T, 4) for k, v in med.items()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", action="store_true")
    a = ap.parse_args()
    if a.legs:
        unchanged_legs()
    else:
        print("rank_sweep.py on %s" % torch.cuda.get_device_name(0))
        kernel_cost()
        fit_cost()
        what_it_buys()
