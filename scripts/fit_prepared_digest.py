"""The bytes the calls on a prepared data set leave, for comparing two builds of the package line by line.

    python3 scripts/fit_prepared_digest.py ROOT [> FILE]     # ROOT: the root of a built tree (it holds gbrl_amd/ with its extension)

One process, one data set per (output_dim, grow policy): 2049 rows x 7 features, n_bins 16, max_depth 3, 6 iterations, batch_size 1024 (three
batches, the last of one row; a ranking objective takes batch_size = n), a 513-row validation set bound with reference=.  Every fit case runs
with set_profiling(0) and with set_profiling(2).  A line per result: the sha256 of the saved model file, every returned loss, curve entry, value,
sum and bits as hex, the names of last_phase_times() in order; a refusal is recorded with its message.  Nothing here is compared with anything:
run it on both builds, each in a process of its own, and compare the two outputs (cmp).  Inputs are NumPy arrays, so every staging path uploads.
"""
import ctypes
import hashlib
import os
import sys
import tempfile

import numpy as np

N, NV, F, BINS, DEPTH, ITERS, BATCH = 2049, 513, 7, 16, 3, 6, 1024
f32 = np.float32


def hexes(a):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return " ".join(float(x).hex() for x in a.ravel())
    return " ".join(str(int(x)) for x in a.ravel())


def main(root):
    sys.path.insert(0, os.path.abspath(root))
    import gbrl_amd
    cpp = gbrl_amd.gbrl_cpp
    unexpected = []
    rng = np.random.default_rng(20)
    X = rng.standard_normal((N, F)).astype(f32)
    XV = rng.standard_normal((NV, F)).astype(f32)

    def model(D, policy, batch=BATCH):
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=DEPTH, n_bins=BINS, split_score_func="L2", generator_type="Quantile",
                          grow_policy=policy, device="cpu", batch_size=batch)
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_weights(np.ones(F, f32))
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m

    def digest(m):
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "m.gbrl_model")
            assert m.save(p) == 0
            with open(p, "rb") as f:
                return hashlib.sha256(f.read()).hexdigest()

    def show(name, r):
        if isinstance(r, dict):
            for k in sorted(r):
                print("%s  %s: %s" % (name, k, r[k] if isinstance(r[k], str) else hexes(r[k])))
        elif isinstance(r, tuple):
            for i, x in enumerate(r):
                print("%s  [%d]: %s" % (name, i, "None" if x is None else hexes(x)))
        elif r is not None:
            print("%s  result: %s" % (name, hexes(r)))

    def call(name, fn, refusal=False):
        """one call: its results, or the refusal's message (unexpected outside the refusal cases: recorded, and the exit status says so)"""
        try:
            r = fn()
        except Exception as exc:   # noqa: BLE001 -- the message is the record
            print("%s  raised %s: %s" % (name, type(exc).__name__, exc))
            if not refusal:
                unexpected.append(name)
            return None
        if refusal:
            print("%s  NOT refused" % name)
            unexpected.append(name)
        show(name, r)
        return r

    # the C ABI itself, for the refusals the binding's own shape checks stand in front of (there m is the caller's)
    lib = ctypes.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = ctypes.c_char_p
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.gbrl_hip_predict_continue_prepared.argtypes = [P, P, P, I, I, P, I, I, I, P]
    lib.gbrl_hip_newton_leaves_prepared_weighted.argtypes = [P, P, P, I, I, P, I, P, I, I, I, ctypes.c_double, P, I, ctypes.c_float, P, P, P]
    lib.gbrl_hip_quantile_leaves_prepared.argtypes = [P, P, P, I, I, P, I, P, I, P, I, P, P, P]

    def c_refusal(name, status):
        print("%s  status %d: %s" % (name, status, lib.gbrl_hip_last_error().decode() if status else "NOT refused"))
        if status == 0:
            unexpected.append(name)

    def fit(name, D, policy, targets, batch=BATCH, twice=False, **kw):
        """the case with profiling off and with every phase timed, each on a fresh model and data set; returns the first model with its data sets"""
        kept = None
        for level in (0, 2):
            tag = "%s D=%d %s profiling=%d" % (name, D, policy, level)
            m = model(D, policy, batch)
            m.set_profiling(level)
            ds = m.prepare_dataset(X)
            if "valid" in kw:
                kw["valid"] = m.prepare_dataset(XV, reference=ds)
            for k in range(2 if twice else 1):
                call(tag + (" call %d" % k if twice else ""), lambda: m.fit_prepared(ds, targets, ITERS, **kw))
                print("%s  phases: %s" % (tag, " ".join(m.last_phase_times().keys())))
                print("%s  model: %s trees=%d" % (tag, digest(m), m.get_num_trees()))
            kept = kept or (m, ds)
        return kept

    w = rng.uniform(0.25, 4.0, N).astype(f32)
    wv = rng.uniform(0.25, 4.0, NV).astype(f32)
    group = np.array([40] * 51 + [9], np.int32)      # 2049 rows
    vgroup = np.array([27] * 19, np.int32)           # 513 rows
    rel = np.clip(np.floor(X[:, 0] + X[:, 1] + 2 + 0.5 * rng.standard_normal(N)), 0, 4).astype(np.int32)
    relv = np.clip(np.floor(XV[:, 0] + XV[:, 1] + 2 + 0.5 * rng.standard_normal(NV)), 0, 4).astype(np.int32)
    rows = rng.integers(0, N, 100).astype(np.int32)
    rows[50:60] = rows[0:10]                         # duplicates

    for D in (1, 3):
        P = rng.standard_normal((F, D)).astype(f32)
        y = (np.tanh(X @ P) + 0.3 * rng.standard_normal((N, D))).astype(f32)
        yv = (np.tanh(XV @ P) + 0.3 * rng.standard_normal((NV, D))).astype(f32)
        yb, ybv = (y > 0).astype(f32), (yv > 0).astype(f32)
        lab, labv = (np.argmax(X[:, :3], 1).astype(np.int32), np.argmax(XV[:, :3], 1).astype(np.int32))
        pred = (0.5 * rng.standard_normal((N, D))).astype(f32)
        for policy in ("oblivious", "greedy"):
            tag = "D=%d %s" % (D, policy)
            m_def, ds_def = fit("defaults", D, policy, y)
            if D == 3:
                fit("softmax", D, policy, lab, valid=True, valid_targets=labv, subsample=0.5, colsample=0.5, seed=3, objective="softmax", eval_metric="error")
            m_log, ds_log = fit("logistic_newton_goss", D, policy, yb, valid=True, valid_targets=ybv, objective="logistic", leaf_update="newton", weights=w,
                                valid_weights=wv, goss=(0.2, 0.3), seed=5)
            fit("logistic_auc", D, policy, yb, valid=True, valid_targets=ybv, objective="logistic", eval_metric="auc", early_stopping_rounds=2)
            m_q, ds_q = fit("quantile", D, policy, y, valid=True, valid_targets=yv, objective="quantile", leaf_update="quantile", alpha=0.3)
            fit("warm_start", D, policy, y, twice=True)
            if D == 1:
                m_rk, ds_rk = fit("lambdarank_newton", D, policy, rel, batch=N, valid=True, valid_targets=relv, objective="lambdarank", leaf_update="newton",
                                  group=group, valid_group=vgroup, ndcg_at=5)
                fit("pairwise", D, policy, rel, batch=N, objective="pairwise", group=group)
            # ---- single calls on the fitted models
            call(tag + " continue whole", lambda: m_def.predict_continue_prepared(ds_def, np.zeros((N, D), f32), 0, 0))
            call(tag + " continue rows", lambda: m_def.predict_continue_prepared(ds_def, np.zeros((100, D), f32), 2, 5, rows=rows))
            m_log.set_profiling(2)
            m_q.set_profiling(2)
            call(tag + " newton plain", lambda: m_log.newton_leaves_prepared(ds_log, pred, yb, "logistic"))
            call(tag + " newton rows weights", lambda: m_log.newton_leaves_prepared(ds_log, pred[rows], yb[rows], "logistic", leaf_l2=0.5, rows=rows, tree=2,
                                                                                     weights=w[rows], weight_max=4.0))
            print("%s newton  model: %s  phases: %s" % (tag, digest(m_log), " ".join(m_log.last_phase_times().keys())))
            call(tag + " quantile rows", lambda: m_q.quantile_leaves_prepared(ds_q, pred[rows], y[rows], 0.3, rows=rows, tree=1))
            print("%s quantile  model: %s  phases: %s" % (tag, digest(m_q), " ".join(m_q.last_phase_times().keys())))
            if D == 1:
                call(tag + " newton group", lambda: m_rk.newton_leaves_prepared(ds_rk, pred, rel, "lambdarank", group=group, ndcg_at=5))
                print("%s newton group  model: %s" % (tag, digest(m_rk)))
            for obj, t in (("rmse", y), ("logistic", yb)) + ((("softmax", lab),) if D == 3 else ()):
                call("%s objective_gradient %s weights" % (tag, obj), lambda: m_def.objective_gradient(pred, t, obj, weights=w))
            call(tag + " objective_gradient quantile alpha", lambda: m_def.objective_gradient(pred, y, "quantile", alpha=0.3))
            call(tag + " eval_metric error", lambda: m_def.eval_metric(pred, yb, "logistic", "error"))
            call(tag + " eval_metric auc", lambda: m_def.eval_metric(pred, yb, "logistic", "auc"))
            if D == 3:
                call(tag + " eval_metric softmax error", lambda: m_def.eval_metric(pred, lab, "softmax", "error"))
            # ---- refusals whose code has a home of its own
            empty = model(D, policy)
            ds_e = empty.prepare_dataset(X)
            call(tag + " refused continue length", lambda: m_def.predict_continue_prepared(ds_def, np.zeros((100, D), f32), 0, 0), True)
            call(tag + " refused newton length", lambda: m_log.newton_leaves_prepared(ds_log, pred[:100], yb[:100], "logistic"), True)
            call(tag + " refused quantile length", lambda: m_q.quantile_leaves_prepared(ds_q, pred[:100], y[:100], 0.3), True)
            short, out_short, levels = np.zeros((100, D), f32), np.zeros((100, D), f32), np.full(D, 0.3, f32)
            c_refusal(tag + " refused continue length (C ABI)", lib.gbrl_hip_predict_continue_prepared(
                m_def._handle(), ds_def._handle(), None, 0, 100, short.ctypes.data, 0, 0, 0, out_short.ctypes.data))
            c_refusal(tag + " refused newton length (C ABI)", lib.gbrl_hip_newton_leaves_prepared_weighted(
                m_log._handle(), ds_log._handle(), None, 0, 100, short.ctypes.data, 0, short.ctypes.data, 0, 1, -1, 1.0, None, 0, -1.0, None, None, None))
            c_refusal(tag + " refused quantile length (C ABI)", lib.gbrl_hip_quantile_leaves_prepared(
                m_q._handle(), ds_q._handle(), None, 0, 100, short.ctypes.data, 0, short.ctypes.data, 0, levels.ctypes.data, -1, None, None, None))
            call(tag + " refused step length", lambda: m_def.step_prepared(ds_def, pred[:100]), True)
            call(tag + " refused newton tree", lambda: m_log.newton_leaves_prepared(ds_log, pred, yb, "logistic", tree=99), True)
            call(tag + " refused quantile tree", lambda: m_q.quantile_leaves_prepared(ds_q, pred, y, 0.3, tree=-2), True)
            call(tag + " refused newton no trees", lambda: empty.newton_leaves_prepared(ds_e, pred, yb, "logistic"), True)
            call(tag + " refused quantile no trees", lambda: empty.quantile_leaves_prepared(ds_e, pred, y, 0.3), True)
            if D == 1:
                call(tag + " refused newton group tree", lambda: m_rk.newton_leaves_prepared(ds_rk, pred, rel, "lambdarank", group=group, tree=99), True)
                call(tag + " refused newton group no trees", lambda: empty.newton_leaves_prepared(ds_e, pred, rel, "lambdarank", group=group), True)
            call(tag + " refused weight_max", lambda: m_log.newton_leaves_prepared(ds_log, pred, yb, "logistic", weights=w, weight_max=1.0), True)
            bad_unit = yb.copy()
            bad_unit[7, 0] = 1.5
            call(tag + " refused newton target", lambda: m_log.newton_leaves_prepared(ds_log, pred, bad_unit, "logistic"), True)
            call(tag + " refused fit newton target", lambda: empty.fit_prepared(ds_e, bad_unit, 2, objective="logistic", leaf_update="newton"), True)
            bad_q = y.copy()
            bad_q[11, D - 1] = np.inf
            call(tag + " refused fit quantile target", lambda: empty.fit_prepared(ds_e, bad_q, 2, objective="quantile", alpha=0.5), True)
            if D == 3:
                bad_lab = lab.copy()
                bad_lab[13] = 3
                call(tag + " refused label host gradient", lambda: cpp.objective_gradient_host(pred, bad_lab, "softmax"), True)
                call(tag + " refused label host metric", lambda: cpp.eval_metric_host(pred, bad_lab, "softmax", "error"), True)
                call(tag + " refused label device gradient", lambda: m_def.objective_gradient(pred, bad_lab, "softmax"), True)
                call(tag + " refused label device metric", lambda: m_def.eval_metric(pred, bad_lab, "softmax", "error"), True)
                call(tag + " refused label fit", lambda: empty.fit_prepared(ds_e, bad_lab, 2, objective="softmax"), True)
            print("%s untouched  model: %s trees=%d" % (tag, digest(empty), empty.get_num_trees()), flush=True)
    if unexpected:
        print("UNEXPECTED: " + "; ".join(unexpected))
    return 1 if unexpected else 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
