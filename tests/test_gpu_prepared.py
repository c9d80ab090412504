"""Prepared data sets on the GPU (GBRL.prepare_dataset / GBRL.step_prepared / PreparedDataset; include/gbrl_hip.h): a batch binned once and stepped
on many times.  Every comparison is exact (bytes):
  * the data set's thresholds and class codes against their NumPy restatement (the rank rule of the quantile candidates, A4:
    fmaf(b, step, min) of the uniform ones; codes = #{thresholds below the value}), at the edges of the fused preparation, the LDS sort, the
    one-launch growth and the radix selection;
  * the gather kernel alone: codes(rows) == codes()[:, rows, :];
  * step_prepared against step: ensemble arrays, metadata and the saved file after every tree of a boosting loop;
  * row subsets against a step on the gathered matrix, built so that the data set's thresholds ARE the subset's own (uniform: the subset holds
    every column's minimum and maximum; quantile: the data set is the subset tiled three times, so every rank falls on the same value);
  * phases, sharing between two models, lifetime, and the refusals that need a live data set.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -5
PREP_PHASES = ("transpose", "candidates", "binning")


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
def _model(F, D=1, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=32, parity="default", fw=None):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=n_bins, split_score_func=score, generator_type=gen,
                      grow_policy=policy, device="cpu", parity_mode=parity)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
    m.set_feature_weights(np.ones(F, np.float32) if fw is None else np.asarray(fw, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _data(n, F, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)     # Gaussian: neither -0.0 nor NaN
    assert not np.any((X == 0) & np.signbit(X))
    W = rng.standard_normal((F, D)).astype(np.float32)
    Y = (np.tanh(X @ W) + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    return X, Y


def _grads(m, X, Y):
    P = np.asarray(m.predict(X, None, 0, 0), np.float32).reshape(Y.shape)
    G = np.ascontiguousarray((P - Y).astype(np.float32))
    return G[:, 0].copy() if Y.shape[1] == 1 else G


def _state(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    e = m.get_ensemble_data()
    return {k: (np.asarray(v).tobytes() if hasattr(v, "shape") else v) for k, v in e.items()}, m.get_metadata(), p.read_bytes()


def _assert_same(a, b, tmp_path, what=""):
    ea, ma, fa = _state(a, tmp_path)
    eb, mb, fb = _state(b, tmp_path)
    assert ea.keys() == eb.keys()
    for k in ea:
        assert ea[k] == eb[k], "%s ensemble array %s differs" % (what, k)
    assert ma == mb, "%s metadata differs" % what
    assert fa == fb, "%s saved files differ" % what


def _fma32(a, b, c):
    """float32 fma(a, b, c): the exact value, rounded once (ties to even)."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    c0 = np.float32(float(exact))
    cands = [np.nextafter(c0, np.float32(-np.inf)), c0, np.nextafter(c0, np.float32(np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def _uniform_thresholds(X, B):
    """step = (max - min) / float(B); value_b = fmaf(float(b), step, min)."""
    out = np.empty((X.shape[1], B), np.float32)
    for f in range(X.shape[1]):
        lo, hi = np.float32(X[:, f].min()), np.float32(X[:, f].max())
        step = np.float32(np.float32(hi - lo) / np.float32(B))
        out[f] = [_fma32(np.float32(b), step, lo) for b in range(B)]
    return out


def _quantile_thresholds(X, B):
    """B + 1 equal-count buckets (the first N mod (B + 1) one row longer); threshold i = the value at rank cum_i - 1."""
    n = X.shape[0]
    per, rem = divmod(n, B + 1)
    cum = np.cumsum([per + (1 if i < rem else 0) for i in range(B)])
    return np.ascontiguousarray(np.sort(X, axis=0)[cum - 1, :].T)


def _codes_of(X, thr):
    """[G][n][16] u16: code of feature f and row r at [f // 16, r, f % 16] = #{k : thr[f, k] < X[r, f]}; padding slots are zero."""
    n, F = X.shape
    out = np.zeros(((F + 15) // 16, n, 16), np.uint16)
    for f in range(F):
        out[f // 16, :, f % 16] = (thr[f][None, :] < X[:, f][:, None]).sum(axis=1)
    return out


def _dev(t):
    return (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")


# ---- thresholds and codes against NumPy ---------------------------------------------------------------------------------------------------
N_EDGES = (1, 65, 384, 4096, 4097, 8193, 20000)     # fused preparation, LDS sort, one-launch growth, radix selection
F_EDGES = (1, 5, 16, 17, 33)                        # one group, a full group, one spilling slot, two spilling groups


@pytest.mark.parametrize("gen", ["Quantile", "Uniform"])
@pytest.mark.parametrize("n_bins", [32, 256])       # 256: k_bin_cols_fast
@pytest.mark.parametrize("n", N_EDGES)
def test_thresholds_and_codes_against_numpy(n, n_bins, gen):
    for F in F_EDGES:
        X, _ = _data(n, F, 1, seed=1000 + n + F)
        m = _model(F, gen=gen, n_bins=n_bins)
        ds = m.prepare_dataset(X)
        assert (ds.n_rows, ds.n_features, ds.n_bins, ds.generator_type) == (n, F, n_bins, gen)
        thr = ds.thresholds()
        want = _quantile_thresholds(X, n_bins) if gen == "Quantile" else _uniform_thresholds(X, n_bins)
        assert thr.dtype == np.float32 and thr.shape == (F, n_bins)
        assert thr.tobytes() == want.tobytes(), "thresholds differ (n=%d F=%d): first at %s" % (n, F, np.argwhere(thr != want)[:3].tolist())
        codes = ds.codes()
        G = (F + 15) // 16
        assert codes.dtype == np.uint16 and codes.shape == (G, n, 16)
        assert codes.tobytes() == _codes_of(X, thr).tobytes(), "codes differ (n=%d F=%d)" % (n, F)
        if F % 16:
            assert not codes[G - 1, :, F % 16:].any(), "padding slots must be zero, as step writes them"
        # at least what it names: thresholds (device + host), keys, codes
        assert ds.nbytes >= 3 * 4 * F * n_bins + 2 * G * n * 16
        assert m.get_num_trees() == 0 and m.get_iteration() == 0


# ---- the gather kernel alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 17, 33])
def test_gather_kernel(F):
    import torch
    n = 5000
    X, _ = _data(n, F, 1, seed=77 + F)
    ds = _model(F).prepare_dataset(X)
    full = ds.codes()
    rng = np.random.default_rng(5 + F)
    for m in (1, 63, 64, 65, 1000, 64 * 37 + 5):
        picks = {
            "sorted": np.sort(rng.choice(n, size=m, replace=False)),
            "shuffled": rng.choice(n, size=m, replace=False),
            "duplicates": rng.integers(0, max(1, m // 3), size=m),
            "all equal": np.full(m, n - 1),
        }
        for what, rows in picks.items():
            rows = np.ascontiguousarray(rows, np.int32)
            want = np.ascontiguousarray(full[:, rows, :]).tobytes()
            assert ds.codes(rows).tobytes() == want, (what, m, "host rows")
            assert ds.codes(rows=_dev(torch.from_numpy(rows).cuda())).tobytes() == want, (what, m, "device rows")
    ar = np.arange(n, dtype=np.int32)
    assert ds.codes(ar).tobytes() == full.tobytes()
    assert ds.codes(_dev(torch.from_numpy(ar).cuda())).tobytes() == full.tobytes()
    # an index outside [0, n) is found before anything reads through it, host or device vector; the next legal call works
    for bad in (-1, n):
        rows = np.array([0, 3, bad, 7], np.int32)
        with pytest.raises(RuntimeError, match="outside"):
            ds.codes(rows)
        with pytest.raises(RuntimeError, match="outside"):
            ds.codes(_dev(torch.from_numpy(rows).cuda()))
        ok = np.array([0, 3, n - 1, 7], np.int32)
        assert ds.codes(ok).tobytes() == np.ascontiguousarray(full[:, ok, :]).tobytes()
    with pytest.raises(RuntimeError):
        ds.codes(np.zeros(0, np.int32))


# ---- step_prepared against step, rows=None -----------------------------------------------------------------------------------------------
def _cases():
    combos = [(p, s, g) for p in ("oblivious", "greedy") for s in ("L2", "Cosine") for g in ("Quantile", "Uniform")]
    ns, Ds, depths, Fs = (384, 4097, 8193, 20000), (1, 3, 8, 17), (1, 4, 6), (5, 16, 17, 33)
    out = []
    for k in range(32):                                  # every combo at every n; D, depth, F and n_bins rotate through their values
        p, s, g = combos[k % 8]
        out.append(dict(policy=p, score=s, gen=g, n=ns[(k // 8 + k) % 4], D=Ds[(k // 2 + k // 8) % 4], depth=depths[k % 3], F=Fs[(k // 4) % 4],
                        n_bins=256 if k % 4 == 0 else 64))
    for k, parity in enumerate(("exact_argmax", "reference")):
        for j in range(3):
            p, s, g = combos[(3 * k + 2 * j + 1) % 8]
            out.append(dict(policy=p, score=s, gen=g, n=ns[(j + k) % 4], D=Ds[(j + 2 * k) % 4], depth=depths[(j + 1) % 3], F=7, n_bins=64, parity=parity))
    out.append(dict(policy="greedy", score="Cosine", gen="Quantile", n=70001, D=3, depth=4, F=6, n_bins=64))        # above the near-tie limit
    out.append(dict(policy="oblivious", score="L2", gen="Quantile", n=4097, D=3, depth=4, F=5, n_bins=64, fw=[1.0, 0.5, 2.0, 1.0, 0.25]))
    out.append(dict(policy="greedy", score="L2", gen="Uniform", n=8193, D=8, depth=4, F=5, n_bins=64, fw=[0.25, 1.0, 3.0, 0.5, 1.0]))
    out.append(dict(policy="oblivious", score="Cosine", gen="Quantile", n=8193, D=3, depth=4, F=9, n_bins=64, device_grads=True))
    out.append(dict(policy="greedy", score="L2", gen="Quantile", n=384, D=1, depth=4, F=9, n_bins=64, device_grads=True))
    return out


def _case_id(c):
    return "-".join(str(c[k]) for k in ("policy", "score", "gen", "n", "D", "depth", "F", "n_bins")) + ("-" + c["parity"] if "parity" in c else "") + \
        ("-fw" if "fw" in c else "") + ("-devgrads" if c.get("device_grads") else "")


@pytest.mark.parametrize("c", _cases(), ids=_case_id)
def test_step_prepared_equals_step(c, tmp_path):
    kw = dict(D=c["D"], policy=c["policy"], score=c["score"], gen=c["gen"], depth=c["depth"], n_bins=c["n_bins"], parity=c.get("parity", "default"),
              fw=c.get("fw"))
    X, Y = _data(c["n"], c["F"], c["D"], seed=sum(map(ord, _case_id(c))))
    a, b = _model(c["F"], **kw), _model(c["F"], **kw)
    ds = b.prepare_dataset(X)
    _assert_same(a, b, tmp_path, "after prepare_dataset:")           # preparing changes nothing
    for t in range(5):
        G = _grads(a, X, Y)
        a.step(X, None, G)
        if c.get("device_grads"):
            import torch
            Gd = torch.from_numpy(G).cuda()
            b.step_prepared(ds, _dev(Gd))
        else:
            b.step_prepared(ds, G)
        _assert_same(a, b, tmp_path, "tree %d:" % t)
    assert a.get_num_trees() == 5


# ---- phases ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [384, 20000])
def test_phases(n):
    """Phases other than the histogram build are recorded from profiling level 2 on (level 1 samples the key kernel only): that is where step()
    reports transpose / candidates / binning, so that is where their absence after step_prepared says something."""
    X, Y = _data(n, 6, 2, seed=3)
    m = _model(6, D=2)
    m.set_profiling(2)
    ds = m.prepare_dataset(X)
    assert all(p in m.last_phase_times() for p in PREP_PHASES)      # the preparation is where the work went
    m.step_prepared(ds, _grads(m, X, Y))
    ph = m.last_phase_times()
    assert not any(p in ph for p in PREP_PHASES), ph
    assert "grad_stats" in ph
    m.step(X, None, _grads(m, X, Y))
    ph = m.last_phase_times()
    assert all(p in ph for p in PREP_PHASES), ph
    m.step_prepared(ds, np.ascontiguousarray(_grads(m, X, Y)[::2]), rows=np.arange(0, n, 2, dtype=np.int32))
    ph = m.last_phase_times()
    assert not any(p in ph for p in PREP_PHASES) and "gather_codes" in ph, ph
    m.set_profiling(1)
    m.step_prepared(ds, _grads(m, X, Y))
    assert not any(p in m.last_phase_times() for p in PREP_PHASES)


# ---- one data set, two models -----------------------------------------------------------------------------------------------------------------
def test_actor_and_critic_share_one_data_set(tmp_path):
    n, F = 4097, 10
    X, Ya = _data(n, F, 4, seed=11)
    _, Yc = _data(n, F, 1, seed=12)
    mk_actor = lambda: _model(F, D=4, policy="greedy", score="Cosine", n_bins=64)
    mk_critic = lambda: _model(F, D=1, policy="oblivious", score="L2", n_bins=64)
    actor, critic, actor_twin, critic_twin = mk_actor(), mk_critic(), mk_actor(), mk_critic()
    ds = critic.prepare_dataset(X)                                      # made by one, served to both
    for t in range(3):
        Ga, Gc = _grads(actor_twin, X, Ya), _grads(critic_twin, X, Yc)
        actor.step_prepared(ds, Ga)
        critic.step_prepared(ds, Gc)
        actor_twin.step(X, None, Ga)
        critic_twin.step(X, None, Gc)
        _assert_same(actor, actor_twin, tmp_path, "actor, tree %d:" % t)
        _assert_same(critic, critic_twin, tmp_path, "critic, tree %d:" % t)


# ---- subsets ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,score", [("oblivious", "L2"), ("greedy", "Cosine")])
@pytest.mark.parametrize("m_rows", [3000, 5000, 9000])          # both sides of 4096 and of 8192
def test_subset_uniform(m_rows, policy, score, tmp_path):
    import torch
    n, F, D = 12000, 17, 3
    X, Y = _data(n, F, D, seed=21 + m_rows)
    rng = np.random.default_rng(m_rows)
    ext = np.concatenate([X.argmin(axis=0), X.argmax(axis=0)])
    idx = np.concatenate([ext, rng.integers(0, n, size=m_rows - ext.size)])
    rng.shuffle(idx)
    idx = np.ascontiguousarray(idx, np.int32)
    assert np.unique(idx).size < idx.size                                # duplicates
    Xs = np.ascontiguousarray(X[idx])
    assert Xs.min(axis=0).tobytes() == X.min(axis=0).tobytes() and Xs.max(axis=0).tobytes() == X.max(axis=0).tobytes()
    Ys = np.ascontiguousarray(Y[idx])
    kw = dict(D=D, policy=policy, score=score, gen="Uniform", depth=5, n_bins=64)
    a, b, c = _model(F, **kw), _model(F, **kw), _model(F, **kw)
    ds = b.prepare_dataset(X)
    idx_dev = torch.from_numpy(idx).cuda()
    for t in range(3):
        G = _grads(a, Xs, Ys)
        a.step(Xs, None, G)
        b.step_prepared(ds, G, rows=idx)
        c.step_prepared(ds, G, rows=_dev(idx_dev))
        _assert_same(a, b, tmp_path, "host rows, tree %d:" % t)
        _assert_same(a, c, tmp_path, "device rows, tree %d:" % t)


@pytest.mark.parametrize("policy", ["oblivious", "greedy"])
@pytest.mark.parametrize("score", ["L2", "Cosine"])
@pytest.mark.parametrize("m_rows", [330, 8580])                 # multiples of n_bins + 1
def test_subset_quantile(m_rows, score, policy, tmp_path):
    n_bins, F, D = 32, 6, 2
    assert m_rows % (n_bins + 1) == 0
    Xs, Ys = _data(m_rows, F, D, seed=31 + m_rows)
    X = np.ascontiguousarray(np.tile(Xs, (3, 1)))
    rows = np.ascontiguousarray(np.arange(m_rows) + m_rows * (np.arange(m_rows) % 3), np.int32)
    assert X[rows].tobytes() == Xs.tobytes()
    kw = dict(D=D, policy=policy, score=score, gen="Quantile", depth=4, n_bins=n_bins)
    a, b = _model(F, **kw), _model(F, **kw)
    ds = b.prepare_dataset(X)
    # every threshold rank of the tiled matrix falls on the value of the subset's own rank
    assert ds.thresholds().tobytes() == a.prepare_dataset(Xs).thresholds().tobytes()
    for t in range(3):
        G = _grads(a, Xs, Ys)
        a.step(Xs, None, G)
        b.step_prepared(ds, G, rows=rows)
        _assert_same(a, b, tmp_path, "tree %d:" % t)


@pytest.mark.parametrize("n", [384, 8193])
@pytest.mark.parametrize("gen", ["Quantile", "Uniform"])
def test_rows_arange_equals_rows_none(n, gen, tmp_path):
    F, D = 17, 3
    X, Y = _data(n, F, D, seed=41 + n)
    kw = dict(D=D, policy="greedy", score="Cosine", gen=gen, depth=4, n_bins=64)
    a, b = _model(F, **kw), _model(F, **kw)
    ds = a.prepare_dataset(X)
    ar = np.arange(n, dtype=np.int32)
    for t in range(3):
        G = _grads(a, X, Y)
        a.step_prepared(ds, G)
        b.step_prepared(ds, G, rows=ar)
        _assert_same(a, b, tmp_path, "tree %d:" % t)


# ---- lifetime -----------------------------------------------------------------------------------------------------------------------------------
def test_obs_is_not_needed_after_prepare_and_a_data_set_outlives_its_model(tmp_path):
    import torch
    n, F, D = 8193, 9, 2
    X, Y = _data(n, F, D, seed=51)
    kw = dict(D=D, policy="oblivious", score="L2", gen="Quantile", depth=4, n_bins=64)
    twin = _model(F, **kw)
    maker = _model(F, **kw)
    Xh = X.copy()
    ds_host = maker.prepare_dataset(Xh)
    Xh[:] = np.nan                                                       # the caller's matrix is gone
    Xd = torch.from_numpy(X).cuda()
    ds_dev = maker.prepare_dataset(_dev(Xd))
    Xd.fill_(float("nan"))
    torch.cuda.synchronize()
    clone = gbrl_amd.GBRL(maker)
    del maker                                                            # ... and so is the model that made the data sets
    other = _model(F, **kw)
    for t in range(3):
        G = _grads(twin, X, Y)
        twin.step(X, None, G)
        clone.step_prepared(ds_host, G)
        other.step_prepared(ds_dev, G)
        _assert_same(twin, clone, tmp_path, "host obs, tree %d:" % t)
        _assert_same(twin, other, tmp_path, "device obs, tree %d:" % t)


# ---- the refusals that need a live data set -------------------------------------------------------------------------------------------------
def test_refusals_with_a_live_data_set(tmp_path):
    import torch
    n, F, D = 500, 6, 2
    X, Y = _data(n, F, D, seed=61)
    m = _model(F, D=D)
    ds = m.prepare_dataset(X)
    G = _grads(m, X, Y)
    m.step_prepared(ds, G)
    before = _state(m, tmp_path)
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_step_prepared.argtypes = [vp, vp, vp, ci, vp, ci, ci]
    lib.gbrl_hip_dataset_destroy.argtypes = [vp]
    lib.gbrl_hip_dataset_destroy.restype = None
    lib.gbrl_hip_dataset_create.argtypes = [vp, vp, ci, ci, ci]
    lib.gbrl_hip_dataset_create.restype = vp

    def c_step(model, grads=G, rows=None, count=n, handle=None):
        return lib.gbrl_hip_step_prepared(model._handle(), ds._handle() if handle is None else handle, None if grads is None else grads.ctypes.data, 0,
                                          None if rows is None else rows.ctypes.data, 0, count)

    # another n_bins, generator or width: invalid argument
    for other, what in ((_model(F, D=D, n_bins=64), "n_bins"), (_model(F, D=D, gen="Uniform"), "generator_type"), (_model(F + 1, D=D), "number of features")):
        with pytest.raises(RuntimeError, match=what):
            other.step_prepared(ds, G)
        assert c_step(other) == E_INVALID and what.encode() in lib.gbrl_hip_last_error()
        assert other.get_num_trees() == 0
    # grads missing or misshapen for n or m; m == 0
    rows = np.arange(100, dtype=np.int32)
    with pytest.raises(RuntimeError, match="grads"):
        m.step_prepared(ds, None)
    with pytest.raises(RuntimeError, match="rows"):
        m.step_prepared(ds, G[:100])                                     # 100 gradient rows, no rows vector, 500 rows in the data set
    with pytest.raises(RuntimeError, match="Number of rows"):
        m.step_prepared(ds, G, rows=rows)
    with pytest.raises(RuntimeError, match="output dim"):
        m.step_prepared(ds, np.zeros((n, D + 1), np.float32))
    with pytest.raises(RuntimeError):
        m.step_prepared(ds, np.zeros((0, D), np.float32), rows=np.zeros(0, np.int32))
    assert c_step(m, grads=None) == E_INVALID
    assert c_step(m, count=100) == E_INVALID
    assert c_step(m, rows=rows, count=0) == E_INVALID
    assert c_step(m, count=0) == E_INVALID
    # rows outside [0, n): host and device vectors; no tree is grown, and the next legal call works
    for bad in (-1, n):
        r = np.array([1, 2, bad, 4], np.int32)
        g4 = np.ascontiguousarray(G[:4])
        with pytest.raises(RuntimeError, match="outside"):
            m.step_prepared(ds, g4, rows=r)
        with pytest.raises(RuntimeError, match="outside"):
            m.step_prepared(ds, g4, rows=_dev(torch.from_numpy(r).cuda()))
        assert c_step(m, grads=g4, rows=r, count=4) == E_INVALID
    assert _state(m, tmp_path) == before
    # a destroyed data set (the C ABI owns this one)
    h = lib.gbrl_hip_dataset_create(m._handle(), X.ctypes.data, 0, n, F)
    assert h is not None
    assert c_step(m, handle=h) == 0
    lib.gbrl_hip_dataset_destroy(h)
    assert c_step(m, handle=h) == E_INVALID and b"destroyed" in lib.gbrl_hip_last_error()
    lib.gbrl_hip_dataset_destroy(h)                                      # twice: ignored
    assert m.get_num_trees() == 2
    # a fresh model that was refused has latched nothing: it can still step on another width
    fresh = _model(F, D=D)
    with pytest.raises(RuntimeError):
        fresh.step_prepared(ds, G[:100])
    fresh.step_prepared(ds, G)
    assert fresh.get_num_trees() == 1
