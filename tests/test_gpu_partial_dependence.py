"""Partial dependence and ICE curves on a prepared data set, on the GPU (GBRL.partial_dependence_prepared; include/gbrl_hip.h, "Partial dependence").

The oracle is built from calls that existed before it.  For a cell that holds column c at code g the observations are materialised on the host,
    Xc = X.copy(); Xc[:, c] = thr[c][g] (g < B) or +inf (g == B); dsc = m.prepare_dataset(Xc, reference=ds_train)
(code = #{thresholds below x}: with strictly increasing thresholds thr[c][g] has code g and +inf has code B -- asserted from dsc.codes() for every
oracle), and the expected rows are P = predict_continue_prepared(dsc, tile(bias), 0, stop).

  1. an ICE block equals P bit for bit;
  2. |pd * m - math.fsum(P[:, d])| <= m * 2**-52 * sum|P[:, d]|: the reordering bound of a float64 sum of m terms (m * 2**-53 relative to sum|x|) plus
     the division and the multiplication back (2**-53 each), doubled for safety -- derived, not measured;
  3. byte equality across two calls, ice=True against ice=False, GBRL_HIP_PD_GENERIC=1 against the streaming kernel, rows=None against arange(n);
  4. an untested column has codes == [0] and pd[0] == the baseline's bytes; the baseline passes 2. against predict_continue_prepared(ds, tile(bias));
  5. the model's file bytes and ds.codes() are unchanged;
  6. the refusals.

Shapes: m in {1, 63, 64, 65, 257, 4097} (tile edges, and enough partials for the finishing sum to matter) on a model grown on 512 other rows with the
same thresholds and n_bins = 32; F in {1, 16, 17, 40} with columns 0, 15, 16 and F - 1 (both sides of the 32-byte record boundary) and the pairs
(0, 15) (one record), (15, 16) and (0, F - 1) (two records); D in {1, 3, 8} streaming, 65 and 128 general; oblivious depth 3 and greedy depth 4; T in
{1, 7, 40} with one n_trees prefix; a Linear schedule; two optimizers over disjoint outputs; rows= with duplicates at m = 1 and 65; a pair with more
cells than a launch takes (partial_dependence_geometry()); max_cells.  The data recipe is tests/test_gpu_perm_importance.py's: the targets lean on the
tested columns, so that the trees use them -- at least half of the tested columns must be used, and every tested column's thresholds must be strictly
increasing (both asserted: conditions on the inputs, not tolerances).
"""
import math
import os

import numpy as np
import pytest

import gbrl_amd

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp

N_TRAIN, N_BINS = 512, 32


def _model(F, D, policy, lr=0.1, n_bins=N_BINS, opts=None):
    m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=3 if policy == "oblivious" else 4, n_bins=n_bins,
                      split_score_func="L2" if policy == "oblivious" else "Cosine", generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=N_TRAIN)
    for o in opts or [dict(algo="SGD", scheduler="Const", init_lr=lr, start_idx=0, stop_idx=D)]:
        m.set_optimizer(**o)
    m.set_feature_weights(np.ones(F, np.float32))
    m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
    return m


def _tested(F):
    return sorted({c for c in (0, 15, 16, F - 1) if 0 <= c < F})


def _pairs(F):
    return list(dict.fromkeys(p for p in ((0, 15), (15, 16), (0, F - 1)) if p[0] != p[1] and max(p) < F))


def _data(rows, F, D, rng, W):
    X = rng.standard_normal((rows, F)).astype(np.float32)
    Y = (X @ W + 0.2 * rng.standard_normal((rows, D))).astype(np.float32)
    return X, (np.ascontiguousarray(Y[:, 0]) if D == 1 else np.ascontiguousarray(Y))


class Case:
    """A model grown by fit_prepared on N_TRAIN rows, and n other rows under the same thresholds to draw the curves on."""

    def __init__(self, n, F, D, policy, T, flat=False, lr=0.1, opts=None):
        self.n, self.F, self.D, self.T = n, F, D, T
        rng = np.random.default_rng(1000 * n + 10 * F + D + T)
        w = np.full(F, 1.0 if flat else 0.4)
        if not flat:
            for c, s in zip(_tested(F), (3.0, 2.5, 2.0, 1.5)):
                w[c] = s
        W = w[:, None] * rng.choice([-1.0, 1.0], size=(F, D))
        self.m = _model(F, D, policy, lr, opts=opts)
        self.Xt, self.yt = _data(N_TRAIN, F, D, rng, W)
        self.X, _ = _data(n, F, D, rng, W)
        self.ds_train = self.m.prepare_dataset(self.Xt)
        self.m.fit_prepared(self.ds_train, self.yt, T)
        assert self.m.get_num_trees() == T
        self.ds = self.m.prepare_dataset(self.X, reference=self.ds_train)
        self.thr = np.asarray(self.ds_train.thresholds())
        self.B = self.thr.shape[1]
        assert self.thr.shape == (F, N_BINS)
        for c in _tested(F):
            assert (np.diff(self.thr[c]) > 0).all(), (c, self.thr[c])          # a condition on the inputs: thr[c][g] then has code g
        self.bias = np.asarray(self.m.get_bias(), np.float32).reshape(1, D)
        self._seen = {}

    def used(self, n_trees=None):
        """the columns the walk of the trees [0, n_trees) tests (greedy: through the trees a trailing run of one-leaf trees runs on into)"""
        e = self.m.get_ensemble_data()
        depths, fidx, ti = np.asarray(e["depths"]), np.asarray(e["feature_indices"]), np.asarray(e["tree_indices"])
        L = np.asarray(e["values"]).shape[0]
        k, first = self.T if n_trees is None else n_trees, np.append(ti, L)
        if self.m.get_metadata()["grow_policy"] == "Oblivious":
            rows = k
        else:
            while k < self.T and first[k] - first[k - 1] == 1:
                k += 1
            rows = int(first[k])
        live = np.arange(fidx.shape[1])[None, :] < depths[:rows, None]
        return set(int(f) for f in fidx[:rows][live])

    def oracle(self, cell=(), stop=None):
        """P [n, D] for the cell ((column, code), ...): computed once, shared, never written"""
        key = (tuple(cell), stop)
        if key not in self._seen:
            Xc = self.X.copy()
            for c, g in cell:
                Xc[:, c] = self.thr[c][g] if g < self.B else np.inf
            dsc = self.m.prepare_dataset(Xc, reference=self.ds_train)
            codes = dsc.codes()
            for c, g in cell:
                assert (codes[c >> 4, :, c & 15] == g).all(), (c, g)
            P = self.m.predict_continue_prepared(dsc, np.tile(self.bias, (self.n, 1)), 0, self.T if stop is None else stop)
            P = np.asarray(P, np.float32).reshape(self.n, self.D)
            P.setflags(write=False)
            self._seen[key] = P
        return self._seen[key]

    def run(self, features, **kw):
        return self.m.partial_dependence_prepared(self.ds, features, **kw)


def _file(m, tmp_path):
    p = tmp_path / "state.gbrl_model"
    assert m.save(str(p)) == 0
    return p.read_bytes()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_result(a, b, ice):
    ok = a["features"] == b["features"] and a["rows"] == b["rows"] and _same(a["baseline"], b["baseline"])
    for i in range(len(a["features"])):
        pair = isinstance(a["features"][i], tuple)
        for key in ("codes", "values"):
            ok = ok and (all(_same(x, y) for x, y in zip(a[key][i], b[key][i])) if pair else _same(a[key][i], b[key][i]))
        ok = ok and _same(a["pd"][i], b["pd"][i])
        if ice:
            ok = ok and _same(a["ice"][i], b["ice"][i])
    return ok


def _env(name, value):
    class _E:
        def __enter__(self):
            os.environ[name] = value
        def __exit__(self, *a):
            os.environ.pop(name, None)
    return _E()


def _check_mean(pd, P, what):
    """check 2: pd [D] against the exactly rounded sums of P [m, D]"""
    m = P.shape[0]
    for d in range(P.shape[1]):
        col = P[:, d].astype(np.float64)
        err, bound = abs(pd[d] * m - math.fsum(col)), m * 2.0 ** -52 * float(np.abs(col).sum())
        print("%s  d %d  |pd * m - fsum| %.3g  bound %.3g" % (what, d, err, bound))
        assert err <= bound, (what, d, err, bound)


def _check_entry(k, r, i, cells, stop=None, rows=None):
    """checks 1 and 2 for the listed cells (index tuples) of entry i"""
    f = r["features"][i]
    cols = f if isinstance(f, tuple) else (f,)
    codes = r["codes"][i] if isinstance(f, tuple) else (r["codes"][i],)
    for idx in cells:
        cell = tuple((c, int(codes[a][j])) for a, (c, j) in enumerate(zip(cols, idx)))
        P = k.oracle(cell, stop)
        if rows is not None:
            P = P[rows]
        assert _same(r["ice"][i][idx], P), (f, idx)
        _check_mean(r["pd"][i][idx], P, "%s cell %s" % (f, idx))


def _sample(shape):
    """first, last and a middle cell of an entry; for a pair also the two other corners"""
    last = tuple(s - 1 for s in shape)
    cells = {tuple(0 for _ in shape), last, tuple(s // 2 for s in shape)}
    if len(shape) == 2:
        cells |= {(0, last[1]), (last[0], 0)}
    return sorted(cells)


CASES = [
    # n, F, D, policy, T
    (1, 1, 1, "oblivious", 1),
    (63, 16, 3, "greedy", 7),
    (64, 17, 8, "oblivious", 40),
    (65, 40, 3, "greedy", 40),
    (257, 17, 1, "oblivious", 7),
    (4097, 40, 8, "greedy", 7),
]


@pytest.mark.parametrize("n,F,D,policy,T", CASES)
def test_cells_equal_the_oracle(n, F, D, policy, T, tmp_path):
    k = Case(n, F, D, policy, T)
    m, tested, B = k.m, _tested(F), k.B
    used = k.used()
    assert 2 * len([c for c in tested if c in used]) >= len(tested), (tested, sorted(used))
    file0, codes0 = _file(m, tmp_path), k.ds.codes().tobytes()
    features = list(tested) + _pairs(F)
    r = k.run(features, ice=True)
    assert sorted(r) == ["baseline", "codes", "features", "ice", "pd", "rows", "values"]
    assert r["features"] == features and r["rows"] == n and r["baseline"].dtype == np.float64 and r["baseline"].shape == (D,)
    # ---- the baseline: no column held
    base = k.oracle()
    _check_mean(r["baseline"], base, "baseline")
    for i, f in enumerate(features):
        cols = f if isinstance(f, tuple) else (f,)
        codes = r["codes"][i] if isinstance(f, tuple) else (r["codes"][i],)
        values = r["values"][i] if isinstance(f, tuple) else (r["values"][i],)
        shape = tuple(len(c) for c in codes)
        for c, cc, vv in zip(cols, codes, values):
            assert cc.dtype == np.int32 and _same(cc, m.partial_dependence_codes(k.thr, c)) and (len(cc) > 1) == (c in used)
            assert vv.dtype == np.float32 and _same(vv, k.thr[c][cc[1:] - 1])
        assert r["pd"][i].dtype == np.float64 and r["pd"][i].shape == shape + (D,)
        assert r["ice"][i].dtype == np.float32 and r["ice"][i].shape == shape + (n, D)
        # ---- checks 1 and 2: every cell of a column at the small shapes, first / last / middle otherwise and for pairs
        every = len(cols) == 1 and n <= 257
        _check_entry(k, r, i, [(j,) for j in range(shape[0])] if every else _sample(shape))
        # ---- check 4: the cell of an untested column is the baseline
        if len(cols) == 1 and cols[0] not in used:
            assert codes[0].tolist() == [0] and _same(r["pd"][i][0], r["baseline"]) and _same(r["ice"][i][0], base)
    # ---- the curve at any code: a code that does not begin a segment, and the two ends
    for i, c in enumerate(tested):
        cc = r["codes"][i]
        inside = [g for g in range(B + 1) if g not in cc.tolist()] or [0]
        for g in sorted({0, B, inside[0], inside[len(inside) // 2], inside[-1]}):
            j = int(np.searchsorted(cc, g, side="right")) - 1
            assert _same(r["ice"][i][j], k.oracle(((c, g),))), (c, g, j)
    # ---- check 3: the same bytes again, without the ICE rows, through the general kernel, and with every row named
    assert _same_result(k.run(features, ice=True), r, True)
    assert "ice" not in k.run(features) and _same_result(k.run(features), r, False)
    with _env("GBRL_HIP_PD_GENERIC", "1"):
        assert _same_result(k.run(features, ice=True), r, True)
        assert _same_result(k.run(features), r, False)
    assert _same_result(k.run(features, ice=True, rows=np.arange(n, dtype=np.int32)), r, True)
    assert _same_result(k.run(features, n_trees=T, ice=True), r, True) and _same_result(k.run(features, n_trees=-1), r, False)
    # ---- one n_trees prefix: the model truncated there
    if T > 1:
        kt = T // 2
        part = k.run(features, n_trees=kt, ice=True)
        _check_mean(part["baseline"], k.oracle((), kt), "baseline of %d trees" % kt)
        assert not _same(part["baseline"], r["baseline"])
        for i, f in enumerate(features):
            first = part["codes"][i][0] if isinstance(f, tuple) else part["codes"][i]
            full = r["codes"][i][0] if isinstance(f, tuple) else r["codes"][i]
            assert set(first.tolist()) <= set(full.tolist())
            _check_entry(k, part, i, _sample(part["pd"][i].shape[:-1]), stop=kt)
    # ---- check 5: nothing was written
    assert _file(m, tmp_path) == file0 and k.ds.codes().tobytes() == codes0


def test_an_untested_column_is_the_baseline():
    """one tree of depth 3 tests at most 3 of 17 columns: every other column has codes [0], is not launched and reports the baseline's bytes"""
    k = Case(257, 17, 3, "oblivious", 7)
    used = k.used(1)
    free = [c for c in range(17) if c not in used]
    assert len(free) >= 14 and used
    busy = sorted(used)[0]
    r = k.run(free[:3] + [busy, (free[0], busy), (free[0], free[1])], n_trees=1, ice=True)
    base = k.oracle((), 1)
    _check_mean(r["baseline"], base, "baseline of 1 tree")
    for i in range(3):
        assert r["codes"][i].tolist() == [0] and r["values"][i].shape == (0,)
        assert r["pd"][i].shape == (1, 3) and _same(r["pd"][i][0], r["baseline"]) and _same(r["ice"][i][0], base)
    assert len(r["codes"][3]) > 1
    _check_entry(k, r, 3, [(j,) for j in range(len(r["codes"][3]))], stop=1)
    # a pair with an untested column is its other column's curve; a pair of two untested columns is the baseline
    assert r["pd"][4].shape == (1, len(r["codes"][3]), 3) and _same(r["pd"][4][0], r["pd"][3]) and _same(r["ice"][4][0], r["ice"][3])
    assert r["pd"][5].shape == (1, 1, 3) and _same(r["pd"][5][0, 0], r["baseline"]) and _same(r["ice"][5][0, 0], base)
    with _env("GBRL_HIP_PD_GENERIC", "1"):
        assert _same_result(k.run(free[:3] + [busy, (free[0], busy), (free[0], free[1])], n_trees=1, ice=True), r, True)


@pytest.mark.parametrize("m_rows", [1, 65])
def test_rows_with_duplicates_out_of_a_larger_data_set(m_rows):
    k = Case(257, 17, 3, "greedy", 7)
    rng = np.random.default_rng(m_rows)
    rows = rng.integers(0, 257, m_rows).astype(np.int32)
    if m_rows > 1:
        rows[3] = rows[64] = rows[0]          # duplicates, in both tiles of the row list
        rows[63] = 256                        # the last row of the data set
    features = [0, 16, (15, 16)]
    r = k.run(features, rows=rows, ice=True)
    assert r["rows"] == m_rows
    _check_mean(r["baseline"], k.oracle()[rows], "baseline")
    for i, f in enumerate(features):
        shape = r["pd"][i].shape[:-1]
        assert r["ice"][i].shape == shape + (m_rows, 3)
        _check_entry(k, r, i, [(j,) for j in range(shape[0])] if len(shape) == 1 else _sample(shape), rows=rows)
    with _env("GBRL_HIP_PD_GENERIC", "1"):
        assert _same_result(k.run(features, rows=rows, ice=True), r, True)
    assert _same_result(k.run(features, rows=rows), r, False)


WIDE = [
    # D, optimizers: the general kernel's widths, a Linear schedule, two optimizers over disjoint outputs
    (65, None),
    (128, None),
    (3, [dict(algo="SGD", scheduler="Linear", init_lr=0.1, stop_lr=0.01, T=50, start_idx=0, stop_idx=3)]),
    (8, [dict(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=3), dict(algo="SGD", scheduler="Const", init_lr=0.03, start_idx=3, stop_idx=8)]),
]


@pytest.mark.parametrize("D,opts", WIDE)
def test_wide_outputs_schedules_and_two_optimizers(D, opts):
    k = Case(65, 17, D, "oblivious", 7, opts=opts)
    used = k.used()
    tested = _tested(17)
    assert 2 * len([c for c in tested if c in used]) >= len(tested), (tested, sorted(used))
    features = [0, 16, (15, 16)]
    r = k.run(features, ice=True)
    _check_mean(r["baseline"], k.oracle(), "baseline")
    for i in range(len(features)):
        _check_entry(k, r, i, _sample(r["pd"][i].shape[:-1]))
    with _env("GBRL_HIP_PD_GENERIC", "1"):
        assert _same_result(k.run(features, ice=True), r, True)
    assert _same_result(k.run(features), r, False)


def test_a_pair_with_more_cells_than_one_launch_takes():
    """flat weights and a large rate spread the splits: the two columns with the most breaks span more cells than a launch's variants (64 at this
    shape), and the cells on both sides of the boundary equal the oracle like the first and the last"""
    k = Case(257, 17, 3, "greedy", 40, flat=True, lr=0.5)
    geo = cpp.partial_dependence_geometry(257, 3)
    assert geo["launch_variants"] == geo["max_launch_variants"] == 64 and geo["partial_rows"] == 64
    breaks = sorted(((len(k.m.partial_dependence_codes(k.thr, c)), c) for c in range(17)), reverse=True)
    (n0, c0), (n1, c1) = breaks[0], breaks[1]
    assert n0 * n1 + 1 > geo["launch_variants"], breaks
    assert (np.diff(k.thr[c0]) > 0).all() and (np.diff(k.thr[c1]) > 0).all()
    r = k.run([(c0, c1)], ice=True)
    assert r["pd"][0].shape == (n0, n1, 3)
    edge = [divmod(v, n1) for v in (62, 63, 64) if v < n0 * n1]          # variant 0 is the baseline: cell 63 opens the second launch
    _check_entry(k, r, 0, sorted(set(_sample((n0, n1)) + edge)))
    with _env("GBRL_HIP_PD_GENERIC", "1"):
        assert _same_result(k.run([(c0, c1)], ice=True), r, True)
    assert _same_result(k.run([(c0, c1)]), r, False)
    # ---- max_cells refuses the entry, naming it and both counts
    with pytest.raises(RuntimeError, match=r"entry 1 of features \(columns %d and %d\) has %d x %d = %d cells, max_cells is %d" % (c0, c1, n0, n1, n0 * n1, n0 * n1 - 1)):
        k.run([c0, (c0, c1)], max_cells=n0 * n1 - 1)
    with pytest.raises(RuntimeError, match=r"entry 0 of features \(column %d\) has %d cells, max_cells is %d" % (c0, n0, n0 - 1)):
        k.run([c0], max_cells=n0 - 1)
    assert _same(k.run([(c0, c1)], max_cells=n0 * n1)["pd"][0], r["pd"][0])


def test_refusals(tmp_path):
    k = Case(65, 17, 3, "oblivious", 7)
    m, ds, F, B = k.m, k.ds, k.F, k.B
    file0 = _file(m, tmp_path)
    P = m.partial_dependence_prepared

    def refused(word, *a, **kw):
        with pytest.raises(RuntimeError, match=word):
            P(*a, **kw)

    refused("features is empty", ds, [])
    refused("sequence of columns", ds, 3)
    refused(r"names column 17, outside \[0, 17\)", ds, [F])
    refused(r"names column -1, outside \[0, 17\)", ds, [0, -1])
    refused(r"entry 1 of features names column 40, outside", ds, [0, (3, 40)])
    refused("names column 5 twice", ds, [(5, 5)])
    refused("has 3 columns: a pair has two", ds, [(1, 2, 3)])
    refused("neither a column nor a pair", ds, [0.5])
    refused("max_cells must be >= 1", ds, [0], max_cells=0)
    refused("n_trees 0 is outside", ds, [0], n_trees=0)
    refused("n_trees 8 is outside", ds, [0], n_trees=8)
    refused("n_trees -2 is outside", ds, [0], n_trees=-2)
    refused("null data set", None, [0])
    # rows: step_prepared's rules
    refused("no rows", ds, [0], rows=np.zeros(0, np.int32))
    refused(r"index 65 \(entry 1\) is outside \[0, 65\)", ds, [0], rows=np.array([0, 65], np.int32))
    refused(r"index -1 \(entry 0\) is outside", ds, [0], rows=np.array([-1], np.int32))
    refused("Expected array of format", ds, [0], rows=np.array([0, 1], np.int64))
    # a model without trees
    fresh = _model(F, 3, "oblivious")
    with pytest.raises(RuntimeError, match="the model has no trees"):
        fresh.partial_dependence_prepared(fresh.prepare_dataset(k.X), [0])
    # what predict_continue_prepared refuses: another bin count, thresholds the trees do not compare against (the tree is named)
    with pytest.raises(RuntimeError, match="n_bins"):
        P(_model(F, 3, "oblivious", n_bins=16).prepare_dataset(k.X), [0])
    own = m.prepare_dataset(k.X)
    with pytest.raises(RuntimeError, match=r"tree \d+, condition \d+ .* does not compare against one of the data set's thresholds"):
        P(own, [0])
    # the C ABI takes explicit variants: its own refusals, with the documented status
    import ctypes as C
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.gbrl_hip_partial_dependence_prepared.argtypes = [vp, vp, vp, ci, vp, ci, ci, ci, vp, vp, ci]
    sums = np.zeros((2, 3), np.float64)

    def c_call(variants, n=65, sums_ptr=sums.ctypes.data, n_variants=None, ice=None):
        v = np.asarray(variants, np.int32).reshape(-1, 4)
        return lib.gbrl_hip_partial_dependence_prepared(m._handle(), ds._handle(), v.ctypes.data, len(v) if n_variants is None else n_variants, None, 0, n, -1, sums_ptr, ice, 0)

    for variants, word in (([[0, B + 1, -1, 0]], b"code 33 of column 0 is outside [0, 32]"), ([[0, -1, -1, 0]], b"code -1 of column 0"),
                           ([[0, 0, 16, B + 1]], b"code 33 of column 16"), ([[F, 0, -1, 0]], b"names column 17, outside"), ([[-2, 0, -1, 0]], b"names column -2"),
                           ([[3, 0, 3, 1]], b"names column 3 twice"), ([[-1, 0, 3, 1]], b"col1 without col0")):
        assert c_call(variants) == -1 and word in lib.gbrl_hip_last_error(), (variants, lib.gbrl_hip_last_error())
    assert c_call([[0, 0, -1, 0]], sums_ptr=None) == -1 and b"no place for the result" in lib.gbrl_hip_last_error()
    assert c_call([[0, 0, -1, 0]], n_variants=0) == -1 and b"no variants" in lib.gbrl_hip_last_error()
    assert c_call([[0, 0, -1, 0]], n=64) == -1 and b"has 64 rows, the data set 65" in lib.gbrl_hip_last_error()
    # ICE rows of 2^31 elements or more: refused before anything is allocated (V is read, the variants are not walked past the checks)
    big = np.tile(np.array([[0, 0, -1, 0]], np.int32), (1 << 20, 1))
    rows = np.zeros(700, np.int32)
    small = np.zeros(16, np.float32)          # a real buffer: the size check does not read through the pointer, and nothing may be written
    lib_rows = rows.ctypes.data
    assert (1 << 20) * 700 * 3 >= 1 << 31
    rc = lib.gbrl_hip_partial_dependence_prepared(m._handle(), ds._handle(), big.ctypes.data, len(big), lib_rows, 0, 700, -1, sums.ctypes.data, small.ctypes.data, 0)
    assert rc == -5 and b"pass rows=" in lib.gbrl_hip_last_error(), lib.gbrl_hip_last_error()
    assert not small.any()
    # the explicit variants of the C ABI: any code in [0, B], the sums of the baseline and of one cell
    two = np.zeros((2, 3), np.float64)
    g = 7
    v = np.array([[-1, 0, -1, 0], [16, g, -1, 0]], np.int32)
    assert lib.gbrl_hip_partial_dependence_prepared(m._handle(), ds._handle(), v.ctypes.data, 2, None, 0, 65, -1, two.ctypes.data, None, 0) == 0, lib.gbrl_hip_last_error()
    r = k.run([16])
    j = int(np.searchsorted(r["codes"][0], g, side="right")) - 1
    assert _same(two[0] / 65.0, r["baseline"]) and _same(two[1] / 65.0, r["pd"][0][j])
    assert _file(m, tmp_path) == file0
