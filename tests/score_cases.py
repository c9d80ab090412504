"""The inputs, the exact reference and the entry point shared by tests/test_score_host.py (CPU: the refusals of gbrl_hip_score_probe, the
reference itself) and tests/test_gpu_score_cells.py (the kernels of step_score.hip, cell by cell).

The reference works in exact integer arithmetic (Python ints in NumPy object arrays): suffix sums by np.cumsum over the reversed classes, a
candidate's exact value (|S_L|^2 / n_L + |S_R|^2 / n_R) * 2^(-2 sbits) as a ratio of integers -- a side without rows contributes nothing --, under
Cosine its square root through math.isqrt, and the expected float32 is that value rounded ONCE (f32_from_ratio, f32_sqrt_ratio).

The selection outputs are not compared with the exact scores again: `select` and the functions built on it restate the reduction rule on the host
and are applied to the scores the probe itself returned in scores mode, which the first group of tests has held to the exact reference."""
import ctypes
import decimal
import math
import os
from fractions import Fraction

import numpy as np

SENT64 = -0x5a5a5a5a5a5a5a5b            # what a cell that no kernel stored must still hold
SENT32 = 0x5a5a5a5b
SENTF = np.array([SENT32], np.int32).view(np.float32)[0]
E_INVALID = -1                          # GBRL_HIP_E_INVALID
NO_CAND = 0x7fffffff
MAX_PATH = 32
NEG_INF = np.float32(-np.inf)
NEAR_CLASS_ROWS = 1024                  # kNearClassRows

_PTRS = ("hist", "hist_prev", "hist_global", "sub_par", "sub_sib", "slots", "thr", "thr_keys", "path_len", "path_slot", "path_bin", "path_val", "cand_w", "cand_ref",
         "ref_to_internal", "cand_slot", "is_root", "seg_start", "scores", "parent", "part_v", "part_s", "best_score", "cand_nr", "part_i", "part_n", "best_idx", "splits",
         "cursors", "counts4")
_INTS = ("n_hist_nodes", "n_prev_nodes", "n_nodes", "Fp", "n_classes", "output_dim", "n_table_slots", "B", "n_cand", "sbits", "min_data", "cosine", "slot0", "n_slots",
         "keep_derived", "do_score", "do_argmax", "do_resolve", "n_parts", "oblivious", "near", "max_front")


class ProbeArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _PTRS] + [("near_rows", ctypes.c_longlong), ("near_rel", ctypes.c_float)] + [(n, ctypes.c_int) for n in _INTS]


_lib = None


def lib():
    global _lib
    if _lib is None:
        import gbrl_amd
        so = ctypes.CDLL(os.path.join(os.path.dirname(gbrl_amd.__file__), "libgbrl_hip.so"))
        so.gbrl_hip_score_probe.restype = ctypes.c_int
        so.gbrl_hip_score_probe.argtypes = [ctypes.POINTER(ProbeArgs)]
        so.gbrl_hip_last_error.restype = ctypes.c_char_p
        _lib = so
    return _lib


# ------------------------------------------------------------------------------------------------------------ rounding, exactly once

def _floor_log2(num, den):
    """e with 2^e <= num / den < 2^(e + 1)"""
    e = num.bit_length() - den.bit_length()
    if (num < (den << e)) if e >= 0 else ((num << -e) < den):
        e -= 1
    return e


def _round_div(n, d):
    """n / d to the nearest integer, ties to even"""
    m, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and (m & 1)):
        m += 1
    return m


def f32_from_ratio(num, den, shift=0):
    """-> (the float32 nearest to num / den * 2^-shift, ties to even, as a Python float; the exponent of its unit in the last place).  num >= 0 < den"""
    if num == 0:
        return 0.0, -149
    q = max(_floor_log2(num, den) - shift, -126) - 23
    s = q + shift
    m = _round_div(num, den << s) if s >= 0 else _round_div(num << -s, den)
    return math.ldexp(m, q), q


def f32_sqrt_ratio(num, den, shift=0):
    """the same for sqrt(num / den) * 2^-shift"""
    if num == 0:
        return 0.0, -149
    q = max(_floor_log2(num, den) // 2 - shift, -126) - 23
    s = q + shift
    n2, d2 = (num, den << (2 * s)) if s >= 0 else (num << (-2 * s), den)
    m = math.isqrt(n2 // d2)                                   # floor(sqrt(x)), x = n2 / d2; the answer is m or m + 1: x against (m + 1/2)^2
    lhs, rhs = 4 * n2, (2 * m + 1) ** 2 * d2
    if lhs > rhs or (lhs == rhs and (m & 1)):
        m += 1
    return math.ldexp(m, q), q


def f32_from_fraction(x):
    """a Fraction rounded once to float32 (an exact zero is +0, as a sum of opposite terms is under round-to-nearest)"""
    if x == 0:
        return 0.0
    v = f32_from_ratio(abs(x.numerator), x.denominator)[0]
    return -v if x < 0 else v


def fma32(a, b, c):
    """float32 arrays: fma(a, b, c) rounded once.  The product of two float32 is exact in float64; where the float64 sum is exact too (two-sum
    error 0) its conversion is the single rounding, elsewhere the value is rounded from the exact Fraction."""
    a, b, c = (np.asarray(x, np.float32) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        cc = c.astype(np.float64)
        s = p + cc
        bb = s - p
        err = (p - (s - bb)) + (cc - bb)
        out = s.astype(np.float32)
    for i in np.flatnonzero(np.isfinite(s).ravel() & (err.ravel() != 0)):
        out.ravel()[i] = f32_from_fraction(Fraction(float(a.ravel()[i])) * Fraction(float(b.ravel()[i])) + Fraction(float(c.ravel()[i])))
    return out


# ------------------------------------------------------------------------------------------------------------ inputs

class Level:
    """The inputs of one gbrl_hip_score_probe call (make_level)."""

    def NBe(self, f):
        return min(self.NB, int(self.slots[f, 1]) + 1)


def class_sums(rng, n, D, data, count_max):
    """[n][D + 1] class sums (int64) of one (node, feature slot); field D is the row count"""
    v = np.zeros((n, D + 1), np.int64)
    if data == "zero":
        return v
    v[:, D] = rng.integers(0, count_max + 1, size=n)
    if data == "random":
        v[:, :D] = rng.integers(-(1 << 24), (1 << 24) + 1, size=(n, D))
    elif data == "negative":
        v[:, :D] = -rng.integers(1, 1 << 24, size=(n, D))
    elif data == "carry":
        # class values alternate around +-2^32: the running suffix sum (from the last class down) is about 2^32 after every other class and about 0
        # in between, on either side of a multiple of 2^32 by the offsets
        sign = np.where(np.arange(n)[::-1] % 2 == 0, 1, -1)[:, None] * np.where(rng.integers(0, 2, size=D) == 0, 1, -1)[None, :]
        v[:, :D] = sign * (1 << 32) + rng.integers(-1000, 1001, size=(n, D))
    elif data == "big":
        # one class per field holds +-(2^52 - 1) less the others' sum, so that suffix sums and totals reach +-(2^52 - 1) exactly
        v[:, :D] = rng.integers(-(1 << 20), (1 << 20) + 1, size=(n, D))
        if n > 1:
            for d in range(D):
                c = int(rng.integers(1, n))
                rest = int(v[1:, d].sum()) - int(v[c, d])
                v[c, d] = (1 if rng.integers(0, 2) else -1) * ((1 << 52) - 1) - rest
    else:
        raise ValueError(data)
    if data != "carry":                                        # (there a missing class would let the suffix sums drift away from 2^32)
        v[rng.random(n) < 0.1] = 0                             # all-zero classes
    return v


def set_suffix(L, node, f, sfx):
    """an accumulated node's classes of slot f from their suffix sums sfx [n_cand + 1][D + 1] (sfx[0] is the node's total)"""
    sfx = np.asarray(sfx, np.int64)
    E = sfx - np.concatenate([sfx[1:], np.zeros((1, sfx.shape[1]), np.int64)])
    assert L.kinds[node][0] != "der" and E.shape == L.eff[node][f].shape
    L.eff[node][f] = E
    L.hist[node, f, :len(E)] = E


def make_level(seed, D, slots, nodes=(("acc",),), *, data="random", sbits=20, min_data=1, cosine=0, count_max=50, NB=None, B=None, spare_slots=1, n_extra_hist=0):
    """slots: (is_cat, n_cand) per feature slot.  nodes: ("acc",) accumulated from data; ("zero",) accumulated, no rows; ("der", j) derived as
    parent - node j (j < 0: the parent alone).  Every slot of a node has the same totals, as real histograms have: class 0 makes up the rest."""
    rng = np.random.default_rng(seed)
    L = Level()
    T = len(slots)
    L.D, L.sbits, L.min_data, L.cosine, L.data = D, sbits, min_data, cosine, data
    L.NB = NB if NB is not None else max(nc for _, nc in slots) + 1
    L.B = B if B is not None else max([nc for c, nc in slots if not c] + [1])
    L.Fp = T + spare_slots
    L.n_nodes, L.n_hist_nodes = len(nodes), len(nodes) + n_extra_hist
    L.kinds = list(nodes)
    base = np.concatenate([[0], np.cumsum([nc for _, nc in slots])]).astype(np.int64)
    L.n_cand = max(1, int(base[-1]))
    L.slots = np.array([(c, nc, base[f], 0) for f, (c, nc) in enumerate(slots)], np.int32).reshape(T, 4)
    W = D + 1
    # the effective class sums of every (node, slot), classes below NBe
    eff = [[None] * T for _ in nodes]
    for k, kind in enumerate(nodes):
        parts = [class_sums(rng, L.NBe(f), D, "zero" if kind[0] == "zero" else data, count_max) for f in range(T)]
        tot = np.zeros(W, np.int64)
        if kind[0] != "zero":
            tot[:D] = rng.integers(-(1 << 20), (1 << 20) + 1, size=D) if data != "negative" else -rng.integers(1, 1 << 20, size=D)
            tot[D] = max(int(p[1:, D].sum()) for p in parts) + int(rng.integers(1, 6))
        for f in range(T):
            parts[f][0] = tot - parts[f][1:].sum(axis=0)
            eff[k][f] = parts[f]
    L.eff = eff
    der = [k for k, kind in enumerate(nodes) if kind[0] == "der"]
    L.n_prev_nodes = len(der) + 1 if der else 0
    L.hist = np.full((L.n_hist_nodes, L.Fp, L.NB, W), SENT64, np.int64)
    L.hist_prev = np.full((L.n_prev_nodes, L.Fp, L.NB, W), SENT64, np.int64) if der else None
    L.sub_par = np.full(L.n_nodes, -1, np.int32) if der else None
    L.sub_sib = np.full(L.n_nodes, -1, np.int32) if der else None
    for k, kind in enumerate(nodes):
        if kind[0] == "der":
            assert kind[1] < 0 or nodes[kind[1]][0] != "der"
            par = 1 + der.index(k)
            L.sub_par[k], L.sub_sib[k] = par, kind[1]
            for f in range(T):
                L.hist_prev[par, f, :L.NBe(f)] = eff[k][f] + (eff[kind[1]][f] if kind[1] >= 0 else 0)
        else:
            for f in range(T):
                L.hist[k, f, :L.NBe(f)] = eff[k][f]
    L.thr = np.zeros((T, L.B), np.float32)
    for f, (c, nc) in enumerate(slots):
        if not c:
            L.thr[f, :nc] = (np.arange(nc) * 0.25 + f).astype(np.float32)
    L.thr_keys = rng.integers(0, 1 << 32, size=(T, L.B), dtype=np.uint64).astype(np.uint32)
    L.path_len = np.zeros(L.n_nodes, np.int32)
    L.path_slot = np.full((L.n_nodes, MAX_PATH), -1, np.int32)
    L.path_val = np.zeros((L.n_nodes, MAX_PATH), np.float32)
    L.path_bin = np.zeros((L.n_nodes, MAX_PATH), np.int32)
    L.cand_w = (0.5 + rng.random(L.n_cand)).astype(np.float32)
    L.cand_ref = rng.permutation(L.n_cand).astype(np.int32)
    L.ref_to_internal = np.argsort(L.cand_ref).astype(np.int32)
    L.cand_slot = np.zeros(L.n_cand, np.int32)
    for f in range(T):
        L.cand_slot[base[f]:base[f + 1]] = f
    L.is_root = np.zeros(L.n_nodes, np.int32)
    L.slot0, L.n_slots, L.keep_derived = 0, T, 1
    return L


def set_path(L, node, entries, length=None):
    """entries: (slot, value, bin) from position 0; `length` (default: all of them) is path_len -- entries behind it must be ignored"""
    for i, (f, val, b) in enumerate(entries):
        L.path_slot[node, i], L.path_val[node, i], L.path_bin[node, i] = f, val, b
    L.path_len[node] = len(entries) if length is None else length


# ------------------------------------------------------------------------------------------------------------ the exact reference

def obj(a):
    return np.asarray(a, np.int64).astype(object)


def suffix_sums(E):
    """[n][W] object array -> suffix sums over the classes (class c and everything above it)"""
    return np.cumsum(E[::-1], axis=0)[::-1]


def near_class(n_right, n_node):
    return 0 if (n_node <= NEAR_CLASS_ROWS or n_right == n_node) else int(n_right)


class Ref:
    pass


def reference_scores(L, suffix_fault=None):
    """-> Ref: scores / parent as the once-rounded float32 (SENTF where no block stores), exact[node][j] = (num, den, ulp exponent) or None where the
    candidate is rejected, cand_nr, and the histograms as the kernel must leave them.  suffix_fault = (node, slot, class, field, delta) adds delta
    to one suffix sum before it is scored: what a wrong scan would do."""
    D, W, sh = L.D, L.D + 1, L.sbits
    R = Ref()
    R.scores = np.full((L.n_nodes, L.n_cand), SENTF, np.float32)
    R.cand_nr = np.full((L.n_nodes, L.n_cand), SENT32, np.int32)
    R.parent = np.full(L.n_nodes, SENTF, np.float32)
    R.exact = [[None] * L.n_cand for _ in range(L.n_nodes)]
    R.parent_exact = [None] * L.n_nodes
    R.hist = L.hist.copy()
    rnd = f32_sqrt_ratio if L.cosine else f32_from_ratio
    shift = sh if L.cosine else 2 * sh
    for k in range(L.n_nodes):
        np_k = int(L.path_len[k])
        for f in range(L.slot0, L.slot0 + L.n_slots):
            is_cat, nc, base = (int(x) for x in L.slots[f, :3])
            E = obj(L.eff[k][f])
            if L.kinds[k][0] == "der" and L.keep_derived:
                R.hist[k, f, :nc + 1] = L.eff[k][f]
            tot = E.sum(axis=0)
            right = (E if is_cat else suffix_sums(E))[1:nc + 1].copy()
            if suffix_fault is not None and suffix_fault[:2] == (k, f):
                right[suffix_fault[2] - 1, suffix_fault[3]] += suffix_fault[4]
            n_tot = int(tot[D])
            if f == L.slot0:
                num = int((tot[:D] ** 2).sum()) if n_tot > 0 else 0
                v, q = rnd(num, max(n_tot, 1), shift)
                R.parent[k], R.parent_exact[k] = v, (num, max(n_tot, 1), q)
            if nc == 0:
                continue
            left = tot[None, :] - right
            sr2, sl2 = (right[:, :D] ** 2).sum(axis=1), (left[:, :D] ** 2).sum(axis=1)
            hits = [i for i in range(np_k) if L.path_slot[k, i] == f]
            for c in range(nc):
                n_r, n_l = int(right[c, D]), int(left[c, D])
                j = base + c
                R.cand_nr[k, j] = near_class(n_r, n_tot)
                reject = n_l < L.min_data or n_r < L.min_data
                for i in hits:
                    reject |= (L.path_bin[k, i] == c + 1) if is_cat else bool(L.path_val[k, i] == L.thr[f, c])
                if reject:
                    R.scores[k, j] = NEG_INF
                    continue
                if n_l > 0 and n_r > 0:
                    num, den = int(sl2[c]) * n_r + int(sr2[c]) * n_l, n_l * n_r
                elif n_l > 0:
                    num, den = int(sl2[c]), n_l
                elif n_r > 0:
                    num, den = int(sr2[c]), n_r
                else:
                    num, den = 0, 1
                v, q = rnd(num, den, shift)
                R.scores[k, j], R.exact[k][j] = v, (num, den, q)
    return R


def exact_value(L, ex):
    """the exact score as a decimal of 80 digits"""
    num, den, _ = ex
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        x = decimal.Decimal(num) / decimal.Decimal(den)
        return (x.sqrt() if L.cosine else x) * decimal.Decimal(2) ** (-(L.sbits if L.cosine else 2 * L.sbits))


def within_bound(L, got, ex):
    """|got - exact| <= ulp32(exact) / 2 + exact * (D + 5) * 2^-53: the kernel evaluates in fp64 with non-negative terms, so its fp64 result is within
    (D + 5) * 2^-53 relative of the exact value, and is then rounded to float32 once"""
    if not np.isfinite(got):
        return False
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        x = exact_value(L, ex)
        two = decimal.Decimal(2)
        return abs(decimal.Decimal(float(got)) - x) <= two ** ex[2] / 2 + x * (L.D + 5) * two ** -53


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def score_failures(L, got, R):
    """the (node, candidate) cells where `got` misses the reference: bit equality with the once-rounded value, or -- a last-bit case -- the derived
    bound; rejected candidates exactly -inf; cells no block stores exactly the sentinel"""
    bad = []
    for k, j in zip(*np.nonzero(bits(got) != bits(R.scores))):
        if R.exact[k][j] is None or not within_bound(L, got[k, j], R.exact[k][j]):
            bad.append((int(k), int(j)))
    return bad


def parent_failures(L, got, R):
    return [k for k in np.flatnonzero(bits(got) != bits(R.parent)) if not within_bound(L, got[k], R.parent_exact[k])]


# ------------------------------------------------------------------------------------------------------------ the reduction rule

def select(gain, ref, cls):
    """The set rule: the highest gain wins, then the lowest reference index; all -inf: no winner.  second = the best gain of a candidate whose
    (gain, class) differs from the winner's.  -> (reference index or NO_CAND, gain, second, the winner's class or None)"""
    gain = np.asarray(gain, np.float32)
    live = np.flatnonzero(gain > NEG_INF)
    if len(live) == 0:
        return NO_CAND, NEG_INF, NEG_INF, None
    top = gain[live].max()
    cands = live[gain[live] == top]
    w = cands[np.argmin(np.asarray(ref)[cands])]
    other = (gain != top) | (np.asarray(cls) != cls[w])
    second = gain[other].max() if other.any() else NEG_INF
    return int(ref[w]), top, np.float32(second), int(cls[w])


def gains(L, scores, parent):
    """[n_nodes][n_cand]: fma(score, w, -parent), a root's parent = 0"""
    par = np.where(L.is_root != 0, np.float32(0), parent).astype(np.float32)
    return fma32(scores, L.cand_w[None, :], -par[:, None])


def expected_greedy_parts(L, scores, parent, cand_nr, with_n):
    """what the fused greedy form of k_score must leave per (node, launched slot), from the scores of the same inputs"""
    g = gains(L, scores, parent)
    shape = (L.n_nodes, L.n_slots)
    pv, pi, ps, pn = np.full(shape, NEG_INF, np.float32), np.full(shape, NO_CAND, np.int32), np.full(shape, NEG_INF, np.float32), np.full(shape, -1, np.int32)
    for k in range(L.n_nodes):
        for b in range(L.n_slots):
            _, nc, base = (int(x) for x in L.slots[L.slot0 + b, :3])
            if nc == 0:
                continue
            cls = cand_nr[k, base:base + nc] if with_n else np.zeros(nc, np.int32)
            i, v, s, c = select(g[k, base:base + nc], L.cand_ref[base:base + nc], cls)
            pv[k, b], pi[k, b], ps[k, b] = v, i, s
            if c is not None:
                pn[k, b] = c
    return pv, pi, ps, pn


def expected_argmax(L, scores):
    """k_argmax_stage1, the oblivious form: float32 sum over the nodes in node order, times w; one (best, index, second) per 256 candidates"""
    sc = np.zeros(L.n_cand, np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(L.n_nodes):
            sc = (sc + scores[k]).astype(np.float32)
        sc = (sc * L.cand_w).astype(np.float32)
    parts = -(-L.n_cand // 256)
    pv, pi, ps = np.full(parts, NEG_INF, np.float32), np.full(parts, NO_CAND, np.int32), np.full(parts, NEG_INF, np.float32)
    for b in range(parts):
        lo, hi = b * 256, min(L.n_cand, b * 256 + 256)
        pi[b], pv[b], ps[b], _ = select(sc[lo:hi], L.cand_ref[lo:hi], np.zeros(hi - lo, np.int32))
    return pv, pi, ps, sc


def merge_parts(pv, pi, ps, pn):
    """the last stage of the selection over one node's per-block results -> (index or NO_CAND, gain, second)"""
    n = len(pv)
    cls = np.zeros(n, np.int32) if pn is None else np.asarray(pn)
    i, v, s, _ = select(pv, pi, cls)
    if ps is not None:
        s = np.float32(max(s, np.max(ps)))
    return i, v, s


def near_window_rel(rel, rows):
    rel = np.float32(rel)
    return max(rel, np.float32(np.float32(1.1920929e-07) * np.sqrt(np.float32(rows)))) if rows > 8192 else rel


def expected_resolve(L, pv, pi, ps, pn, *, oblivious, near=0, near_rel=0.0, near_rows=0, parent=None, seg_start=None, hist_global=None, thr_keys=True, max_front=None):
    """k_resolve_splits on the per-block results pv / pi (/ ps / pn): [n_nodes][n_parts] (oblivious: row 0 serves every node).  The class counts of
    a node are L.eff's whether the node was accumulated, derived and written back, or (last level, keep_derived = 0) derived by the kernel
    itself from parent - sibling."""
    mf = L.n_nodes if max_front is None else max_front
    D = L.D
    R = Ref()
    R.best_idx, R.best_score = np.full(mf, SENT32, np.int32), np.full(mf, SENTF, np.float32)
    R.counts4 = np.full((4, mf), SENT64, np.int64)
    R.splits = np.zeros((L.n_nodes, 8), np.int32)
    R.cursors = np.full((L.n_nodes, 2), SENT32, np.int32)
    R.second = np.full(L.n_nodes, NEG_INF, np.float32)
    for k in range(L.n_nodes):
        src = 0 if oblivious else k
        i, v, s = merge_parts(pv[src], pi[src], ps[src] if (near and ps is not None) else None, pn[src] if (near and pn is not None) else None)
        if not near:
            s = NEG_INF
        R.second[k] = s
        best = 0 if i == NO_CAND else i
        if k == src:
            R.best_idx[k], R.best_score[k] = best, v
        j = int(L.ref_to_internal[best])
        f = int(L.cand_slot[j])
        is_cat, nc, base = (int(x) for x in L.slots[f, :3])
        b = j - base + 1 if is_cat else j - base
        n = obj(L.eff[k][f])[:, D]
        tot = int(n.sum())
        right = int(n[b]) if is_cat else int(n[b + 1:].sum())
        R.counts4[0, k], R.counts4[1, k] = tot, right
        if hist_global is not None:
            g = obj(hist_global[k, f, :nc + 1, D])
            R.counts4[2, k], R.counts4[3, k] = int(g.sum()), int(g[b]) if is_cat else int(g[b + 1:].sum())
        else:
            if k == src:
                R.counts4[3, k] = int(np.array([s], np.float32).view(np.int32)[0])
            flag = 0
            if near and v != NEG_INF and k == src:
                with np.errstate(over="ignore"):
                    if oblivious:
                        mag = np.abs(v)
                    else:
                        par = np.float32(0) if L.is_root[k] else np.float32(parent[k])
                        mag = max(np.abs(np.float32(v + par)), np.abs(par))
                    win = np.float32(near_window_rel(near_rel, near_rows if oblivious else tot) * np.float32(mag))
                    if s != NEG_INF and np.float32(v - s) <= win:
                        flag = 1
                    if not oblivious and not L.is_root[k] and np.abs(v) <= win and not (L.cosine == 0 and (right == 0 or right == tot)):
                        flag = 1
            R.counts4[2, k] = flag
        q = R.splits[k]
        q[1], q[2], q[3] = f, b, is_cat
        if not is_cat and thr_keys:
            q[6] = np.array([L.thr_keys[f, b]], np.uint32).view(np.int32)[0]
        if seg_start is not None:
            q[0] = int(v != NEG_INF) if oblivious else int(v >= 0)
            q[4], q[5] = seg_start[k], tot - right
            R.cursors[k] = 0
    return R


# ------------------------------------------------------------------------------------------------------------ the entry point

class Out:
    pass


def probe(L, *, do_score=1, do_argmax=0, do_resolve=0, oblivious=0, near=0, near_rel=0.0, near_rows=0, with_s=False, with_n=False, with_nr=False, parts=None, n_parts=None,
          seg_start=None, hist_global=None, thr_keys=True, max_front=None, scores=None, parent=None, overrides=None, drop=()):
    """One gbrl_hip_score_probe call -> Out (rc, the error text, and every output array; the arrays the call does not take are None).
    parts = (part_v, part_i, part_s or None, part_n or None) given directly; overrides: ProbeArgs fields set last; drop: pointers set to null."""
    o = Out()
    mf = L.n_nodes if max_front is None else max_front
    if n_parts is None:
        n_parts = L.n_slots if do_score == 2 else (-(-L.n_cand // 256) if do_argmax else (parts[0].shape[-1] if parts is not None else 0))
    o.hist = L.hist.copy()
    o.scores = np.full((L.n_nodes, L.n_cand), SENTF, np.float32) if scores is None else np.array(scores, np.float32)
    o.parent = np.full(L.n_nodes, SENTF, np.float32) if parent is None else np.array(parent, np.float32)
    o.cand_nr = np.full((L.n_nodes, L.n_cand), SENT32, np.int32) if with_nr else None
    shape = (L.n_nodes, max(n_parts, 1))
    o.part_v = o.part_i = o.part_s = o.part_n = None
    if do_score == 2 or do_argmax or do_resolve:
        o.part_v, o.part_i = np.full(shape, SENTF, np.float32), np.full(shape, SENT32, np.int32)
        o.part_s = np.full(shape, SENTF, np.float32) if with_s else None
        o.part_n = np.full(shape, SENT32, np.int32) if with_n else None
        if parts is not None:
            o.part_v, o.part_i = np.array(parts[0], np.float32).reshape(shape), np.array(parts[1], np.int32).reshape(shape)
            o.part_s = None if parts[2] is None else np.array(parts[2], np.float32).reshape(shape)
            o.part_n = None if parts[3] is None else np.array(parts[3], np.int32).reshape(shape)
    o.best_idx, o.best_score = np.full(mf, SENT32, np.int32), np.full(mf, SENTF, np.float32)
    o.counts4 = np.full((4, mf), SENT64, np.int64)
    o.splits = np.full((L.n_nodes, 8), SENT32, np.int32)
    o.cursors = np.full((L.n_nodes, 2), SENT32, np.int32)
    ins = dict(hist_prev=L.hist_prev, hist_global=hist_global, sub_par=L.sub_par, sub_sib=L.sub_sib, slots=L.slots, thr=L.thr, thr_keys=L.thr_keys if thr_keys else None,
               path_len=L.path_len, path_slot=L.path_slot, path_bin=L.path_bin, path_val=L.path_val, cand_w=L.cand_w, cand_ref=L.cand_ref, ref_to_internal=L.ref_to_internal,
               cand_slot=L.cand_slot, is_root=L.is_root, seg_start=None if seg_start is None else np.asarray(seg_start, np.int32))
    dtypes = dict(hist_prev=np.int64, hist_global=np.int64, thr=np.float32, thr_keys=np.uint32, path_val=np.float32, cand_w=np.float32)
    keep = {n: np.ascontiguousarray(a, dtypes.get(n, np.int32)) for n, a in ins.items() if a is not None}
    a = ProbeArgs()
    for n, arr in keep.items():
        setattr(a, n, arr.ctypes.data)
    for n in ("hist", "scores", "parent", "cand_nr", "part_v", "part_i", "part_s", "part_n", "best_idx", "best_score", "counts4", "splits", "cursors"):
        if getattr(o, n) is not None:
            assert getattr(o, n).flags.c_contiguous
            setattr(a, n, getattr(o, n).ctypes.data)
    a.near_rows, a.near_rel = near_rows, near_rel
    a.n_hist_nodes, a.n_prev_nodes, a.n_nodes, a.Fp, a.n_classes, a.output_dim = L.n_hist_nodes, L.n_prev_nodes, L.n_nodes, L.Fp, L.NB, L.D
    a.n_table_slots, a.B, a.n_cand, a.sbits, a.min_data, a.cosine = len(L.slots), L.B, L.n_cand, L.sbits, L.min_data, L.cosine
    a.slot0, a.n_slots, a.keep_derived = L.slot0, L.n_slots, L.keep_derived
    a.do_score, a.do_argmax, a.do_resolve, a.n_parts, a.oblivious, a.near, a.max_front = do_score, do_argmax, do_resolve, n_parts, oblivious, near, mf
    for n in drop:
        setattr(a, n, None)
    for n, v in (overrides or {}).items():
        setattr(a, n, v)
    o.rc = lib().gbrl_hip_score_probe(ctypes.byref(a))
    o.error = (lib().gbrl_hip_last_error() or b"").decode() if o.rc != 0 else ""
    if o.rc not in (0, E_INVALID):                             # a device error: nothing more is started on a device that may have faulted
        import pytest
        pytest.exit("gbrl_hip_score_probe failed on the device: " + o.error, returncode=3)
    return o
