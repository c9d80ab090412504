"""The host side of gbrl_hip_score_probe and the exact reference of tests/score_cases.py, without a device: the symbol, every refusal (nothing a
kernel would index outside its arrays reaches a device), the reference on a case small enough to count by hand, the once-only float32 rounding
against np.float32 where rounding twice differs, the reduction rule against the kernels' merge steps in random merge orders, and that the
comparison of tests/test_gpu_score_cells.py does fail on a score one float32 ulp off and on a suffix sum 2^32 off."""
import ctypes
import math
from fractions import Fraction

import numpy as np

import score_cases as S


def _small(**kw):
    return S.make_level(1, 2, [(0, 5), (1, 3), (0, 0)], nodes=(("acc",), ("der", 0)), **kw)


def _refused(L, text, **kw):
    o = S.probe(L, **kw)
    assert np.array_equal(o.hist, L.hist), "a refused call must not touch its arrays"
    return o.rc == S.E_INVALID and text in o.error


def test_the_symbol_is_exported():
    assert S.lib().gbrl_hip_score_probe
    assert S.lib().gbrl_hip_score_probe(None) == S.E_INVALID


def test_refusals_on_the_host():
    for name in ("hist", "slots", "thr", "path_len", "path_slot", "path_bin", "path_val", "cand_w", "cand_ref", "ref_to_internal", "cand_slot", "is_root", "parent", "scores"):
        assert _refused(_small(), "null array", drop=(name,)), name
    assert _refused(_small(), "null array", do_score=2, n_parts=3, drop=("part_v",))
    assert _refused(_small(), "null array", do_resolve=1, n_parts=3, parts=(np.zeros((2, 3)), np.zeros((2, 3)), None, None), drop=("counts4",))
    for field, value in (("n_nodes", 0), ("n_nodes", 3), ("n_hist_nodes", 5000), ("Fp", 2), ("n_classes", 1), ("output_dim", 0), ("output_dim", 513), ("B", 0), ("n_cand", 0),
                         ("sbits", 41), ("sbits", -1), ("min_data", -1), ("max_front", 1), ("n_table_slots", 0)):
        assert _refused(_small(), "a size is out of range", overrides={field: value}), (field, value)
    assert _refused(_small(), "do_score is 0, 1 or 2", overrides={"do_score": 3})
    assert _refused(_small(), "do_score is 0, 1 or 2", do_score=2, do_argmax=1)
    # the LDS tile: (n_classes + 2) x (D + 1) x 8 bytes over 150 KiB
    assert (6398 + 2) * 3 * 8 == 150 * 1024 and _refused(_small(), "the launch window", overrides={"n_classes": 6398, "slot0": -1})      # (a later check)
    assert _refused(_small(), "does not fit the LDS", overrides={"n_classes": 6399})
    for col, value in ((1, -1), (1, 9), (2, -1), (2, 7), (0, 2)):
        L = _small()
        L.slots[1, col] = value
        assert _refused(L, "a slot's candidates leave [0, n_cand)"), (col, value)
    L = _small()
    L.slots[0, 1], L.slots[1, 2], L.slots[1, 1] = 8, 8, 0            # 8 candidates, 6 classes
    assert _refused(L, "more candidates than classes")
    for arr, value, text in (("sub_par", 2, "outside hist_prev"), ("sub_sib", 2, "outside hist")):
        L = _small()
        getattr(L, arr)[1] = value
        assert _refused(L, text), arr
    L = _small()
    L.hist_prev = None
    assert _refused(L, "outside hist_prev")
    L = _small()
    L.sub_sib = None
    assert _refused(L, "sub_par without sub_sib")
    for value in (33, -1):
        L = _small()
        L.path_len[1] = value
        assert _refused(L, "path_len above 32"), value
    for j, value in ((0, -1), (0, 8), (3, None)):
        L = _small()
        L.cand_ref[j] = L.cand_ref[j + 1] if value is None else value
        assert _refused(L, "cand_ref is no permutation"), (j, value)
    L = _small()
    L.ref_to_internal[2] = 8
    assert _refused(L, "ref_to_internal leaves")
    for value in (3, 0):
        L = _small()
        L.cand_slot[6] = value
        assert _refused(L, "cand_slot does not name"), value
    for slot0, n in ((1, 3), (3, 1), (-1, 2), (0, 0), (0, 4)):
        L = _small()
        L.slot0, L.n_slots = slot0, n
        assert _refused(L, "the launch window leaves the slot table"), (slot0, n)
    assert _refused(_small(), "n_parts must be n_slots", do_score=2, n_parts=2)
    assert _refused(_small(), "n_parts must be ceil(n_cand / 256)", do_argmax=1, n_parts=2, oblivious=1)
    assert _refused(_small(), "part_n needs part_s", do_score=2, with_n=True)
    assert _refused(_small(), "near-tie detection needs part_s", do_score=2, do_resolve=1, near=1)
    given = (np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32), None, None)
    for value in (8, -1, S.NO_CAND):                                 # (NO_CAND only beside a gain of -inf)
        given[1][1, 2] = value
        assert _refused(_small(), "a given part_i is no candidate", do_score=0, do_resolve=1, parts=given), value


def test_the_reference_on_a_case_small_enough_to_count_by_hand():
    """one node, D = 1: a numeric slot of three classes (S, n) = (1, 1), (2, 1), (3, 2) and a categorical slot of classes (1, 1), (5, 3):
    total (6, 4), parent 36 / 4"""
    L = S.make_level(0, 1, [(0, 2), (1, 1)], sbits=0)
    L.eff[0][0][:] = ((1, 1), (2, 1), (3, 2))
    L.eff[0][1][:] = ((1, 1), (5, 3))
    assert S.suffix_sums(S.obj(L.eff[0][0])).tolist() == [[6, 4], [5, 3], [3, 2]]
    R = S.reference_scores(L)
    assert [e[:2] for e in R.exact[0]] == [(1 * 3 + 25 * 1, 3), (9 * 2 + 9 * 2, 4), (1 * 3 + 25 * 1, 3)]
    assert R.scores[0].tolist() == [np.float32(28 / 3), 9.0, np.float32(28 / 3)] and R.parent[0] == 9.0
    L.cosine, L.sbits = 1, 3
    R = S.reference_scores(L)
    assert R.scores[0].tolist() == [np.float32(math.sqrt(28 / 3) / 8), 3 / 8, np.float32(math.sqrt(28 / 3) / 8)] and R.parent[0] == 3 / 8
    L.cosine, L.sbits, L.min_data = 0, 0, 2
    R = S.reference_scores(L)                                        # one row on a side: rejected
    assert R.scores[0].tolist() == [-np.inf, 9.0, -np.inf] and R.exact[0][0] is None
    L.min_data = 0
    S.set_path(L, 0, [(1, 0.0, 1), (0, float(L.thr[0, 1]), 0), (0, float(L.thr[0, 0]), 0)], length=2)
    R = S.reference_scores(L)                                        # the categorical class 1 and the threshold of candidate 1 are on the path; entry 2 is behind path_len
    assert R.scores[0].tolist() == [np.float32(28 / 3), -np.inf, -np.inf]
    assert R.cand_nr[0].tolist() == [0, 0, 0] and S.near_class(3, 1025) == 3 and S.near_class(1025, 1025) == 0 and S.near_class(3, 1024) == 0


def test_rounding_once_against_np_float32():
    # 1 + 2^-24 + 2^-60: above the tie, so the float32 is 1 + 2^-23; through float64 the 2^-60 is lost first and the tie goes to even, 1.0
    num, den = (1 << 60) + (1 << 36) + 1, 1 << 60
    assert S.f32_from_ratio(num, den)[0] == 1 + 2.0 ** -23 and np.float32(num / den) == 1.0
    assert S.f32_from_ratio(num, den << 7, 5)[0] == (1 + 2.0 ** -23) * 2.0 ** -12
    assert S.f32_from_ratio((1 << 60) + (1 << 36), den)[0] == 1.0 and S.f32_from_ratio((1 << 60) + 3 * (1 << 36), den)[0] == 1 + 2.0 ** -22      # ties to even
    assert S.f32_from_ratio((1 << 25) - 1, 1)[0] == 2.0 ** 25 and S.f32_from_ratio(3, 1 << 150)[0] == 2.0 ** -149 * 2 and S.f32_from_ratio(0, 5) == (0.0, -149)
    rng = np.random.default_rng(0)
    for _ in range(2000):                                            # a ratio that float64 holds exactly: np.float32 rounds it once
        n, sh = int(rng.integers(1, 1 << 53)), int(rng.integers(0, 80))
        assert S.f32_from_ratio(n, 1 << sh)[0] == float(np.float32(math.ldexp(n, -sh)))
    for _ in range(2000):                                            # the square root: the result's rounding interval holds the exact value
        n, d, sh = int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 40)), int(rng.integers(0, 41))
        r, q = S.f32_sqrt_ratio(n, d, sh)
        lo, hi = Fraction(r) - Fraction(2) ** q / 2, Fraction(r) + Fraction(2) ** q / 2
        assert lo * lo <= Fraction(n, d) / 4 ** sh <= hi * hi and r == math.ldexp(round(math.ldexp(r, -q)), q)
    assert S.f32_sqrt_ratio(49, 4, 1)[0] == 1.75
    # the fused multiply-add of the gain: 1 + 2^-23 times itself is 1 + 2^-22 + 2^-46; less 1 + 2^-22 it is 2^-46, where a product rounded to
    # float32 first leaves 0
    a, c = np.float32(1 + 2.0 ** -23), np.float32(-(1 + 2.0 ** -22))
    assert S.fma32(a, a, c)[()] == np.float32(2.0 ** -46) and np.float32(a * a) + c == 0
    x = Fraction(float(a)) * Fraction(float(np.float32(3.1))) - Fraction(float(np.float32(1e-30)))              # (the float64 sum is inexact: the Fraction path)
    assert S.fma32(a, np.float32(3.1), np.float32(-1e-30))[()] == np.float32(S.f32_from_fraction(x))
    assert S.fma32(np.float32(-np.inf), np.float32(0.7), np.float32(-3.0))[()] == -np.inf and S.fma32(np.float32(0), np.float32(0.7), np.float32(-0.0))[()] == 0


def _merge(a, b):
    """second_merge / better_takes_second of score_common.h on (gain, index, class, second) states"""
    (v1, i1, n1, s1), (v2, i2, n2, s2) = a, b
    s = max(s1, s2)
    if v1 == v2:
        if n1 != n2 and v1 > -np.inf:
            s = v1
    else:
        s = max(s, min(v1, v2))
    takes = v2 > v1 or (v2 == v1 and v2 > -np.inf and i2 < i1)
    return (v2, i2, n2, s) if takes else (v1, i1, n1, s)


def test_the_set_rule_equals_the_merge_steps_in_any_order():
    """the kernels reduce through four different trees; the rule they must all follow is S.select"""
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        gain = rng.choice(np.array([-np.inf, 0.0, 1.0, 1.0, 2.5, 2.5, 2.5], np.float32), size=n)
        cls = rng.integers(0, 3, size=n).astype(np.int32)
        ref = rng.permutation(n).astype(np.int32)
        want = S.select(gain, ref, cls)
        for order in range(4):
            states = [(float(gain[j]), int(ref[j]), int(cls[j]), -np.inf) if gain[j] > -np.inf else (-np.inf, S.NO_CAND, -1, -np.inf) for j in rng.permutation(n)]
            states.insert(int(rng.integers(0, len(states) + 1)), (-np.inf, S.NO_CAND, -1, -np.inf))          # a thread without candidates
            while len(states) > 1:                                    # merge two random neighbours, either way round
                q = int(rng.integers(0, len(states) - 1))
                a, b = states[q], states.pop(q + 1)
                states[q] = _merge(a, b) if rng.integers(0, 2) else _merge(b, a)
            v, i, c, s = states[0]
            assert (i, v, s) == (want[0], float(want[1]), float(want[2])), (trial, order)
            assert want[3] is None or c == want[3]


def test_a_score_one_ulp_off_and_a_suffix_sum_2_to_the_32_off_fail_the_comparison():
    for cosine in (0, 1):
        L = S.make_level(3, 3, [(0, 40), (1, 6)], nodes=(("acc",), ("acc",)), data="carry", sbits=20, cosine=cosine)
        R = S.reference_scores(L)
        assert S.score_failures(L, R.scores, R) == [] and S.parent_failures(L, R.parent, R) == []
        live = [(k, j) for k in range(2) for j in range(L.n_cand) if R.exact[k][j] is not None]
        assert len(live) > 40
        for k, j in live:
            got = R.scores.copy()
            above = S.exact_value(L, R.exact[k][j]) <= float(got[k, j])                                     # step away from the exact value
            got[k, j] = np.nextafter(got[k, j], np.float32(np.inf if above else -np.inf))
            assert S.score_failures(L, got, R) == [(k, j)]
        got = R.parent.copy()
        got[1] = np.nextafter(got[1], np.float32(np.inf if S.exact_value(L, R.parent_exact[1]) <= float(got[1]) else -np.inf))
        assert S.parent_failures(L, got, R) == [1]
        got = R.scores.copy()
        got[0, 3] = S.NEG_INF                                                                               # a live candidate rejected, a rejected one scored
        assert S.score_failures(L, got, R) == [(0, 3)]
        # a lost carry: one suffix sum 2^32 off changes that candidate's score
        for c, d, delta in ((1, 0, 1 << 32), (17, 2, -(1 << 32)), (40, 1, 1 << 32)):
            bad = S.reference_scores(L, suffix_fault=(1, 0, c, d, delta))
            assert S.score_failures(L, bad.scores, R) == [(1, c - 1)], (c, d)
            rel = abs(float(bad.scores[1, c - 1]) - float(R.scores[1, c - 1])) / float(R.scores[1, c - 1])
            assert rel >= 0.25 or cosine, rel
