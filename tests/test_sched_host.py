"""CPU-side checks of the Linear learning-rate scheduler (scheduler.h:124-134): the optimizer surface, the schedule's values against
recordings of the reference, the .gbrl_model record (scheduler.cpp:64-75) and the exported header (types.cpp:596-625).  The fixtures were
written by the reference's CPU build (tests/golden/make_sched_golden.py)."""
import os

import numpy as np
import pytest

import cases as K
import gbrl_amd
import sched_cases as S
from helpers import GOLDEN, load_golden as load_const_golden

REC = os.path.join(GOLDEN, "sched_recordings.npz")


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = S.BY_NAME[name]
    X, Xc, G, y = K.make_inputs(case)
    assert K.inputs_digest(X, Xc, G, y) == str(g["inputs_sha256"]), "input synthesis drifted from the fixture"
    return case, g, (X, Xc, G, y)


def _mask_header_padding(b):
    b = bytearray(b)
    b[6:8] = b"\0\0"        # serializationHeader padding after the three u16 (uninitialised in the reference)
    b[20:24] = b"\0\0\0\0"  # ... and after reserved2
    return bytes(b)


def _model(**kw):
    base = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile",
                grow_policy="oblivious", device="cpu")
    base.update(kw)
    return gbrl_amd.GBRL(**base)


def test_linear_is_accepted_and_adam_and_bad_T_are_refused():
    m = _model()
    m.set_optimizer(algo="SGD", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=1, stop_lr=0.01, T=100)
    m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.02, start_idx=1, stop_idx=2)
    o = m.get_optimizers()
    assert len(o) == 2
    assert o[0]["algo"] == "SGD" and o[0]["scheduler_func"] == "Linear" and o[0]["T"] == 100
    assert o[0]["init_lr"] == np.float32(0.1) and o[0]["stop_lr"] == np.float32(0.01)
    assert (o[0]["start_idx"], o[0]["stop_idx"]) == (0, 1)
    assert o[1]["scheduler_func"] == "Const" and o[1]["init_lr"] == np.float32(0.02)
    for bad_T in (0, -5):
        with pytest.raises(RuntimeError):
            _model().set_optimizer(algo="SGD", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=2, stop_lr=0.01, T=bad_T)
    with pytest.raises(RuntimeError):
        _model().set_optimizer(algo="Adam", scheduler="Linear", init_lr=0.1, start_idx=0, stop_idx=2, stop_lr=0.01, T=10)
    with pytest.raises(RuntimeError):
        _model().set_optimizer(algo="Adam", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2)
    m2 = gbrl_amd.GBRL(m)       # the copy constructor carries the schedule
    assert m2.get_optimizers() == o


def _schedule(o, t):
    """scheduler.h:124-134 restated in float32."""
    if o["scheduler"] != "Linear":
        return np.float32(o["init_lr"])
    f = np.float32
    T_, t_ = f(o["T"]), f(t) + f(1)
    pr = f((T_ - t_) / T_)
    lr = f(f(o["init_lr"]) + f(f(f(1) - pr) * f(f(o["stop_lr"]) - f(o["init_lr"]))))
    return f(o["stop_lr"]) if lr < f(o["stop_lr"]) else lr


def _file_with(ref_bytes, n_trees, opts):
    """The reference's file of the oblivious golden `sched_obl_l2_q`, cut down to its first n_trees trees and given the optimizer records
    `opts` (layout: model.cpp Model::save): a host-only way to a model with a chosen tree count and schedule."""
    import struct
    b = ref_bytes
    meta = np.frombuffer(b[24:104], np.int32).copy()
    L, T, inp, D, md = int(meta[0]), int(meta[1]), int(meta[6]), int(meta[7]), int(meta[9])
    pos = 24 + 80 + 2
    name_len = struct.unpack_from("<Q", b, pos)[0]
    pos += 8 + name_len
    head = b[24 + 80:pos]
    ti = np.frombuffer(b, np.int32, T, pos + 1 + (D + inp) * 4 + 2)
    assert ti[0] == 0 and n_trees <= T
    L2 = L if n_trees == T else int(ti[n_trees])
    # (elements per unit, bytes per element, unit: 'D' = fixed, 'T' = per tree, 'L' = per leaf)
    arrays = [(D, 4, "D"), (inp, 4, "D"), (1, 4, "T"), (1, 4, "T"), (D, 4, "L"), (md, 4, "T"), (md, 4, "T"), (md, 4, "L"), (inp, 4, "D"), (inp, 4, "D"),
              (inp, 4, "D"), (inp, 1, "D"), (md, 1, "T"), (md, 1, "L"), (md * 128, 1, "T")]
    out = bytearray()
    for per, size, unit in arrays:
        assert b[pos] == 1
        old_n = per * {"D": 1, "T": T, "L": L}[unit]
        new_n = per * {"D": 1, "T": n_trees, "L": L2}[unit]
        out += b[pos:pos + 1 + new_n * size]
        pos += 1 + old_n * size
    meta[0], meta[1] = L2, n_trees
    tail = struct.pack("<i", len(opts))
    for o in opts:
        tail += struct.pack("<Bii", 0, o["start_idx"], o["stop_idx"])
        if o["scheduler"] == "Linear":
            tail += struct.pack("<Bffi", 1, o["init_lr"], o["stop_lr"], o["T"])
        else:
            tail += struct.pack("<Bf", 0, o["init_lr"])
    return b[:24] + meta.tobytes() + head + bytes(out) + tail


def test_the_cut_down_file_is_the_original_at_full_length():
    case, g, _ = load_golden("sched_obl_l2_q")
    ref = g["model_file"].tobytes()
    assert _file_with(ref, int(g["n_trees"]), case["opts"]) == ref


@pytest.mark.parametrize("name", sorted(S.LRS_SCHEDULES))
def test_get_scheduler_lrs_equals_the_recorded_reference_values(name, tmp_path):
    """get_scheduler_lrs() = get_lr(n_trees) per optimizer (gbrl.cpp:527-539) at 0 .. 14 trees, against the reference's recorded values
    at every tree count.  No GPU here, so the trees come from a file: the first t trees of a golden ensemble with this schedule's
    optimizer records (the schedule only reads the tree count)."""
    want = np.load(REC)["lrs_" + name]
    opts = S.LRS_SCHEDULES[name]
    assert want.shape == (S.LRS_TREES + 1, len(opts))
    _, g, _ = load_golden("sched_obl_l2_q")
    ref = g["model_file"].tobytes()
    for t in range(S.LRS_TREES + 1):
        p = tmp_path / ("t%d.gbrl_model" % t)
        p.write_bytes(_file_with(ref, t, opts))
        m = gbrl_amd.GBRL.load(str(p))
        assert m.get_num_trees() == t and len(m.get_optimizers()) == len(opts)
        got = np.asarray(m.get_scheduler_lrs(), np.float32)
        assert got.shape == (len(opts),)
        assert np.all(np.abs(got - want[t]) <= 1e-6 * np.abs(want[t])), (t, got, want[t])
        # the formula of scheduler.h:124-134, restated above, says the same
        for i, o in enumerate(opts):
            assert abs(float(_schedule(o, t)) - float(want[t, i])) <= 1e-6 * abs(float(want[t, i]))
    m = gbrl_amd.GBRL(**S.LRS_KW)      # ... and a model constructed here, before its first tree
    for o in opts:
        m.set_optimizer(**o)
    got0 = np.asarray(m.get_scheduler_lrs(), np.float32)
    assert np.all(np.abs(got0 - want[0]) <= 1e-6 * np.abs(want[0])), (got0, want[0])


@pytest.mark.parametrize("name", S.MODEL_FILE_CASES)
def test_scheduler_lrs_of_a_loaded_ensemble(name, tmp_path):
    """... and at the tree count of the golden ensembles, loaded from the reference's file: the reference's own get_scheduler_lrs()."""
    case, g, _ = load_golden(name)
    p = tmp_path / "ref.gbrl_model"
    p.write_bytes(g["model_file"].tobytes())
    m = gbrl_amd.GBRL.load(str(p))
    got, want = np.asarray(m.get_scheduler_lrs(), np.float32), g["scheduler_lrs"]
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (got, want)


@pytest.mark.parametrize("name", S.MODEL_FILE_CASES)
def test_linear_model_file_roundtrip_is_byte_compatible(name, tmp_path):
    case, g, _ = load_golden(name)
    ref_bytes = g["model_file"].tobytes()
    p = tmp_path / "ref.gbrl_model"
    p.write_bytes(ref_bytes)
    m = gbrl_amd.GBRL.load(str(p))            # a Linear file written by the reference loads ...
    e = m.get_ensemble_data()
    for k in K.ENSEMBLE_KEYS:
        assert np.array_equal(np.asarray(e[k]), g[k]), k
    assert m.get_num_trees() == int(g["n_trees"]) and m.get_iteration() == int(g["iteration"])
    assert m.get_learner_name() == case["name"]
    got = m.get_optimizers()
    assert len(got) == len(case["opts"])
    for o, w in zip(got, case["opts"]):
        assert o["scheduler_func"] == w["scheduler"] and o["init_lr"] == np.float32(w["init_lr"])
        assert (o["start_idx"], o["stop_idx"]) == (w["start_idx"], w["stop_idx"])
        if w["scheduler"] == "Linear":
            assert o["stop_lr"] == np.float32(w["stop_lr"]) and o["T"] == w["T"]
    q = tmp_path / "ours.gbrl_model"
    assert m.save(str(q)) == 0                # ... and what we write back is the same file
    assert _mask_header_padding(q.read_bytes()) == _mask_header_padding(ref_bytes)
    r = tmp_path / "copy.gbrl_model"
    assert gbrl_amd.GBRL(m).save(str(r)) == 0
    assert r.read_bytes() == q.read_bytes()


def test_fresh_linear_model_file_is_the_file_the_reference_writes(tmp_path):
    m = gbrl_amd.GBRL(**S.FRESH_KW)
    for o in S.FRESH_OPTS:
        m.set_optimizer(**o)
    p = tmp_path / "fresh.gbrl_model"
    assert m.save(str(p)) == 0
    theirs = np.load(REC)["fresh_model_file"].tobytes()
    assert _mask_header_padding(p.read_bytes()) == _mask_header_padding(theirs)


def test_a_file_with_T_zero_is_refused(tmp_path):
    """The Linear record ends the file (type u8, init_lr f32, stop_lr f32, T i32 of the LAST optimizer when it is Linear)."""
    case, g, _ = load_golden("sched_obl_l2_q")
    b = bytearray(g["model_file"].tobytes())
    assert int(np.frombuffer(bytes(b[-4:]), np.int32)[0]) == case["opts"][-1]["T"]
    b[-4:] = np.int32(0).tobytes()
    p = tmp_path / "t0.gbrl_model"
    p.write_bytes(bytes(b))
    with pytest.raises(RuntimeError):
        gbrl_amd.GBRL.load(str(p))


@pytest.mark.parametrize("name", sorted(S.EXPORT_CASES))
def test_exported_header_equals_the_reference_text(name, tmp_path):
    case, g, _ = load_golden(name)
    p = tmp_path / "ref.gbrl_model"
    p.write_bytes(g["model_file"].tobytes())
    m = gbrl_amd.GBRL.load(str(p))
    modelname, fmt, typ, prefix = S.EXPORT_CASES[name]
    h = tmp_path / "m.h"
    m.export(str(h), modelname, fmt, typ, prefix)
    assert h.read_bytes() == g["export_text"].tobytes()


def test_a_const_only_model_still_writes_the_same_bytes(tmp_path):
    case, g, _ = load_const_golden("grd_cos_q_ac")
    p = tmp_path / "ref.gbrl_model"
    p.write_bytes(g["model_file"].tobytes())
    q = tmp_path / "ours.gbrl_model"
    assert gbrl_amd.GBRL.load(str(p)).save(str(q)) == 0
    assert _mask_header_padding(q.read_bytes()) == _mask_header_padding(g["model_file"].tobytes())
