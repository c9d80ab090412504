"""The parity mode of a model on the GPU (include/gbrl_hip.h, gbrl_hip_set_parity_mode): where the near-tie replay decides.

A mode is defined by the environment hook it replaces, so every comparison here is byte equality of the whole ensemble against a run of an
unconfigured model under that hook -- "reference" = GBRL_HIP_NEARTIE_MAX_ROWS=<limit>, "exact_argmax" = GBRL_HIP_NO_NEARTIE_REPLAY=1,
"default" = neither -- or bit equality of the tree structure against a fixture written by the reference build.  The specimens are the
committed near-ties of tests/test_gpu_neartie.py: two above 65 536 rows (bign30: the deciding node has at most 65 536 rows; bign9: an
oblivious level of larger nodes) and the 3 000-row one of the golden cases.  What the environment cannot express is here too: two models of
one process in different modes, a clone that keeps its mode, a hook that still overrides the model, and the refusal of "reference" where no
replay exists (row-sharded models; the two opt-in loops without a replay)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases as K
from helpers import load_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = ("GBRL_HIP_NO_NEARTIE_REPLAY", "GBRL_HIP_NEARTIE_MAX_ROWS", "GBRL_HIP_NO_SMALL_GROW", "GBRL_HIP_NO_SMALL_PREP", "GBRL_HIP_NEARTIE_REL",
         "GBRL_HIP_NEARTIE_SERIAL", "GBRL_HIP_DEVICE_LEVELS", "GBRL_HIP_EVENT_RESULTS", "GBRL_HIP_FORCE_COLLECTIVE")
STRUCTURE = ("tree_indices", "depths", "feature_indices", "inequality_directions")


def _env(monkeypatch, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _arrays(m):
    return {k: np.asarray(v) for k, v in m.get_ensemble_data().items() if isinstance(v, np.ndarray)}


def _same_bytes(a, b):
    assert set(a) == set(b)
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def _model(case, mode=None, limit=0, via="setter"):
    import gbrl_amd
    if mode is None:
        return gbrl_amd.GBRL(**K.ctor_kwargs(case))               # nobody configures it
    if via == "ctor":
        assert limit == 0
        return gbrl_amd.GBRL(parity_mode=mode, **K.ctor_kwargs(case))
    m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
    m.set_parity_mode(mode, limit)
    return m


# ---- above 65 536 rows ------------------------------------------------------------------------------------------------------------------
_BIG = {}      # name -> (case, inputs, the reference's tree); runs: (name, how) -> (ensemble arrays, counters)


def _big(name):
    if name not in _BIG:
        fx = np.load(os.path.join(HERE, "golden", name + ".npz"))
        case = json.loads(str(fx["case_json"]))
        X, Xc, G, y = K.make_inputs(case)
        assert K.inputs_digest(X, Xc, G, y) == str(fx["inputs_sha256"])
        _BIG[name] = (case, (X, G), {k: fx[k] for k in fx.files})
    return _BIG[name]


def _is_reference_tree(name, e):
    ref = _big(name)[2]
    return all(np.array_equal(e[k], ref[k]) for k in STRUCTURE) and np.array_equal(e["feature_values"].view(np.uint32), ref["feature_values"].view(np.uint32))


def _big_run(name, monkeypatch, env=None, mode=None, limit=0, via="setter", model=None):
    """One tree of the specimen; memoised (the inputs, the hooks and the setting determine the bytes).  Returns (arrays, counters)."""
    key = (name, tuple(sorted((env or {}).items())), mode, limit, via)
    if model is None and key in _BIG:
        return _BIG[key]
    case, (X, G), _ = _big(name)
    _env(monkeypatch, env or {})
    m = model if model is not None else _model(case, mode, limit, via)
    m.set_profiling(2)
    K.drive(m, case, X, None, G, None)
    out = (_arrays(m), dict(m.last_phase_times()))
    _env(monkeypatch, {})
    if model is None:
        _BIG[key] = out
    return out


@pytest.mark.parametrize("name,small_node", [("bign30", True), ("bign9", False)])
def test_reference_mode_is_the_hook_above_65536_rows(name, small_node, monkeypatch):
    hook_all, _ = _big_run(name, monkeypatch, env={"GBRL_HIP_NEARTIE_MAX_ROWS": "0"})
    hook_none, _ = _big_run(name, monkeypatch)
    hook_64k, _ = _big_run(name, monkeypatch, env={"GBRL_HIP_NEARTIE_MAX_ROWS": "65536"})
    assert _is_reference_tree(name, hook_all) and not _is_reference_tree(name, hook_none)      # (what the specimens were chosen for)
    # "reference": the reference's tree, the bytes of GBRL_HIP_NEARTIE_MAX_ROWS=0; levels were replayed
    ref_mode, ref_counters = _big_run(name, monkeypatch, mode="reference")
    assert _is_reference_tree(name, ref_mode)
    assert _same_bytes(ref_mode, hook_all)
    assert ref_counters["near_replays"] > 0
    # "default", set explicitly: not the reference's tree, the bytes of a run with no variable set; nothing was replayed
    def_mode, def_counters = _big_run(name, monkeypatch, mode="default")
    assert not _is_reference_tree(name, def_mode)
    assert _same_bytes(def_mode, hook_none)
    assert def_counters["near_replays"] == 0
    # "reference" with a node-row limit: the reference's tree exactly where the deciding node is that small; the bytes of the hook
    lim_mode, _ = _big_run(name, monkeypatch, mode="reference", limit=65536)
    assert _is_reference_tree(name, lim_mode) == small_node
    assert _same_bytes(lim_mode, hook_64k)
    # the constructor keyword is the setter
    ctor_mode, ctor_counters = _big_run(name, monkeypatch, mode="reference", via="ctor")
    assert _same_bytes(ctor_mode, ref_mode) and ctor_counters["near_replays"] > 0


def test_a_set_hook_overrides_the_model(monkeypatch):
    """GBRL_HIP_NO_NEARTIE_REPLAY=1 wins over "reference" (the exact arg-max's bytes); GBRL_HIP_NEARTIE_MAX_ROWS wins over the model's limit
    and over "default" / "exact_argmax" for these batches, as it did before the setting existed."""
    hook_none, _ = _big_run("bign30", monkeypatch)
    hook_all, _ = _big_run("bign30", monkeypatch, env={"GBRL_HIP_NEARTIE_MAX_ROWS": "0"})
    e, counters = _big_run("bign30", monkeypatch, env={"GBRL_HIP_NO_NEARTIE_REPLAY": "1"}, mode="reference")
    assert _same_bytes(e, hook_none) and counters["near_replays"] == 0
    e, _ = _big_run("bign30", monkeypatch, env={"GBRL_HIP_NEARTIE_MAX_ROWS": "0"}, mode="exact_argmax")
    assert _same_bytes(e, hook_all)
    hook_tiny, _ = _big_run("bign30", monkeypatch, env={"GBRL_HIP_NEARTIE_MAX_ROWS": "1000"})      # (smaller than the deciding node: the specimens' are of 4 553 rows and up)
    assert not _is_reference_tree("bign30", hook_tiny)
    e, _ = _big_run("bign30", monkeypatch, env={"GBRL_HIP_NEARTIE_MAX_ROWS": "1000"}, mode="reference", limit=0)
    assert _same_bytes(e, hook_tiny)


def test_two_models_of_one_process_keep_their_own_modes(monkeypatch):
    """Stepped alternately on the same batch, twice each: the "reference" model grows the reference's tree both times, the "default" model the
    exact arg-max's.  (The gradients are given, so a model's second tree is its first one again.)"""
    case, (X, G), _ = _big("bign30")
    one_ref, _ = _big_run("bign30", monkeypatch, mode="reference")
    one_def, _ = _big_run("bign30", monkeypatch, mode="default")
    _env(monkeypatch, {})
    a, b = _model(case, "reference"), _model(case)
    in_dim = case["F"]
    for m in (a, b):
        m.set_feature_weights(np.ones(in_dim, np.float32))
        for o in K.optimizers(case):
            m.set_optimizer(**o)
        m.set_feature_mapping(np.arange(in_dim, dtype=np.int32), np.ones(in_dim, dtype=bool))
    for m in (a, b, b, a):
        m.step(X, None, np.ascontiguousarray(G.copy()))
    for m, one, is_ref in ((a, one_ref, True), (b, one_def, False)):
        e = _arrays(m)
        assert m.get_num_trees() == 2
        for k in STRUCTURE[1:] + ("feature_values", "values", "edge_weights"):
            assert e[k].tobytes() == np.concatenate([one[k], one[k]]).tobytes(), (is_ref, k)
        assert _is_reference_tree("bign30", one) == is_ref


def test_a_clone_keeps_the_mode(monkeypatch):
    import gbrl_amd
    case, _, _ = _big("bign30")
    _env(monkeypatch, {})
    m = _model(case, "reference")
    c = gbrl_amd.GBRL(m)
    del m
    assert c.get_parity_mode() == ("reference", 0)
    e, counters = _big_run("bign30", monkeypatch, model=c)
    assert _is_reference_tree("bign30", e) and counters["near_replays"] > 0
    assert _same_bytes(e, _big_run("bign30", monkeypatch, mode="reference")[0])


# ---- a small batch: the modes differ the other way round (the default replays) -------------------------------------------------------------
@pytest.mark.parametrize("no_small_grow", [False, True])
def test_exact_argmax_mode_is_the_hook_on_a_small_batch(no_small_grow, monkeypatch):
    """The golden near-tie specimen, through the one-launch growth kernel and (GBRL_HIP_NO_SMALL_GROW=1) through the level loop."""
    import neartie
    case, g, inputs = load_golden("grd_cos_q_ac_d6_neartie")
    path = {"GBRL_HIP_NO_SMALL_GROW": "1"} if no_small_grow else {}

    def grow(env, mode, via="setter"):
        _env(monkeypatch, dict(path, **env))
        m = _model(case, mode, 0, via)
        pred = np.asarray(K.drive(m, case, *inputs))
        _env(monkeypatch, {})
        return dict(_arrays(m), pred=pred)

    e_default = grow({}, None)
    e_hook = grow({"GBRL_HIP_NO_NEARTIE_REPLAY": "1"}, None)
    e_mode = grow({}, "exact_argmax")
    assert _same_bytes(e_mode, e_hook)
    assert _same_bytes(grow({}, "exact_argmax", via="ctor"), e_hook)
    assert neartie.first_mismatch(g, e_default, case["policy"]) is None, "the default replays this batch: the fixture's tree"
    assert neartie.first_mismatch(g, e_mode, case["policy"]) is not None and not _same_bytes(e_mode, e_default)
    # "reference" and an explicit "default" are the default here, with or without a node-row limit (the limit is for batches above 65 536 rows)
    for mode, limit in (("default", 0), ("reference", 0), ("reference", 100)):
        _env(monkeypatch, path)
        m = _model(case, mode, limit)
        pred = np.asarray(K.drive(m, case, *inputs))
        _env(monkeypatch, {})
        assert _same_bytes(dict(_arrays(m), pred=pred), e_default), (mode, limit)
    # the hook wins over "reference" and "default"
    assert _same_bytes(grow({"GBRL_HIP_NO_NEARTIE_REPLAY": "1"}, "reference"), e_hook)


def test_fit_honours_the_mode(monkeypatch):
    case, g, (X, Xc, G, y) = load_golden("fit_grd_cos_u")
    out = []
    for env, mode in (({"GBRL_HIP_NO_NEARTIE_REPLAY": "1"}, None), ({}, "exact_argmax")):
        _env(monkeypatch, env)
        m = _model(case, mode)
        loss, pred = K.drive_fit(m, case, X, y, Xc)
        _env(monkeypatch, {})
        out.append(dict(_arrays(m), pred=pred, loss=np.float32(loss), bias=np.asarray(m.get_bias())))
    assert out[0]["tree_indices"].size > 0
    assert _same_bytes(out[1], out[0])


# ---- where no replay exists, "reference" is refused, not ignored ---------------------------------------------------------------------------
@pytest.mark.parametrize("hook", ["GBRL_HIP_DEVICE_LEVELS", "GBRL_HIP_EVENT_RESULTS"])
def test_reference_mode_refuses_the_loops_without_a_replay(hook, monkeypatch):
    """The opt-in device-planned oblivious loop and the copy-engine read-back have no replay: in "reference" mode the step raises and leaves
    the model as it was; the other modes run as before, and so does "reference" once the hook is gone."""
    case, g, (X, Xc, G, y) = load_golden("obl_l2_q_d6")
    _env(monkeypatch, {hook: "1"})
    m = _model(case, "reference")
    with pytest.raises(RuntimeError, match=hook):
        K.drive(m, case, X, Xc, G, y)
    assert m.get_num_trees() == 0 and m.get_parity_mode() == ("reference", 0)
    plain = _model(case)
    K.drive(plain, case, X, Xc, G, y)                                # (an unconfigured model under the hook: as before)
    assert plain.get_num_trees() == case["trees"]
    _env(monkeypatch, {})
    again = _model(case, "reference")
    K.drive(again, case, X, Xc, G, y)
    unconfigured = _model(case)
    K.drive(unconfigured, case, X, Xc, G, y)
    assert _same_bytes(_arrays(again), _arrays(unconfigured))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


def test_row_sharded_models_refuse_reference_and_hold_the_exact_argmax(monkeypatch, tmp_path):
    """One rank whose collective hooks stay installed (tests/parity_mode_sharded_worker.py): "reference" is refused in both orders with a message
    that says what row-sharded runs hold; "exact_argmax" and "default" are accepted, the step runs through the hooks, and on the near-tie
    specimen both grow the bytes of a ONE-GPU model in "exact_argmax" mode -- not those of the one-GPU default (include/gbrl_hip.h, the
    qualifier at gbrl_hip_collective)."""
    name = "grd_cos_q_ac_d6_neartie"
    case, g, inputs = load_golden(name)
    _env(monkeypatch, {})
    env = dict(os.environ, GBRL_HIP_FORCE_COLLECTIVE="1")
    out = str(tmp_path / "sharded.npz")
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "parity_mode_sharded_worker.py"), _free_port(), name, out],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    d = np.load(out)
    for msg in (str(d["set_after_install"]), str(d["install_after_set"])):
        assert "row-sharded" in msg and "exact arg-max" in msg, msg
    assert str(d["mode_after_refusal"]) == "default"
    one_gpu = {}
    for mode in ("exact_argmax", "default"):
        m = _model(case, mode)
        pred = np.asarray(K.drive(m, case, *inputs))
        one_gpu[mode] = dict({k: v for k, v in _arrays(m).items() if k in K.ENSEMBLE_KEYS}, pred=pred)
    assert not _same_bytes(one_gpu["exact_argmax"], one_gpu["default"])
    for mode in ("exact_argmax", "default"):
        assert str(d[mode + "/mode"]) == mode and int(d[mode + "/calls"]) > 0
        sharded = dict({k: d[mode + "/" + k] for k in K.ENSEMBLE_KEYS}, pred=d[mode + "/pred"])
        assert _same_bytes(sharded, one_gpu["exact_argmax"]), mode
