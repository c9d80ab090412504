"""The parity mode of a model through the Python class and the C ABI, without a GPU (include/gbrl_hip.h, gbrl_hip_set_parity_mode).

Where the near-tie replay decides is a setting of the model: "default" | "reference" (+ a node-row limit) | "exact_argmax".  Here: the
setting itself -- defaults, round trips, the constructor keyword, errors, what a clone carries and what a saved file does not -- and the
refusal of "reference" on a row-sharded model, in both orders.  What the modes compute is tests/test_gpu_parity_mode.py."""
import ctypes as C

import numpy as np
import pytest

import cases as K
import gbrl_amd
from helpers import load_golden

MODES = ("default", "reference", "exact_argmax")
KW = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, split_score_func="L2", generator_type="Quantile", grow_policy="oblivious", device="cpu")


def _loaded(tmp_path, name="obl_l2_q"):
    _, g, _ = load_golden(name)
    p = tmp_path / (name + ".gbrl_model")
    p.write_bytes(g["model_file"].tobytes())
    return gbrl_amd.GBRL.load(str(p))


def test_default_is_default_everywhere(tmp_path):
    assert gbrl_amd.GBRL().get_parity_mode() == ("default", 0)
    assert gbrl_amd.GBRL(**KW).get_parity_mode() == ("default", 0)
    assert _loaded(tmp_path).get_parity_mode() == ("default", 0)


def test_setter_and_getter_round_trip():
    m = gbrl_amd.GBRL(**KW)
    for mode in MODES + MODES[::-1]:
        m.set_parity_mode(mode)
        assert m.get_parity_mode() == (mode, 0)
    m.set_parity_mode("reference", 65536)
    assert m.get_parity_mode() == ("reference", 65536)
    m.set_parity_mode(mode="reference", max_node_rows=7)
    assert m.get_parity_mode() == ("reference", 7)
    m.set_parity_mode("reference")                      # the limit's default is 0 = every node, not "keep the last one"
    assert m.get_parity_mode() == ("reference", 0)
    m.set_parity_mode("exact_argmax", 12)               # stored with every mode, read in "reference" only
    assert m.get_parity_mode() == ("exact_argmax", 12)


@pytest.mark.parametrize("mode", MODES)
def test_constructor_keyword(mode):
    assert gbrl_amd.GBRL(parity_mode=mode, **KW).get_parity_mode() == (mode, 0)
    assert gbrl_amd.GBRL(4, 2, 2, 3, 0, 256, 10, 0.9, "L2", "Quantile", False, 5000, "oblivious", 0, "cpu", "name", mode).get_parity_mode() == (mode, 0)


def test_positional_calls_of_the_reference_signature_are_unaffected():
    m = gbrl_amd.GBRL(4, 2, 2, 3, 0, 256, 10, 0.9, "L2", "Quantile", False, 5000, "oblivious", 0, "cpu", "name")
    assert m.get_parity_mode() == ("default", 0) and m.get_learner_name() == "name"
    assert "parity_mode" in gbrl_amd.GBRL.__init__.__doc__


def test_bad_arguments_raise_and_change_nothing():
    m = gbrl_amd.GBRL(**KW)
    m.set_parity_mode("reference", 5)
    for bad in ("Reference", "exact", "", "bit_exact"):
        with pytest.raises(RuntimeError, match="Invalid parity mode"):
            m.set_parity_mode(bad)
        with pytest.raises(RuntimeError, match="Invalid parity mode"):
            gbrl_amd.GBRL(parity_mode=bad, **KW)
    with pytest.raises(RuntimeError, match="max_node_rows"):
        m.set_parity_mode("reference", -1)
    with pytest.raises(RuntimeError, match="max_node_rows"):
        m.set_parity_mode("default", -65536)
    assert m.get_parity_mode() == ("reference", 5)


def test_copy_constructor_carries_mode_and_limit(tmp_path):
    m = gbrl_amd.GBRL(**KW)
    m.set_parity_mode("reference", 4096)
    c = gbrl_amd.GBRL(m)
    assert c.get_parity_mode() == ("reference", 4096)
    c.set_parity_mode("exact_argmax")                   # ... a copy, not a shared setting
    assert m.get_parity_mode() == ("reference", 4096) and gbrl_amd.GBRL(c).get_parity_mode() == ("exact_argmax", 0)
    assert gbrl_amd.GBRL(_loaded(tmp_path)).get_parity_mode() == ("default", 0)


@pytest.mark.parametrize("fresh", [True, False])
def test_model_file_does_not_carry_the_mode(fresh, tmp_path):
    """The file format is the reference's: the same bytes whatever the mode, and a loaded model is "default"."""
    def model():
        if not fresh:
            return _loaded(tmp_path, "grd_cos_q_ac")        # a model with trees
        m = gbrl_amd.GBRL(**KW)
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=2)
        return m
    files = {}
    for mode, limit in (("default", 0), ("reference", 0), ("reference", 65536), ("exact_argmax", 0)):
        m = model()
        m.set_parity_mode(mode, limit)
        p = tmp_path / ("%s_%d.gbrl_model" % (mode, limit))
        assert m.save(str(p)) == 0
        assert m.get_parity_mode() == (mode, limit)
        files[(mode, limit)] = p.read_bytes()
        assert gbrl_amd.GBRL.load(str(p)).get_parity_mode() == ("default", 0)
    for k, b in files.items():
        assert b == files[("default", 0)], k


# ---- the same through the C ABI ---------------------------------------------------------------------------------------------------------
class _Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "output_dim", "policy_dim", "max_depth", "min_data_in_leaf", "n_bins", "par_th")] + \
               [("cv_beta", C.c_float)] + \
               [(n, C.c_int32) for n in ("split_score_func", "generator_type", "use_control_variates", "batch_size", "grow_policy", "verbose", "device_ordinal")] + \
               [("learner_name", C.c_char_p)]


_REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


class _Collective(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("world_size", C.c_int), ("rank", C.c_int)] + [(n, _REDUCE) for n in ("sum_i64", "sum_f64", "max_f32", "min_f32")]


DEFAULT, REFERENCE, EXACT_ARGMAX = 0, 1, 2           # gbrl_hip_parity_mode
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture()
def lib():
    lib = C.CDLL(gbrl_amd.LIB_PATH)
    lib.gbrl_hip_create.restype = C.c_void_p
    lib.gbrl_hip_create.argtypes = [C.POINTER(_Config)]
    lib.gbrl_hip_clone.restype = C.c_void_p
    lib.gbrl_hip_clone.argtypes = [C.c_void_p]
    lib.gbrl_hip_load.restype = C.c_void_p
    lib.gbrl_hip_load.argtypes = [C.c_char_p]
    lib.gbrl_hip_save.argtypes = [C.c_void_p, C.c_char_p]
    lib.gbrl_hip_destroy.restype = None
    lib.gbrl_hip_destroy.argtypes = [C.c_void_p]
    lib.gbrl_hip_set_parity_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.gbrl_hip_get_parity_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.gbrl_hip_set_collective.argtypes = [C.c_void_p, C.c_void_p]
    lib.gbrl_hip_last_error.restype = C.c_char_p
    return lib


def _create(lib):
    cfg = _Config(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, min_data_in_leaf=0, n_bins=256, par_th=10, cv_beta=0.9, split_score_func=0,
                  generator_type=1, use_control_variates=0, batch_size=5000, grow_policy=1, verbose=0, device_ordinal=-1, learner_name=b"c")
    h = lib.gbrl_hip_create(C.byref(cfg))
    assert h, lib.gbrl_hip_last_error()
    return h


def _get(lib, h):
    mode, limit = C.c_int(-7), C.c_int(-7)
    assert lib.gbrl_hip_get_parity_mode(h, C.byref(mode), C.byref(limit)) == 0
    return mode.value, limit.value


def test_c_entry_points(lib, tmp_path):
    h = _create(lib)
    try:
        assert _get(lib, h) == (DEFAULT, 0)
        for mode, limit in ((REFERENCE, 0), (EXACT_ARGMAX, 0), (DEFAULT, 0), (REFERENCE, 65536)):
            assert lib.gbrl_hip_set_parity_mode(h, mode, limit) == 0, lib.gbrl_hip_last_error()
            assert _get(lib, h) == (mode, limit)
        for mode, limit, what in ((3, 0, b"parity mode"), (-1, 0, b"parity mode"), (REFERENCE, -1, b"max_node_rows"), (DEFAULT, -2, b"max_node_rows")):
            assert lib.gbrl_hip_set_parity_mode(h, mode, limit) == E_INVALID
            assert what in lib.gbrl_hip_last_error()
        assert _get(lib, h) == (REFERENCE, 65536)
        assert lib.gbrl_hip_set_parity_mode(None, REFERENCE, 0) == E_INVALID and lib.gbrl_hip_get_parity_mode(None, None, None) == E_INVALID
        only = C.c_int(-7)                                # either output pointer may be NULL
        assert lib.gbrl_hip_get_parity_mode(h, C.byref(only), None) == 0 and only.value == REFERENCE
        assert lib.gbrl_hip_get_parity_mode(h, None, C.byref(only)) == 0 and only.value == 65536
        c = lib.gbrl_hip_clone(h)
        assert c and _get(lib, c) == (REFERENCE, 65536)
        lib.gbrl_hip_destroy(c)
        p = str(tmp_path / "c.gbrl_model").encode()
        assert lib.gbrl_hip_save(h, p) == 0
        ld = lib.gbrl_hip_load(p)
        assert ld and _get(lib, ld) == (DEFAULT, 0)
        lib.gbrl_hip_destroy(ld)
        reference_bytes = open(p, "rb").read()
        assert lib.gbrl_hip_set_parity_mode(h, DEFAULT, 0) == 0 and lib.gbrl_hip_save(h, p) == 0
        assert open(p, "rb").read() == reference_bytes
    finally:
        lib.gbrl_hip_destroy(h)


def test_reference_and_row_sharding_exclude_each_other(lib):
    """Installing hooks stores them; nothing is called before a step.  World size 2: a row-sharded model."""
    never = _REDUCE(lambda ctx, buf, n: 1)
    coll = _Collective(None, 2, 0, never, never, never, never)
    h = _create(lib)
    try:
        assert lib.gbrl_hip_set_parity_mode(h, REFERENCE, 0) == 0
        assert lib.gbrl_hip_set_collective(h, C.byref(coll)) == E_UNSUPPORTED          # hooks after "reference"
        msg = lib.gbrl_hip_last_error()
        assert b"row-sharded" in msg and b"exact arg-max" in msg, msg
        assert _get(lib, h) == (REFERENCE, 0)
        assert lib.gbrl_hip_set_collective(h, None) == 0                                # (uninstalling is always fine)
        for mode in (DEFAULT, EXACT_ARGMAX):
            assert lib.gbrl_hip_set_parity_mode(h, mode, 0) == 0
            assert lib.gbrl_hip_set_collective(h, C.byref(coll)) == 0, lib.gbrl_hip_last_error()
            assert lib.gbrl_hip_set_parity_mode(h, REFERENCE, 0) == E_UNSUPPORTED      # "reference" after hooks
            msg = lib.gbrl_hip_last_error()
            assert b"row-sharded" in msg and b"exact arg-max" in msg, msg
            assert _get(lib, h) == (mode, 0)
            assert lib.gbrl_hip_set_parity_mode(h, DEFAULT, 3) == 0 and lib.gbrl_hip_set_parity_mode(h, EXACT_ARGMAX, 0) == 0   # both accepted sharded
            c = lib.gbrl_hip_clone(h)                                                   # a clone has no hooks: it may be "reference"
            assert c and lib.gbrl_hip_set_parity_mode(c, REFERENCE, 0) == 0
            lib.gbrl_hip_destroy(c)
            assert lib.gbrl_hip_set_collective(h, None) == 0
        assert lib.gbrl_hip_set_parity_mode(h, REFERENCE, 0) == 0                       # single-GPU again
    finally:
        lib.gbrl_hip_destroy(h)


def test_header_declares_a_plain_c_enum(tmp_path):
    """A C99 program names the three modes and calls both entry points."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "p.c"
    src.write_text('#include "gbrl_hip.h"\n#include <string.h>\nint main(void) {\n'
                   '  gbrl_hip_config c; int mode = -1, rows = -1; gbrl_hip_parity_mode want = GBRL_HIP_PARITY_REFERENCE; gbrl_hip_model *m;\n'
                   '  memset(&c, 0, sizeof c); c.input_dim = 2; c.output_dim = 1; c.policy_dim = 1; c.max_depth = 2; c.n_bins = 8; c.device_ordinal = -1; c.learner_name = "c";\n'
                   '  m = gbrl_hip_create(&c);\n'
                   '  if (!m || GBRL_HIP_PARITY_DEFAULT != 0 || GBRL_HIP_PARITY_EXACT_ARGMAX != 2) return 1;\n'
                   '  if (gbrl_hip_set_parity_mode(m, want, 9) != GBRL_HIP_OK || gbrl_hip_get_parity_mode(m, &mode, &rows) != GBRL_HIP_OK) return 2;\n'
                   '  if (mode != GBRL_HIP_PARITY_REFERENCE || rows != 9) return 3;\n'
                   '  if (gbrl_hip_set_parity_mode(m, 7, 0) != GBRL_HIP_E_INVALID || !strstr(gbrl_hip_last_error(), "parity mode")) return 4;\n'
                   '  gbrl_hip_destroy(m); return 0; }\n')
    exe = tmp_path / "p"
    libdir = os.path.dirname(gbrl_amd.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), str(src), "-L", libdir, "-lgbrl_hip",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
