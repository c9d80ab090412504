"""Shared assertions for the parity tests."""
import os

import numpy as np

import cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

STRUCTURE_KEYS = ("tree_indices", "depths", "feature_indices", "feature_values", "is_numerics",
                  "inequality_directions", "categorical_values")
VALUE_KEYS = ("values", "edge_weights")


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = K.BY_NAME[name]
    X, Xc, G, y = K.make_inputs(case)
    assert K.inputs_digest(X, Xc, G, y) == str(g["inputs_sha256"]), "input synthesis drifted from the fixture"
    return case, g, (X, Xc, G, y)


def assert_structure_equal(e, g, what=""):
    """Tree structure must be BIT-identical (split feature / threshold bits / directions / layout)."""
    for k in STRUCTURE_KEYS:
        a, b = np.asarray(e[k]), np.asarray(g[k])
        assert a.shape == b.shape, f"{what}{k}: shape {a.shape} != {b.shape}"
        if a.dtype.kind == "f":
            # Signed zeros are canonicalised on both sides: -0.0 and +0.0 are ONE order statistic (they compare equal), the
            # reference stores whichever of the two its std::sort happens to leave at the rank, the product stores +0.0; no
            # comparison `x > t` the model ever makes can tell them apart.  Every other threshold must match bit for bit.
            a = (a.astype(np.float32) + np.float32(0.0)).astype(np.float32)
            b = (b.astype(np.float32) + np.float32(0.0)).astype(np.float32)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                f"{what}{k}: threshold bits differ at {np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:5].tolist()}"
        else:
            assert np.array_equal(a, b), f"{what}{k}: differs at {np.argwhere(a != b)[:5].tolist()}"


def rel_err(a, b, scale):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), scale))) if a.size else 0.0


def assert_values_close(e, g, grad_scale, tol=1e-5, what=""):
    """Leaf values within `tol` relative: |a-b| <= tol * max(|b|, grad_scale) (north_star: 1e-5; SURVEY.md
    hard part 5 for why the floor is the gradient scale)."""
    for k in VALUE_KEYS:
        a, b = np.asarray(e[k]), np.asarray(g[k])
        assert a.shape == b.shape, f"{what}{k}: shape {a.shape} != {b.shape}"
        err = rel_err(a, b, grad_scale if k == "values" else 1.0)
        assert err <= tol, f"{what}{k}: rel err {err:.3g} > {tol}"


# ---- the reference build's outputs without the reference build ---------------------------------------------------------------------------
# Tests that compare with oracle/_ref (the reference's own CPU path, built by oracle/Makefile only where the reference's sources are) call it
# live when it is built and otherwise read what it returned for the same inputs from tests/golden/ref_recordings.npz.  The recording is
# written by tests/golden/make_ref_recordings.py, which runs those tests against the live build with GBRL_RECORD_REF=<dir> set: every
# process then writes what the reference returned to <dir>/<pid>.npz at exit, and the script merges the files.
REF_RECORDINGS = os.path.join(GOLDEN, "ref_recordings.npz")
_recorded = None
_to_record = {}


def _recording():
    global _recorded
    if _recorded is None:
        assert os.path.exists(REF_RECORDINGS), "oracle/_ref is not built and " + REF_RECORDINGS + " is missing"
        with np.load(REF_RECORDINGS) as f:
            _recorded = {k: f[k] for k in f.files}
    return _recorded


def _save_recording():
    d = os.environ.get("GBRL_RECORD_REF")
    if d and _to_record:
        os.makedirs(d, exist_ok=True)
        np.savez(os.path.join(d, "%d.npz" % os.getpid()), **_to_record)


def _live_ref():
    import oracle
    return oracle.load_ref()


def ref_arrays(key, compute):
    """compute(ref_module) -> {name: array} from the live reference build, or the recorded arrays under `key`."""
    ref = _live_ref()
    if ref is None:
        rec = _recording()
        out = {k.split("::", 1)[1]: v for k, v in rec.items() if k.startswith(key + "::")}
        assert out, "no recording of the reference for " + key
        return out
    out = {k: np.asarray(v) for k, v in compute(ref).items()}
    if os.environ.get("GBRL_RECORD_REF"):
        if not _to_record:
            import atexit
            atexit.register(_save_recording)
        _to_record.update({key + "::" + k: v for k, v in out.items()})
    return out


class RefScalars:
    """A sequence of float32 tuples from the reference's functions (oracle/_ref/ref_score_probe.so), live when the probe is built, else
    replayed in call order from the recording under `key`."""

    def __init__(self, key):
        import oracle
        self.key, self.live, self.rows, self.pos = key, oracle.ref_score_probe() is not None, [], 0
        if not self.live:
            self.recorded = _recording()[key + "::scalars"]

    def next(self, compute):
        if self.live:
            v = tuple(np.float32(x) for x in compute())
            self.rows.append(v)
            return v
        v = tuple(self.recorded[self.pos])
        self.pos += 1
        return v

    def finish(self):
        """All recorded calls were replayed; in record mode the sequence is stored."""
        if self.live:
            if os.environ.get("GBRL_RECORD_REF"):
                if not _to_record:
                    import atexit
                    atexit.register(_save_recording)
                _to_record[self.key + "::scalars"] = np.array(self.rows, np.float32)
        else:
            assert self.pos == len(self.recorded), (self.key, self.pos, len(self.recorded))
