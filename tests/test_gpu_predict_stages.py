"""The nine predict-family entry points share their staging on one engine: the observation, id and target uploads, the output workspace, the
event pool and the device mirror.  A stage that leaks state from one call into the next would show as a result that depends on what ran before.

One model object makes every call in an interleaved order, twice -- host inputs and a "cpu" model first, then device inputs and a "cuda" model
-- and every result is compared BYTE FOR BYTE with the same call made on a fresh clone that has made no other call.  staged_loss is directly
followed by refit_leaves (on a clone of the busy model, then on the busy model itself: both share the targets workspace with it) and by
predict_continue with a host base (continued in place in the output workspace).  After a refit the fresh clones are clones of a fresh model
refitted the same way.  No tolerance anywhere.

257 rows (four waves and one row), 5 numeric columns (20-byte rows: unaligned), 2 categorical columns (encoded on every call), 3 outputs,
depth 3, 6 trees."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, F, FC, D, DEPTH, TREES = 257, 5, 2, 3, 3, 6
TOKENS = np.array(["tok%d" % i for i in range(6)], dtype="S128")
OPTS = {"const": dict(algo="SGD", scheduler="Const", init_lr=0.1), "linear": dict(algo="SGD", scheduler="Linear", init_lr=0.1, stop_lr=0.01, T=50)}


def _grown(policy, opt):
    import gbrl_amd
    rng = np.random.default_rng(4242)
    m = gbrl_amd.GBRL(input_dim=F + FC, output_dim=D, policy_dim=D, max_depth=DEPTH, min_data_in_leaf=0, n_bins=32, par_th=10, cv_beta=0.9,
                      split_score_func="L2", generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy=policy,
                      verbose=0, device="cpu", learner_name="stages")
    m.set_feature_weights(np.ones(F + FC, np.float32))
    m.set_optimizer(start_idx=0, stop_idx=D, **OPTS[opt])
    m.set_feature_mapping(np.arange(F + FC, dtype=np.int32), np.array([True] * F + [False] * FC, dtype=bool))
    m.set_bias(np.asarray(0.25 + 0.5 * np.arange(D), np.float32))
    for _ in range(TREES):
        X = rng.standard_normal((384, F)).astype(np.float32)
        Xc = TOKENS[rng.integers(0, 6, (384, FC))]
        G = rng.standard_normal((384, D)).astype(np.float32)
        G[:, 0] += X[:, 0] * 2.0
        G[:, -1] += (Xc[:, 0] == TOKENS[1]) * 3.0
        m.step(X, Xc, np.ascontiguousarray(G))
    assert m.get_num_trees() == TREES
    X = rng.standard_normal((N, F)).astype(np.float32)
    Xc = np.ascontiguousarray(TOKENS[rng.integers(0, 6, (N, FC))])
    Y = rng.standard_normal((N, D)).astype(np.float32)
    Y[:, 0] += 1.5 * X[:, 0]
    return m, X, Xc, np.ascontiguousarray(Y)


def _to_numpy(x):
    import torch
    return np.ascontiguousarray(x if isinstance(x, np.ndarray) else torch.from_dlpack(x).cpu().numpy())


class HostInputs:
    """NumPy in; the model delivers NumPy."""
    device = "cpu"

    def __init__(self, X, Xc, Y):
        self.X, self.Xc, self.Y = X, Xc, Y

    def ids(self, ids):
        return _to_numpy(ids)

    def base(self, b):
        return b.copy(), None


class DeviceInputs:
    """(data_ptr, shape, dtype, "cuda") tuples in; the model delivers DLPack capsules on its device."""
    device = "cuda"

    def __init__(self, X, Xc, Y):
        import torch
        self.keep = []
        self.X = self._tuple(torch.from_numpy(X), "torch.float32", X.shape)
        self.Xc = self._tuple(torch.from_numpy(np.frombuffer(Xc.tobytes(), np.uint8).reshape(N, FC, 128).copy()), "S128", (N, FC))
        self.Y = self._tuple(torch.from_numpy(Y), "torch.float32", Y.shape)

    def _tuple(self, t, dtype, shape):
        t = t.cuda()
        self.keep.append(t)
        return (t.data_ptr(), tuple(shape), dtype, "cuda")

    def ids(self, ids):
        import torch
        t = torch.from_dlpack(ids)
        self.keep.append(t)
        return (t.data_ptr(), tuple(t.shape), "torch.int32", "cuda")

    def base(self, b):                       # updated in place: the call returns None and the tensor holds the result
        import torch
        t = torch.from_numpy(b.copy()).cuda()
        return (t.data_ptr(), tuple(t.shape), "torch.float32", "cuda"), t


def _continue(m, obs, cat, base, tensor, a, b, token=None):
    got = m.predict_continue(obs, cat, base, a, b) if token is None else m.predict_continue_encoded(obs, cat, token, base, a, b)
    if tensor is None:
        return got
    assert got is None
    return tensor.cpu().numpy()


def _script(inp, base0, prefix, refit):
    """(name, fn(model) -> result) in call order; `refit_leaves` changes the model it is called on.  prefix["base"]: the prediction over the
    trees [0, 2) of the model as it is now."""
    X, Xc, Y = inp.X, inp.Xc, inp.Y
    enc = {}

    def encoded(m):                          # the ids of the batch, encoded once by the first model that asks (valid for every clone)
        if not enc:
            ids, token = m.encode_categorical(Xc)
            enc["ids"], enc["token"] = inp.ids(ids), token
        return enc["ids"], enc["token"]

    def host_continue(m):                    # a host base whatever the inputs are
        return m.predict_continue(X, Xc, base0.copy(), 0, 4)

    def continue_encoded(m):
        ids, token = encoded(m)
        b, t = inp.base(prefix["base"])
        return _continue(m, X, ids, b, t, 2, 0, token)

    def continue_plain(m):
        b, t = inp.base(prefix["base"])
        return _continue(m, X, Xc, b, t, 2, 5)

    return [
        ("predict_leaves", lambda m: m.predict_leaves(X, Xc, 1, 5)),
        ("predict", lambda m: m.predict(X, Xc, 0, 0)),
        ("staged_loss", lambda m: m.staged_loss(X, Xc, Y, [0, 2, 6])),
        ("refit_leaves", lambda m: m.refit_leaves(X, Xc, Y, *refit)),
        ("predict_continue host base", host_continue),
        ("leaf_counts", lambda m: m.leaf_counts(X, Xc, 0, 0)),
        ("predict_staged", lambda m: m.predict_staged(X, Xc, [1, 3, 6])),
        ("predict_encoded", lambda m: m.predict_encoded(X, *encoded(m), 0, 0)),
        ("predict_continue_encoded", continue_encoded),
        ("staged_loss all", lambda m: m.staged_loss(X, Xc, Y, None)),
        ("predict_continue", continue_plain),
        ("predict_leaves_encoded", lambda m: m.predict_leaves_encoded(X, *encoded(m), 0, 0)),
        ("leaf_counts_encoded", lambda m: m.leaf_counts_encoded(X, *encoded(m), 2, 3)),
        ("predict range", lambda m: m.predict(X, Xc, 2, 5)),
        ("predict_staged bias", lambda m: m.predict_staged(X, Xc, [0])),
    ]


def _values(m):
    return np.asarray(m.get_ensemble_data()["values"], np.float32).tobytes()


def _result_bytes(r):
    return np.float64(r).tobytes() if isinstance(r, float) else _to_numpy(r).tobytes()


@pytest.mark.parametrize("policy,opt", [("oblivious", "const"), ("greedy", "const"), ("oblivious", "linear")])
def test_every_call_on_a_busy_model_gives_the_bytes_of_a_fresh_clone(policy, opt):
    import gbrl_amd
    grown, X, Xc, Y = _grown(policy, opt)
    bias = np.asarray(grown.get_bias(), np.float32).reshape(-1)
    base0 = np.ascontiguousarray(np.tile(bias, (N, 1)))
    busy = gbrl_amd.GBRL(grown)              # makes every call
    ref = gbrl_amd.GBRL(grown)               # never makes a call but a refit: the fresh clones are cloned from it
    for inputs, refit in ((HostInputs, (1, 4, 0.0)), (DeviceInputs, (2, 0, 0.5))):      # refit: (start, stop, decay_rate)
        inp = inputs(X, Xc, Y)
        busy.to_device(inp.device)
        ref.to_device(inp.device)
        prefix = {"base": _to_numpy(gbrl_amd.GBRL(ref).predict_continue(X, Xc, base0.copy(), 0, 2))}
        for name, call in _script(inp, base0, prefix, refit):
            what = "%s (%s inputs)" % (name, inp.device)
            if name == "refit_leaves":
                # a clone of the busy model first: it leaves the busy model as it is
                side, fresh = gbrl_amd.GBRL(busy), gbrl_amd.GBRL(ref)
                want = call(fresh)
                assert _result_bytes(call(side)) == _result_bytes(want), what + ": the loss of a clone of the busy model"
                assert _values(side) == _values(fresh), what + ": the values of a clone of the busy model"
                assert _values(fresh) != _values(ref), what + ": the refit changed nothing"
                got = call(busy)             # then the busy model itself, right behind its staged_loss
                assert _result_bytes(got) == _result_bytes(want), what + ": loss"
                assert _values(busy) == _values(fresh), what + ": values"
                ref = fresh
                prefix["base"] = _to_numpy(gbrl_amd.GBRL(ref).predict_continue(X, Xc, base0.copy(), 0, 2))
                continue
            got, want = call(busy), call(gbrl_amd.GBRL(ref))
            a, b = _to_numpy(got), _to_numpy(want)
            assert a.dtype == b.dtype and a.shape == b.shape and a.size > 0, what
            assert a.tobytes() == b.tobytes(), what
