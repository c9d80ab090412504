"""Control variates on the GPU (GBRL.control_variates / control_variates_prepared; include/gbrl_hip.h, "Control variates").  Device against
gbrl_cpp.control_variates_host: equality of bytes, float rows and data set, streaming and one-thread-per-row walk (GBRL_HIP_CV_GENERIC=1, read per
call).  Against NumPy (tests/test_control_variates_host.py has the reference and the derivation of the bounds): momentum byte for byte over the leaves
predict_leaves reports, scale and alpha within one float32 ulp, grads recomputed from the returned statistics byte for byte.  Models by fit_prepared on
512 rows, n_bins = 32, F = 20 (two code groups); the corrected rows bound with reference=.  One axis varies at a time around n = 130, D = 3, 40 trees."""
import numpy as np
import pytest

import gbrl_amd
from test_control_variates_host import check_result, cv_chain, f32

pytestmark = pytest.mark.gpu
cpp = gbrl_amd.gbrl_cpp
N_TRAIN, F, BETA = 512, 20, 0.9
GROUP = cpp.control_variates_geometry(130, F, False, 3)["walk_trees"]

# id: n, D, policy, trees, depth
CASES = {
    "base": (130, 3, "oblivious", 40, 4),
    "n2": (2, 3, "oblivious", 40, 4),
    "n63": (63, 3, "oblivious", 40, 4),
    "n65": (65, 3, "oblivious", 40, 4),
    "d1": (130, 1, "oblivious", 40, 4),
    "d8": (130, 8, "oblivious", 40, 4),
    "d64": (130, 64, "oblivious", 40, 4),
    "d96_general": (130, 96, "oblivious", 40, 4),
    "greedy": (130, 3, "greedy", 40, 4),
    "t1": (130, 3, "oblivious", 1, 4),
    "t_group_plus_1": (130, 3, "oblivious", GROUP + 1, 4),
    "stump": (130, 3, "oblivious", 40, 1),
}


class Case:
    def __init__(self, n, D, policy, T, depth):
        rng = np.random.default_rng(1000 * D + 10 * T + depth + n)
        self.m = m = self.model(D, policy, depth)
        W = np.where(np.arange(F)[:, None] % 2 == 0, 1.5, 0.2) * rng.choice([-1.0, 1.0], size=(F, D))   # every even column matters: both code groups
        Xt = rng.standard_normal((N_TRAIN, F)).astype(f32)
        Y = (Xt @ W + 0.2 * rng.standard_normal((N_TRAIN, D))).astype(f32)
        self.Xt, self.ds_train, self.Y = Xt, m.prepare_dataset(Xt), np.ascontiguousarray(Y[:, 0]) if D == 1 else Y
        m.fit_prepared(self.ds_train, self.Y, T)
        assert m.get_num_trees() == T
        self.n, self.D, self.T, self.args = n, D, T, (D, policy, depth)
        self.X = rng.standard_normal((n, F)).astype(f32)
        self.ds = m.prepare_dataset(self.X, reference=self.ds_train)
        self.values = np.asarray(m.get_ensemble_data()["values"], f32).reshape(-1, D)
        self.leaves = np.asarray(m.predict_leaves(self.X, None))
        self.m_ref = cv_chain(self.values, self.leaves, (n, D), BETA)                      # the NumPy chain over the leaves predict_leaves reports
        self.ms = (self.m_ref * f32(cpp.control_variates_host(m, self.X, np.zeros((n,) if D == 1 else (n, D), f32), beta=BETA)["scale"])).astype(f32)
        G = (0.7 * self.ms + 0.3 * rng.standard_normal((n, D))).astype(f32)
        self.G = np.ascontiguousarray(G[:, 0]) if D == 1 else G
        self.host = cpp.control_variates_host(m, self.X, self.G, beta=BETA)   # computed once, shared, never written

    @staticmethod
    def model(D, policy, depth):
        m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=depth, n_bins=32, split_score_func="L2" if policy == "oblivious" else "Cosine",
                          generator_type="Quantile", grow_policy=policy, device="cpu", batch_size=N_TRAIN)
        m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.1, start_idx=0, stop_idx=D)
        m.set_feature_weights(np.ones(F, f32))
        m.set_feature_mapping(np.arange(F, dtype=np.int32), np.ones(F, dtype=bool))
        return m


@pytest.fixture(scope="module")
def case():
    made = {}
    return lambda name: made.setdefault(name, Case(*CASES[name]))


def _same(a, b, what):
    for key in ("grads", "momentum", "alpha", "mean_grads", "mean_momentum", "var", "cov", "scale", "n_trees"):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key, int((x != y).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_rule_and_numpy_through_both_kernels(name, case, monkeypatch):
    k = case(name)
    m, host = k.m, k.host
    plan = cpp.control_variates_geometry(k.n, F, False, k.D)
    assert plan["streaming"] == (k.D <= 64) and plan["launches"] == 4
    check_result(host, k.G, k.T, "host", k.m_ref)
    g0 = k.G.copy()
    _same(m.control_variates(k.X, None, k.G, beta=BETA), host, "float rows")
    _same(m.control_variates_prepared(k.ds, k.G, beta=BETA), host, "data set")
    _same(m.control_variates(k.X, None, k.G, beta=BETA), host, "float rows, again")           # determinism
    monkeypatch.setenv("GBRL_HIP_CV_GENERIC", "1")
    _same(m.control_variates(k.X, None, k.G, beta=BETA), host, "float rows, general walk")
    _same(m.control_variates_prepared(k.ds, k.G, beta=BETA), host, "data set, general walk")
    monkeypatch.delenv("GBRL_HIP_CV_GENERIC")
    assert k.G.tobytes() == g0.tobytes()                                                       # the input is not written
    rows = np.array([k.n - 1, 0, 1, k.n - 1, 0], np.int32)                                      # duplicates, out of order
    _same(m.control_variates_prepared(k.ds, k.G[rows], beta=BETA, rows=rows), m.control_variates(k.X[rows], None, k.G[rows], beta=BETA), "rows=")
    clipped = m.control_variates_prepared(k.ds, (3 * k.ms).astype(f32).reshape(k.G.shape), beta=BETA)
    assert (clipped["alpha"] == 1.0).all(), clipped["alpha"]
    held = np.asarray(host["momentum"])                                                        # nothing left to walk: the statistics alone
    _same(m.control_variates_prepared(k.ds, k.G, beta=BETA, momentum=held, start_tree_idx=k.T), host, "momentum over every tree")


@pytest.mark.parametrize("name", ["base", "d1", "d8", "d96_general"])
def test_a_cuda_model_on_device_tensors_gives_the_host_bytes_and_steps(name, case):
    """the path of a learner: a "cuda" model, observations, gradients and momentum on the device, capsules back, r["grads"] into step_prepared"""
    import torch
    k = case(name)
    tup = lambda t: (t.data_ptr(), tuple(t.shape), str(t.dtype), "cuda")
    X, G = torch.from_numpy(k.X).cuda(), torch.from_numpy(k.G).cuda()
    k.m.to_device("cuda")
    try:
        first = k.m.control_variates(tup(X), None, tup(G), beta=BETA, start_tree_idx=0)
        got = {key: torch.from_dlpack(v).cpu().numpy() if key in ("grads", "momentum") else v for key, v in first.items()}
        _same(got, k.host, "cuda model, float rows")
        mom = torch.from_dlpack(k.m.control_variates_prepared(k.ds, tup(G), beta=BETA)["momentum"])
        r = k.m.control_variates_prepared(k.ds, tup(G), beta=BETA, momentum=tup(mom), start_tree_idx=k.T)
        grads = torch.from_dlpack(r["grads"])
        assert grads.cpu().numpy().tobytes() == np.asarray(k.host["grads"]).tobytes() and G.cpu().numpy().tobytes() == k.G.tobytes()
    finally:
        k.m.to_device("cpu")
    stepped = gbrl_amd.GBRL(k.m)                                                               # (a copy: the shared case keeps its trees)
    stepped.step_prepared(k.ds, tup(grads))
    assert stepped.get_num_trees() == k.T + 1


@pytest.mark.parametrize("name", ["base", "greedy", "d64", "d96_general"])
def test_a_held_momentum_continued_gives_the_bytes_of_the_full_call(name, case):
    k = case(name)
    cut = GROUP + 3                                                                            # not a multiple of the walk's tree group
    short = Case.model(*k.args)
    train = short.prepare_dataset(k.Xt)                                                        # the same rows, the same fit: the full model's first trees
    short.fit_prepared(train, k.Y, cut)
    ds = short.prepare_dataset(k.X, reference=train)
    held = short.control_variates_prepared(ds, k.G, beta=BETA)
    assert held["n_trees"] == cut
    full = k.m.control_variates(k.X, None, k.G, beta=BETA, momentum=np.asarray(held["momentum"]), start_tree_idx=cut)
    _same(full, k.host, "continued, float rows")
    _same(k.m.control_variates_prepared(k.ds, k.G, beta=BETA, momentum=np.asarray(held["momentum"]), start_tree_idx=cut), k.host, "continued, data set")


def test_constant_momentum_no_trees_and_refusals(case):
    k = case("base")
    X = np.tile(k.X[:1], (70, 1))
    G = np.random.default_rng(5).standard_normal((70, 3)).astype(f32)
    r = k.m.control_variates(X, None, G, beta=BETA)
    assert not r["var"].any() and not r["alpha"].any() and np.asarray(r["grads"]).tobytes() == G.tobytes()
    empty = Case.model(3, "oblivious", 4)
    e = empty.control_variates(X, None, G)
    assert np.asarray(e["grads"]).tobytes() == G.tobytes() and not np.asarray(e["momentum"]).any() and not e["alpha"].any() and e["n_trees"] == 0
    for kw, text in ((dict(beta=1.5), "beta must lie in"), (dict(start_tree_idx=41), "start_tree_idx"), (dict(momentum=np.zeros((69, 3), f32)), "momentum")):
        with pytest.raises(RuntimeError, match=text):
            k.m.control_variates(X, None, G, **kw)
    with pytest.raises(RuntimeError, match="at least 2 rows"):
        k.m.control_variates(X[:1], None, G[:1])
    with pytest.raises(RuntimeError, match="130"):
        k.m.control_variates_prepared(k.ds, G)                                                 # 70 gradients, a data set of 130 rows, no rows=
