"""Case list of the categorical-ranking fixtures (made by make_catrank_golden.py, read by tests/test_gpu_cat_rank.py and
tests/test_cat_rank_host.py): batches and data sets with MORE distinct (feature, category) pairs than the Fc * n_bins candidates the
reference keeps.  It then ranks the categories by their mean squared gradient norm (split_candidate_generator.cpp:117-163): float32
totals in row order, std::sort on the hash map's iteration order, the first Fc * n_bins survive.

Same case dicts as cases.py and the same drivers (cases.drive / cases.drive_fit); the inputs are synthesised here because cases.py's
token table ends at 32 tokens.  Integer PCG64 draws and exactly-rounded IEEE float32 arithmetic only, like cases.make_inputs.
"""
import numpy as np

import cases as K
from cases import _c

TOKENS = np.array([f"k{i:02d}" for i in range(64)], dtype="S128")


def make_inputs(case):
    rng = np.random.default_rng(case["seed"])
    N, F, Fc, D, T = case["N"], case["F"], case["Fc"], case["D"], case["n_tokens"]
    X = K._normalish(rng, (N, F))
    idx = rng.integers(0, T, size=(N, Fc))
    Xc = TOKENS[idx]
    effect = K._normalish(rng, (T,))                       # every token shifts the gradient by its own amount: the mean norms differ
    if case.get("unit_grads"):                              # every squared norm is exactly D: all means tie
        G = (rng.integers(0, 2, size=(N, D)).astype(np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    else:
        noise = K._normalish(rng, (N, D)) * np.float32(0.5)
        G = np.empty((N, D), np.float32)
        for d in range(D):
            G[:, d] = X[:, d % F] * np.float32(0.5) + effect[idx[:, d % Fc]] + noise[:, d]
    y = None
    if case.get("loop") == "rmse":
        x0 = np.clip(X[:, 0], np.float32(-2), np.float32(2))
        y = (x0 - x0 * x0 * x0 / np.float32(6.0) + effect[idx[:, 0]] - effect[idx[:, Fc - 1]] * np.float32(0.5)
             + K._normalish(rng, (N,)) * np.float32(0.1)).astype(np.float32)
        if D > 1:
            y = np.stack([y * np.float32(d + 1) for d in range(D)], axis=1).astype(np.float32)
    return X, Xc, np.ascontiguousarray(G), y


STEP_CASES = [
    # 80 distinct (feature, token) pairs against 8 kept
    _c("catrank_grd_l2_q", seed=51, N=600, F=3, Fc=2, D=2, depth=3, policy="greedy", n_bins=4, n_tokens=40, trees=2),
    # 60 against 15
    _c("catrank_obl_cos_u", seed=52, N=500, F=2, Fc=3, D=1, depth=3, score="Cosine", gen="Uniform", n_bins=5, n_tokens=20, trees=2),
    # gradients in {-1, +1}, D = 4: every norm is 4.0, every total a multiple of 4 and every mean 4.0.  60 tied categories against 16 kept:
    # std::sort leaves its insertion-sort regime (more than 16 elements) and the kept set is decided by the container's iteration order
    _c("catrank_ties", seed=53, N=4096, F=2, Fc=2, D=4, depth=3, n_bins=8, n_tokens=30, trees=2, unit_grads=True),
]

# fit(): N * D and batch_size * D are multiples of 24 (cases.py, FIT_CASES).  60 distinct pairs against 8 kept.  `fit2_iterations`: a
# second fit() on the grown model; 6 > the 4 trees it holds, so the reference's full_grads come from the bias alone (predictor.cpp:130-133)
FIT_CASES = [
    _c("catrank_fit", seed=54, N=2400, F=4, Fc=2, D=1, depth=3, n_bins=4, n_tokens=30, loop="rmse", batch_size=1200, fit_iterations=4,
       fit2_iterations=6, opts=[dict(algo="SGD", scheduler="Const", init_lr=0.4, start_idx=0, stop_idx=1)]),
]

BY_NAME = {c["name"]: c for c in STEP_CASES + FIT_CASES}
FIT2_KEYS = tuple("fit2_" + k for k in K.ENSEMBLE_KEYS)
