"""The bytes step() leaves, over a grid that reaches every step kernel, for comparing two builds of the package line by line.

    python3 scripts/step_digest.py ROOT [> FILE]     # ROOT: the root of a built tree (it holds gbrl_amd/ with its extension)

One process.  Every case: 4100 rows x 19 numeric features (the shape of scripts/hist_variants_probe.py), NumPy inputs, 2 trees at depth 4, once with
set_profiling(0) and once with set_profiling(2).  A line per run: the sha256 of the saved model file and the names of last_phase_times() after the last step.
  - D in {1, 8, 16} at n_bins 64, both growth policies, both score functions, Quantile candidates (compile-time-D histogram kernels, 16 features
    per block; the root's histogram goes count-less) and Uniform candidates (column min / max, uniform thresholds, bisection binning);
  - (D, n_bins) = (17, 256), (24, 256), (31, 64): the wide and quad histogram kernels;  (40, 64), (63, 256): the run-time-D kernel at 2 features per block;
  - 5 categorical columns beside the 19 numeric ones;  257 rows (the small-step path);
  - oblivious growth with GBRL_HIP_DEVICE_LEVELS=1 (the device-side level planner), in a child process: a hook is read once per call, set before the start.
Categorical candidates, once each behind the first pass ("categorical: "): the Fc=5 case on the host scan (GBRL_HIP_HOST_CATEGORICAL=1); 40 categories per
column at n_bins 4 (more distinct cells than Fc * n_bins: the on-device ranking and the cut); no numeric column at all; 6 categories per column in the first
step and 300 in the second (the tables regrow; at n_bins 64 the 1500 cells are ranked, at n_bins 512 the list is published again as it is); fit() with categorical columns (the candidates-only step and the dictionary form
of the result).  The Quantile cases of the level-loop pass also under GBRL_HIP_QUANTILE_RADIX=1 and GBRL_HIP_QUANTILE_SAMPLE=1 ("radix: ", "sample: "), so
that every threshold route is reached.
A batch of 4100 rows is RL-sized: by default its statistics, preparation and whole tree growth run in the fused small-batch kernels (small_prep.hip,
small_grow.hip) and the level loop's kernels -- histogram build / reduce, score, arg-max, resolve, partition, leaf sums, the planner -- never start.  So the
whole grid runs again with GBRL_HIP_NO_SMALL_GROW=1 GBRL_HIP_NO_SMALL_PREP=1 GBRL_HIP_NO_SMALL_STATS=1 ("level loop"), which sends the same shapes through
the step kernels, and its Quantile cases a third time with GBRL_HIP_FORCE_BISECTION=1 on top ("bisection": k_bin_rows and the k_qsel kernels; Uniform
candidates are binned by bin_like.hip, not by them).  Not reached on one GPU: the winner / localize / count-right / place kernels of multi-GPU steps, k_stage_copy.
Nothing here is compared with anything: run it on both builds, each in a process of its own, and compare the two outputs (cmp).
"""
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests", "golden"))


def cases():
    def case(name, **kw):
        base = dict(name=name, seed=0, N=4100, F=19, Fc=0, D=8, depth=4, n_bins=64, score="L2", gen="Quantile", policy="greedy", trees=2)
        base.update(kw)
        return base
    for gen in ("Quantile", "Uniform"):
        for D in (1, 8, 16):
            for policy in ("greedy", "oblivious"):
                for score in ("L2", "Cosine"):
                    yield case("%s D=%d %s %s" % (gen, D, policy, score), gen=gen, D=D, policy=policy, score=score)
    for D, nb, policy in ((17, 256, "greedy"), (24, 256, "greedy"), (31, 64, "oblivious"), (40, 64, "greedy"), (63, 256, "greedy")):
        yield case("D=%d n_bins=%d %s" % (D, nb, policy), D=D, n_bins=nb, policy=policy, score="Cosine" if D % 2 else "L2")
    yield case("categorical Fc=5", Fc=5)
    yield case("rows=257", N=257)


DEVICE_LEVELS = dict(name="device levels oblivious", seed=0, N=4100, F=19, Fc=0, D=8, depth=4, n_bins=64, score="L2", gen="Quantile", policy="oblivious",
                     trees=2)


LEVEL_LOOP = ("GBRL_HIP_NO_SMALL_GROW", "GBRL_HIP_NO_SMALL_PREP", "GBRL_HIP_NO_SMALL_STATS")
PASSES = (("", ()), ("level loop: ", LEVEL_LOOP), ("bisection: ", LEVEL_LOOP + ("GBRL_HIP_FORCE_BISECTION",)))


def tokens(seed, N, Fc, n_tokens):
    """[N][Fc] S128 cells, n_tokens categories per column (cases.TOKENS stops at 32)."""
    import numpy as np
    names = np.array(["k%04d" % i for i in range(n_tokens)], dtype="S128")
    return names[np.random.default_rng(seed).integers(0, n_tokens, size=(N, Fc))]


def categorical_cases():
    base = dict(seed=0, N=4100, F=19, Fc=5, D=8, depth=4, n_bins=64, score="L2", gen="Quantile", policy="greedy", trees=2)
    yield dict(base, name="Fc=5 host scan"), {"GBRL_HIP_HOST_CATEGORICAL": "1"}
    yield dict(base, name="overflow Fc=3 n_bins=4", Fc=3, n_bins=4, cells=[40, 40]), {}
    yield dict(base, name="F=0 Fc=5", F=0), {}
    yield dict(base, name="cardinality jump", cells=[6, 300]), {}
    yield dict(base, name="cardinality jump n_bins=512", cells=[6, 300], n_bins=512), {}
    yield dict(base, name="fit Fc=5", fit=True), {}


def run(gbrl_amd, K, case, tag):
    import numpy as np
    X, Xc, G, y = K.make_inputs(case)
    F, Fc = case["F"], case["Fc"]
    for level in (0, 2):
        m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
        m.set_profiling(level)
        m.set_feature_weights(np.ones(F + Fc, np.float32))
        for o in K.optimizers(case):
            m.set_optimizer(**o)
        m.set_feature_mapping(np.arange(F + Fc, dtype=np.int32), np.array([True] * F + [False] * Fc, dtype=bool))
        if case.get("fit"):
            m.fit(X, Xc, np.ascontiguousarray(G.copy()), 3, False, "MultiRMSE")
        for t in range(0 if case.get("fit") else case["trees"]):
            cells = tokens(t, case["N"], Fc, case["cells"][t]) if "cells" in case else Xc
            m.step(X, cells, np.ascontiguousarray(G.copy()))
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "m.gbrl_model")
            assert m.save(p) == 0
            with open(p, "rb") as f:
                sha = hashlib.sha256(f.read()).hexdigest()
        print("%s%s profiling=%d  model: %s trees=%d  phases: %s" % (tag, case["name"], level, sha, m.get_num_trees(), " ".join(m.last_phase_times().keys())), flush=True)


def main(root, child):
    sys.path.insert(0, os.path.abspath(root))
    import cases as K
    import gbrl_amd
    if child:
        run(gbrl_amd, K, DEVICE_LEVELS, os.environ.get("STEP_DIGEST_TAG", ""))
        return 0
    status = 0
    for tag, hooks in PASSES:
        for hook in PASSES[-1][1]:      # (the library reads a hook anew in every call)
            os.environ.pop(hook, None)
        for hook in hooks:
            os.environ[hook] = "1"
        os.environ["STEP_DIGEST_TAG"] = tag
        for case in cases():
            if case["gen"] == "Quantile" or "GBRL_HIP_FORCE_BISECTION" not in hooks:
                run(gbrl_amd, K, case, tag)
        if not hooks:
            for case, env in categorical_cases():
                os.environ.update(env)
                run(gbrl_amd, K, case, "categorical: ")
                for k in env:
                    del os.environ[k]
        if tag == "level loop: ":
            for route, hook in (("radix: ", "GBRL_HIP_QUANTILE_RADIX"), ("sample: ", "GBRL_HIP_QUANTILE_SAMPLE")):
                os.environ[hook] = "1"
                for case in cases():
                    if case["gen"] == "Quantile":
                        run(gbrl_amd, K, case, route)
                del os.environ[hook]
        sys.stdout.flush()
        status |= subprocess.run([sys.executable, os.path.abspath(__file__), root, "--device-levels"], env=dict(os.environ, GBRL_HIP_DEVICE_LEVELS="1")).returncode
    return status


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3) or (len(sys.argv) == 3 and sys.argv[2] != "--device-levels"):
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], len(sys.argv) == 3))
