"""Host time of one predict() call at RL batch sizes: the configurations of scripts/predict_latency.py (depth 4, oblivious, 64 features, 8
outputs; 100 .. 20 000 trees x 1 .. 16 384 rows; NumPy in / NumPy out and device in / device out), 21 timed calls each after 3 warm-up
calls, the MEDIAN reported.  Used to compare two builds of the host side of the predict path (profiles/predict_stages.txt).
python scripts/predict_stages_latency.py [label]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, gbrl_amd

label = sys.argv[1] if len(sys.argv) > 1 else "run"
F, D, NB, CALLS = 64, 8, 4096, 21
rng = np.random.default_rng(0)
Xb = rng.standard_normal((16384, F)).astype(np.float32)
W = rng.standard_normal((F, D)).astype(np.float32)
m = gbrl_amd.GBRL(input_dim=F, output_dim=D, policy_dim=D, max_depth=4, min_data_in_leaf=0, n_bins=256, par_th=10, cv_beta=0.9,
                  split_score_func="cosine", generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy="oblivious",
                  verbose=0, device="cuda", learner_name="lat")
m.set_bias(np.zeros(D, np.float32)); m.set_feature_weights(np.ones(F, np.float32))
m.set_optimizer(algo="SGD", scheduler="Const", init_lr=0.01, start_idx=0, stop_idx=D)


def median_ms(call):
    for _ in range(3): call()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter(); r = call(); ts.append(time.perf_counter() - t0); del r
    return float(np.median(ts)) * 1e3


grown = 0
print("# %s: median of %d calls, ms" % (label, CALLS))
print("%6s %6s %12s %12s" % ("trees", "rows", "numpy", "device"))
for T in (100, 1000, 5000, 20000):
    while grown < T:
        G = np.tanh(Xb[:NB] @ W * (0.3 + 0.01 * (grown % 50))).astype(np.float32) + 0.1 * rng.standard_normal((NB, D)).astype(np.float32)
        m.step(Xb[:NB], None, G)
        grown += 1
    for n in (1, 16, 64, 256, 1024, 4096, 16384):
        x = np.ascontiguousarray(Xb[:n])
        xd = torch.from_numpy(x).cuda()
        tup = (xd.data_ptr(), tuple(xd.shape), "torch.float32", "cuda")
        print("%6d %6d %12.4f %12.4f" % (T, n, median_ms(lambda: m.predict(x, None, 0, 0)), median_ms(lambda: m.predict(tup, None, 0, 0))), flush=True)
