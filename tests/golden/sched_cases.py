"""Case list of the Linear learning-rate scheduler fixtures (made by make_sched_golden.py, read by tests/test_sched_host.py and
tests/test_gpu_sched.py).  Same case dicts as cases.py; the inputs come from cases.make_inputs and the runs go through cases.drive /
cases.drive_fit, whose `opts` entries pass any set_optimizer keyword.

LinearScheduler::get_lr (scheduler.h:124-134): lr(t) = init_lr + ((t + 1) / T) * (stop_lr - init_lr), never below stop_lr.  With a
falling schedule the clamp holds from t + 1 == T on, so T is chosen INSIDE the ensemble: trees before, at and after t + 1 == T exist.
"""
from cases import _c


def _lin(init_lr, stop_lr, T, start_idx, stop_idx):
    return dict(algo="SGD", scheduler="Linear", init_lr=init_lr, start_idx=start_idx, stop_idx=stop_idx, stop_lr=stop_lr, T=T)


def _const(init_lr, start_idx, stop_idx):
    return dict(algo="SGD", scheduler="Const", init_lr=init_lr, start_idx=start_idx, stop_idx=stop_idx)


CASES = [
    # oblivious / L2 / Quantile, one Linear optimizer; t + 1 == T at tree 9 of 16
    _c("sched_obl_l2_q", seed=41, N=2048, F=8, D=3, depth=4, loop="rmse", trees=16, opts=[_lin(0.3, 0.05, 10, 0, 3)],
       pred_ranges=[[0, 5], [3, 12], [9, 16], [12, 16], [15, 16]]),
    # shared actor-critic, greedy / Cosine: a Const policy range and a Linear value range (the schedule is not exhausted: T = 20 > trees)
    _c("sched_grd_cos_q_ac", seed=42, N=2048, F=8, D=8, depth=5, policy="greedy", score="Cosine", loop="rmse", trees=14,
       opts=[_const(0.1, 0, 7), _lin(0.05, 0.005, 20, 7, 8)], pred_ranges=[[2, 9], [5, 14], [13, 14]]),
    # categorical columns; a RISING schedule (stop_lr > init_lr: the clamp `lr < stop_lr` then holds BEFORE t + 1 == T)
    _c("sched_obl_cos_q_cat", seed=43, N=1536, F=5, Fc=2, D=2, depth=4, score="Cosine", loop="rmse", y_cat_weight=1.0, trees=12,
       opts=[_lin(0.2, 0.02, 8, 0, 1), _lin(0.02, 0.2, 8, 1, 2)], pred_ranges=[[4, 12]]),
]

FIT_CASES = [
    _c("sched_fit_obl_l2_q", seed=44, N=3000, F=6, D=2, depth=4, n_bins=64, loop="rmse", batch_size=1200, fit_iterations=12,
       opts=[_lin(0.5, 0.1, 8, 0, 2)]),
]

BY_NAME = {c["name"]: c for c in CASES + FIT_CASES}
MODEL_FILE_CASES = ("sched_obl_l2_q", "sched_grd_cos_q_ac")
# name -> (modelname, export_format, export_type, prefix) of the stored exported header (export is oblivious-only in the reference)
EXPORT_CASES = {"sched_obl_l2_q": ("", "float", "full", "")}

# ---- recordings (sched_recordings.npz) ----
# get_scheduler_lrs() after 0, 1, 2, ... trees for these optimizer lists (a tiny model stepped on 64 rows)
LRS_SCHEDULES = {
    "falling": [_lin(0.3, 0.05, 10, 0, 1), _const(0.07, 1, 2)],
    "rising": [_lin(0.01, 0.25, 7, 0, 2)],
    "long": [_lin(0.1, 1e-8, 10000, 0, 1), _lin(0.05, 0.049, 3, 1, 2)],
}
LRS_TREES = 14
LRS_KW = dict(input_dim=3, output_dim=2, policy_dim=2, max_depth=2, min_data_in_leaf=0, n_bins=16, par_th=10, cv_beta=0.9, split_score_func="L2",
              generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy="oblivious", verbose=0, device="cpu",
              learner_name="lrs")
# the model file of a fresh, treeless model with these optimizers
FRESH_KW = dict(input_dim=4, output_dim=2, policy_dim=2, max_depth=3, min_data_in_leaf=0, n_bins=256, par_th=10, cv_beta=0.9, split_score_func="L2",
                generator_type="Quantile", use_control_variates=False, batch_size=5000, grow_policy="oblivious", verbose=0, device="cpu",
                learner_name="fresh_linear")
FRESH_OPTS = [_lin(0.1, 0.001, 500, 0, 1), _const(0.01, 1, 2)]
