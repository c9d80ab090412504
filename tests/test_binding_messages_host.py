"""The refusals of the binding's shared argument readers (gbrl_amd/csrc/binding_common.cpp: require_input, require_host; binding.cpp:
read_sample_shape), caller by caller and character for character.  No device: every call here is refused before one is touched.  The
expected texts were written down from the callers' own wording before they shared a reader, so a message that two callers spell
differently ("takes a NumPy array" / "takes NumPy arrays", "Gradient" / "Targets") must still differ."""
import numpy as np
import pytest

import gbrl_amd

cpp = gbrl_amd.gbrl_cpp
F32 = "torch.float32"
NULL_F32 = (0, (4,), F32, "cpu")          # a tensor tuple with a null pointer: refused in the words of a missing argument


def model(input_dim=3, output_dim=1):
    return gbrl_amd.GBRL(input_dim=input_dim, output_dim=output_dim, policy_dim=1, max_depth=2, n_bins=16, split_score_func="L2",
                         generator_type="Quantile", grow_policy="oblivious", device="cpu", batch_size=8)


def message(call):
    with pytest.raises(RuntimeError) as e:
        call()
    return str(e.value)


OBS = np.zeros((4, 3), np.float32)
Y = np.zeros(4, np.float32)
LABELS = np.zeros(4, np.int32)

# (caller, the missing argument) -> the call with `x` in the argument's place, the expected text.  PreparedDataset.sample_goss(grads) is the
# seventeenth caller of require_input; it needs a data set, hence a device, and shares read_goss_grads with goss_rows_host below.
REQUIRED = {
    ("encode_categorical", "cat_obs"): (lambda m, x: m.encode_categorical(x), "Cannot call encode_categorical without cat_obs!"),
    ("prepare_dataset", "obs"): (lambda m, x: m.prepare_dataset(x), "Cannot call prepare_dataset without obs!"),
    ("goss_rows_host", "grads"): (lambda m, x: cpp.goss_rows_host(x, 0.2, 0.1), "Cannot call goss_rows_host without grads!"),
    ("predict_continue_prepared", "base"): (lambda m, x: m.predict_continue_prepared(None, x), "Cannot call predict_continue_prepared without base!"),
    ("newton_leaves_prepared", "pred"): (lambda m, x: m.newton_leaves_prepared(None, x, Y, "logistic"), "Cannot call newton_leaves_prepared without pred!"),
    ("newton_leaves_prepared (ranking)", "pred"): (lambda m, x: m.newton_leaves_prepared(None, x, LABELS, "pairwise", group=[4]),
                                                   "Cannot call newton_leaves_prepared without pred!"),
    ("quantile_leaves_prepared", "pred"): (lambda m, x: m.quantile_leaves_prepared(None, x, Y, 0.5), "Cannot call quantile_leaves_prepared without pred!"),
    ("eval_metric", "pred"): (lambda m, x: m.eval_metric(x, Y, "logistic", "error"), "Cannot call eval_metric without pred!"),
    ("rank_gradient", "pred"): (lambda m, x: m.rank_gradient(x, LABELS, [4], "pairwise"), "Cannot call rank_gradient without pred!"),
    ("objective_gradient", "pred"): (lambda m, x: m.objective_gradient(x, Y, "rmse"), "Cannot call objective_gradient without pred!"),
    ("rank_gradient", "labels"): (lambda m, x: m.rank_gradient(Y, x, [4], "pairwise"), "Cannot call rank_gradient without labels!"),
    ("rank_gradient_host", "labels"): (lambda m, x: cpp.rank_gradient_host(Y, x, [4], "pairwise"), "Cannot call rank_gradient_host without labels!"),
    ("predict_continue", "base"): (lambda m, x: m.predict_continue(OBS, None, x), "Cannot call predict_continue without base!"),
    ("predict_continue_encoded", "base"): (lambda m, x: m.predict_continue_encoded(OBS, None, 0, x), "Cannot call predict_continue without base!"),
    ("staged_loss", "targets"): (lambda m, x: m.staged_loss(OBS, None, x), "Cannot call staged_loss without targets!"),
    ("refit_leaves", "targets"): (lambda m, x: m.refit_leaves(OBS, None, x), "Cannot call refit_leaves without targets!"),
}


@pytest.mark.parametrize("site", sorted(REQUIRED), ids=lambda s: "%s-%s" % s)
def test_a_missing_required_argument_is_refused_in_the_callers_words(site):
    call, text = REQUIRED[site]
    null = {"cat_obs": (0, (4, 1), "S128", "cpu"), "labels": (0, (4,), "torch.int32", "cpu")}.get(site[1], NULL_F32)
    m = model()
    assert message(lambda: call(m, None)) == text
    assert message(lambda: call(m, null)) == text


def dev(shape, dtype=F32):
    return (64, shape, dtype, "cuda")      # never read: the host rules refuse a device tensor by where it says it lives


HOST_ONLY = {
    ("goss_rows_host", "grads"): (lambda m: cpp.goss_rows_host(dev((4,)), 0.2, 0.1), "goss_rows_host takes a NumPy array"),
    ("condition_bins", "thresholds"): (lambda m: m.condition_bins(dev((3, 16))), "condition_bins takes a NumPy array"),
    ("partial_dependence_codes", "thresholds"): (lambda m: m.partial_dependence_codes(dev((3, 16)), 0), "partial_dependence_codes takes a NumPy array"),
    ("objective_hessian_host", "pred"): (lambda m: cpp.objective_hessian_host(dev((4,))), "objective_hessian_host takes NumPy arrays"),
    ("objective_hessian_host", "weights"): (lambda m: cpp.objective_hessian_host(Y, None, "logistic", dev((4,))), "objective_hessian_host takes NumPy arrays"),
    ("eval_metric_host", "pred"): (lambda m: cpp.eval_metric_host(dev((4,)), Y, "logistic", "error"), "eval_metric_host takes NumPy arrays"),
    ("eval_metric_host", "targets"): (lambda m: cpp.eval_metric_host(Y, dev((4,)), "logistic", "error"), "eval_metric_host takes NumPy arrays"),
    ("objective_gradient_host", "pred"): (lambda m: cpp.objective_gradient_host(dev((4,)), Y, "rmse"), "objective_gradient_host takes NumPy arrays"),
    ("objective_gradient_host", "targets"): (lambda m: cpp.objective_gradient_host(Y, dev((4,)), "rmse"), "objective_gradient_host takes NumPy arrays"),
    ("objective_gradient_host", "weights"): (lambda m: cpp.objective_gradient_host(Y, Y, "rmse", dev((4,))), "objective_gradient_host takes NumPy arrays"),
    ("rank_gradient_host", "scores"): (lambda m: cpp.rank_gradient_host(dev((4,)), LABELS, [4], "pairwise"), "rank_gradient_host takes NumPy arrays"),
    ("rank_gradient_host", "labels"): (lambda m: cpp.rank_gradient_host(Y, dev((4,), "torch.int32"), [4], "pairwise"), "rank_gradient_host takes NumPy arrays"),
}


@pytest.mark.parametrize("site", sorted(HOST_ONLY), ids=lambda s: "%s-%s" % s)
def test_a_host_rule_refuses_a_device_tensor_in_its_own_words(site):
    call, text = HOST_ONLY[site]
    assert message(lambda: call(model())) == text


def cells(n, f):
    return np.zeros((n, f), "S128")


# step and fit read their shapes alike; fit names its targets where step names its gradients, and keeps step's "gradient samples" elsewhere
SHAPES = {
    "missing": (lambda first: (OBS, None, None), "Cannot call {fn} without {name}!"),
    "output dim": (lambda first: (OBS, None, np.zeros((4, 3), np.float32)), "{noun} output dim 3 != correct output dim 2"),
    "observations": (lambda first: (np.zeros((3, 3), np.float32), None, first), "Number of observations 3 != number of gradient samples 4"),
    "categorical observations": (lambda first: (np.zeros((4, 2), np.float32), cells(3, 1), first),
                                 "Number of categorical observations 3 != number of gradient samples 4"),
    "feature total": (lambda first: (np.zeros((4, 2), np.float32), None, first), "Total number of features 2 != correct input dim 3"),
}


@pytest.mark.parametrize("refusal", list(SHAPES))
@pytest.mark.parametrize("fn,name,noun", [("step", "grads", "Gradient"), ("fit", "targets", "Targets")])
def test_step_and_fit_refuse_a_shape_in_the_same_words_but_for_the_noun(fn, name, noun, refusal):
    args, text = SHAPES[refusal]
    m = model(input_dim=3, output_dim=2)
    obs, cat, first = args(np.zeros((4, 2), np.float32))
    call = (lambda: m.step(obs, cat, first)) if fn == "step" else (lambda: m.fit(obs, cat, first, 1))
    assert message(call) == text.format(fn=fn, name=name, noun=noun)


def test_step_prepared_reads_its_gradients_as_step_does():
    m = model(input_dim=3, output_dim=2)
    assert message(lambda: m.step_prepared(None, np.zeros((4, 3), np.float32))) == "Gradient output dim 3 != correct output dim 2"
    assert message(lambda: m.step_prepared(None, None)) == "Cannot call step_prepared without grads!"
