"""The numpy restatement of include/mi_iqn.h (tests/_iqn_ref.py) against the fixtures captured from the reference's own statements (tools/capture_iqn_ref.py):
every checkpoint's current / target quantiles, next actions, loss, gradient and parameters after Adam; the acting forwards of the two reference classes; the
i_pi table; the fixtures' form.  The figures measured here are the MEASURED_* constants of _iqn_ref.py (each test asserts the constant covers what it measures and
prints the figure); the device bounds of the GPU tests are 8 x those constants."""
import os
import re

import numpy as np
import pytest

import _iqn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["iqn_ref_trace.npz", "iqn_ref_start.npz"]


@pytest.fixture(scope="module")
def trace():
    return R.load_trace()


@pytest.fixture(scope="module")
def evaluated(trace):
    """f32 and float64 restatement of every checkpoint update, computed once"""
    out = {}
    ringv = R.ring(trace)
    for k in trace["checkpoints"]:
        c = R.load_ckpt(int(k))
        args = (c["params_before"], c["target_params"], ringv, c["batch_inds"], c["taus"], c["next_taus"], c["tau_dashes"])
        out[int(k)] = (c, R.update(*args, dtype=np.float32), R.update(*args, dtype=np.float64))
    return out


def test_fixtures_hold_numbers_only_and_stay_small(trace):
    names = FILES + ["iqn_ref_ckpt%d.npz" % k for k in trace["checkpoints"]]
    learning = os.path.join(R.GOLD, "iqn_learning_stats.npz")
    if os.path.exists(learning):
        names.append("iqn_learning_stats.npz")
    assert len(trace["checkpoints"]) == 4
    for n in names:
        path = os.path.join(R.GOLD, n)
        assert os.path.getsize(path) < (1 << 20), n
        z = np.load(path, allow_pickle=False)
        assert all(z[k].dtype.kind in "fiu" for k in z.files), n


def test_fixture_is_what_the_issue_asks_for(trace, evaluated):
    B = int(trace["hparams"][5])   # the trace run's batch (tools/capture_iqn_ref.py: TRACE_BATCH)
    assert B == 8 and trace["batch_inds"].shape == (21, B) and trace["taus"].shape == (21, B, 64) and trace["next_taus"].shape == (21, B, 32) and trace["tau_dashes"].shape == (21, B, 64)
    assert trace["init_params"].shape == (R.NPARAMS,) and trace["sync_after_update"].tolist() == [10] and {10, 11} <= set(trace["checkpoints"].tolist())
    assert 100 <= len(trace["ring_actions"]) <= 2000 and trace["act_obs"].shape[0] >= 4
    hp = trace["hparams"]
    assert hp[:7].tolist() == [0.99, 5e-5, 1e-2 / B, 0.01, 1.0, B, 4] and hp[7:10].tolist() == [1000, 500, 50000]
    assert trace["near_kappa"].shape == (21,) and trace["flip_allowance"].shape == (21,) and all(trace["near_kappa"][k] == 0 for k in trace["checkpoints"])
    # the batch rows the update block formed are the compact ring's rows
    ringv = R.ring(trace)
    for k, (c, _r32, r64) in evaluated.items():
        X, A, Xn, Rw, T = R.batch_of(ringv, c["batch_inds"])
        assert np.array_equal(X, c["b_observations"]) and np.array_equal(Xn, c["b_next_observations"]) and np.array_equal(A, c["b_actions"])
        assert np.array_equal(Rw, c["b_rewards"]) and np.array_equal(T, c["b_terminated"])
        # the condition the capture tool asserts: no td error within NEAR_KAPPA_REL x max |quantile| of kappa, the 8 x margin
        d = r64["target"][:, None, :] - r64["current"][:, :, None]
        scale = max(1.0, np.abs(r64["target"]).max(), np.abs(r64["current"]).max())
        assert np.abs(np.abs(d) - 1.0).min() > R.NEAR_KAPPA_REL * scale, k
    assert any(c["b_terminated"].any() for c, _a, _b in evaluated.values())


def test_i_pi_table_equals_the_headers_constants(trace):
    hdr = open(os.path.join(ROOT, "include", "mi_iqn.h")).read()
    body = re.search(r"#define MI_IQN_I_PI_BITS(.*?)\n\n", hdr, flags=re.S).group(1)
    bits = np.array([int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", body)], np.uint32)
    assert bits.shape == (64,) and np.array_equal(bits, trace["i_pi"].view(np.uint32)) and np.array_equal(R.I_PI.view(np.uint32), bits)


def test_restated_forward_of_the_reference_classes_at_the_acting_forwards(trace):
    p = trace["act_params"]
    fig = {}
    for mode in (np.float32, np.float64):
        r = R.forward(p, trace["act_obs"], trace["act_taus"], mode)
        fig[mode.__name__] = (float(np.abs(r["quantiles"] - trace["act_quantiles"]).max()), float(np.abs(r["q"] - trace["act_q"]).max()))
        assert np.array_equal((r["q"][:, 1] > r["q"][:, 0]).astype(np.int32), trace["act_action"])
    scale = float(np.abs(trace["act_quantiles"]).max())
    print("acting forwards: |quantile|, |q| error f32 %s, float64 %s, max |quantile| %.3f" % (fig["float32"], fig["float64"], scale))
    assert fig["float32"][0] <= max(R.MEASURED_QUANT_ABS, R.MEASURED_QUANT_REL * scale) and fig["float32"][1] <= R.MEASURED_Q_ABS


def test_restatement_at_every_checkpoint_within_the_measured_figures(evaluated):
    worst = dict(quant_abs=0.0, quant_rel=0.0, q_abs=0.0, loss_rel=0.0, grad_rel=0.0, grad_tensor_rel=0.0, preact=0.0)
    for k, (c, r32, r64) in evaluated.items():
        scale = max(np.abs(c["current_action_quantiles"]).max(), np.abs(c["target_action_quantiles"]).max())
        for ref_cur, ref_tgt, ref_loss, ref_g in ((c["current_action_quantiles"], c["target_action_quantiles"], float(c["loss"][0]), c["grads"]),
                                                  (r64["current"], r64["target"], float(r64["loss"]), r64["grads"])):
            qa = max(np.abs(r32["current"] - ref_cur).max(), np.abs(r32["target"] - ref_tgt).max())
            worst["quant_abs"] = max(worst["quant_abs"], qa); worst["quant_rel"] = max(worst["quant_rel"], qa / scale)
            worst["loss_rel"] = max(worst["loss_rel"], abs(float(r32["loss"]) - ref_loss) / abs(ref_loss))
            worst["grad_rel"] = max(worst["grad_rel"], np.abs(r32["grads"] - ref_g).max() / np.abs(ref_g).max())
        worst["grad_tensor_rel"] = max([worst["grad_tensor_rel"]] + list(R.tensor_grad_errors(r32["grads"], c["grads"]).values()) + list(R.tensor_grad_errors(r32["grads"], r64["grads"]).values()))
        worst["q_abs"] = max(worst["q_abs"], np.abs(r32["q_next"] - r64["q_next"]).max())
        worst["preact"] = max([worst["preact"]] + [np.abs(r32["fw"][n].astype(np.float64) - r64["fw"][n]).max() for n in ("z1", "z2", "z3", "zc", "z")])
        assert np.array_equal(r32["next_actions"], c["next_actions"]) and np.array_equal(r64["next_actions"], c["next_actions"]), k
        # float64 against the reference's own f32: the same order of magnitude, i.e. the fixture IS this arithmetic
        assert np.abs(r64["grads"] - c["grads"]).max() / np.abs(c["grads"]).max() <= R.MEASURED_GRAD_REL
    print("restatement, worst over the checkpoints:", {k: float(v) for k, v in worst.items()})
    assert worst["quant_abs"] <= R.MEASURED_QUANT_ABS and worst["quant_rel"] <= R.MEASURED_QUANT_REL and worst["q_abs"] <= R.MEASURED_Q_ABS
    assert worst["loss_rel"] <= R.MEASURED_LOSS_REL and worst["grad_rel"] <= R.MEASURED_GRAD_REL and worst["preact"] <= R.MEASURED_PREACT_ABS
    assert worst["grad_tensor_rel"] <= R.MEASURED_GRAD_TENSOR_REL
    # the constants are figures, not head-room: each lies within 4 x of what is measured here
    assert worst["quant_rel"] >= R.MEASURED_QUANT_REL / 4 and worst["grad_rel"] >= R.MEASURED_GRAD_REL / 4 and worst["loss_rel"] >= R.MEASURED_LOSS_REL / 4


def test_chained_restatement_lands_on_the_references_parameters(trace):
    """the 21 chained updates in the f32 restatement (its own gradients, its own Adam) from the window's start: the distance from the reference's parameters at the
    checkpoints is MEASURED_PARAM_ABS, the figure the device's 21-step bound is 8 x of"""
    st = R.load_start()
    ringv, B = R.ring(trace), int(trace["hparams"][5])
    p, m, v, tp = st["params"].copy(), st["exp_avg"].copy(), st["exp_avg_sq"].copy(), st["target_params"].copy()
    step = int(trace["start_adam_step"][0])
    after = {int(k): R.load_ckpt(int(k))["params_after"] for k in trace["checkpoints"]}
    worst = 0.0
    for k in range(21):
        r = R.update(p, tp, ringv, trace["batch_inds"][k], trace["taus"][k], trace["next_taus"][k], trace["tau_dashes"][k], dtype=np.float32)
        step += 1
        R.adam_step(p, r["grads"], m, v, step, eps=0.01 / B)
        if k in after:
            worst = max(worst, float(np.abs(p - after[k]).max()))
        assert abs(float(r["loss"]) - trace["loss"][k]) <= R.MEASURED_LOSS_REL * trace["loss"][k] + trace["flip_allowance"][k], k
        if k in trace["sync_after_update"]:
            tp = p.copy()
    print("21 chained updates of the f32 restatement: max |p - reference| at the checkpoints = %.3g" % worst)
    assert R.MEASURED_PARAM_ABS / 4 <= worst <= R.MEASURED_PARAM_ABS


def test_adam_step_at_every_checkpoint(evaluated):
    """the parameters after optimizer.step() at the checkpoints: a finite, small, non-zero step (Adam's arithmetic itself is measured through the 21 chained updates
    above, whose moments are known from the window's start)"""
    for k, (c, _a, _b) in evaluated.items():
        step = np.abs(c["params_after"] - c["params_before"])
        assert np.isfinite(step).all() and 0 < step.max() <= 1e-3, k   # a few lr: m / sqrt(v) is O(1)
