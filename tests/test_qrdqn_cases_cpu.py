"""The synthetic QR-DQN cases (tests/_qrdqn_cases.py) hold what they claim — on the CPU, before tests/test_gpu_qrdqn_cases.py leans on them: both Huber branches
and both indicator values in every case, terminated rows, successors across the ring's end, rows near a ReLU kink and rows with close action values within their
caps in float64 alone, and the f32 restatement (torch stands in for the missing reference script; the expectation here is float64) within the device bounds."""
import numpy as np
import pytest

import _qrdqn_cases as K
import _qrdqn_ref as X


@pytest.fixture(scope="module")
def cases():
    return [K.make_case(i) for i in range(len(K.SHAPES))]


def test_cases_hold_what_they_claim(cases):
    assert {c["batch"] for c in cases} >= {1, 5, 129, 300} and {c["n_envs"] for c in cases} >= {1, 3} and min(c["slots"] for c in cases) == 2
    assert sum(c["terminated_rows"] for c in cases) > 0 and sum(c["wraps"] for c in cases) >= 2 * 4
    for c in cases:
        assert c["quadratic"] > 0 and c["linear"] > 0, c["batch"]                        # |u| <= kappa and |u| > kappa
        assert c["negative"] > 0 and c["non_negative"] > 0, c["batch"]                   # both values of the indicator u < 0
        assert c["idx"].max() < c["slots"] * c["n_envs"] and np.isfinite(c["grad"]).all() and np.abs(c["grad"]).max() > 0
        assert c["batch"] < 5 or (len(set(c["next_actions"].tolist())) == 2 and c["terminated_rows"] > 0 and c["wraps"] >= 2)
        assert K.holds(c)
    one = [c for c in cases if c["slots"] == 2][0]
    assert one["wraps"] == one["batch"] == 1                                             # slots = 2: the successor of the last slot is slot 0


def test_kink_and_close_value_rows_are_within_their_caps(cases):
    for c in cases:
        assert int(c["kink"].sum()) <= K.KINK_SHARE * c["batch"], (c["batch"], int(c["kink"].sum()))       # float64 alone; nothing is excluded for it
        assert int(c["close"].sum()) <= X.MAX_EXCLUDED * c["batch"], (c["batch"], int(c["close"].sum()))


def test_f32_restatement_is_within_the_device_bounds_on_the_cases(cases):
    """the cases sit in the regime the bounds were measured in: the f32 restatement, one more f32 evaluation, stays within the device bounds of float64"""
    for c in cases:
        total = c["slots"] * c["n_envs"]
        nxt = (c["idx"] + c["n_envs"]) % total
        fo = c["obs"].reshape(total, 4)
        na, tgt, q = X.target(c["target_params"], fo[nxt], c["rewards"].reshape(total)[nxt], c["term"].reshape(total)[nxt])
        far = ~c["close"]
        assert np.array_equal(na[far], c["next_actions"][far])
        same = na == c["next_actions"]
        assert np.abs(tgt - c["target"])[same].max() <= X.BOUND_TARGET_ABS and np.abs(q - c["q"]).max() <= X.BOUND_Q_ABS
        loss, g, cur = X.loss_grad(c["params"], fo[c["idx"]], c["actions"].reshape(total)[c["idx"]], c["target"])
        assert np.abs(cur - c["current"]).max() <= X.BOUND_QUANT_ABS
        assert abs(loss - c["loss"]) <= X.BOUND_LOSS_REL * abs(c["loss"]) and np.abs(g - c["grad"]).max() <= X.BOUND_GRAD_REL * np.abs(c["grad"]).max()
