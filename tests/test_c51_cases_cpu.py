"""The synthetic C51 cases (tests/_c51_cases.py) are what they claim to be — on the CPU, before tests/test_gpu_c51_cases.py leans on them: every branch of the
projection is reached, rows near a ReLU kink and rows with close action values are at most 1 % of a case, and the f32 restatement agrees with the float64
expectation within the device bounds."""
import numpy as np
import pytest

import _c51_cases as K
import _c51_ref as X


@pytest.fixture(scope="module")
def cases():
    return [K.make_case(i) for i in range(len(K.SHAPES))]


def test_branches_are_reached(cases):
    assert sum(c["clamped_low"] for c in cases) > 0 and sum(c["clamped_high"] for c in cases) > 0          # the clamp of c51.py:135, never active in the reference's run
    assert sum(c["integral"] for c in cases) > 0 and sum(c["fractional"] for c in cases) > 0                # both sides of (l == u) (:149)
    assert sum(c["terminated_rows"] for c in cases) > 0 and sum(c["wraps"] for c in cases) >= 2 * 4         # the 101-fold collision; successors across the ring's end
    assert {c["batch"] for c in cases} >= {1, 129, 300} and max(c["n_envs"] for c in cases) >= 3 and min(c["slots"] for c in cases) == 2
    for c in cases:
        assert c["b"].min() >= 0 and c["b"].max() <= 100 and c["idx"].max() < c["slots"] * c["n_envs"]
        assert np.abs(c["target_probs"].sum(-1) - 1).max() < 1e-12 and np.isfinite(c["grad"]).all() and np.abs(c["grad"]).max() > 0
        assert len(set(c["next_actions"].tolist())) == 2 or c["batch"] < 5              # both greedy actions occur


def test_kink_and_close_value_rows_are_rare(cases):
    for c in cases:
        assert int(c["kink"].sum()) <= K.KINK_SHARE * c["batch"], (c["batch"], int(c["kink"].sum()))       # float64 alone; nothing is excluded for it
        assert int(c["close"].sum()) <= X.MAX_EXCLUDED * c["batch"], (c["batch"], int(c["close"].sum()))


def test_f32_restatement_meets_the_measured_figures_on_the_cases(cases):
    """the cases sit in the regime the bounds were measured in: the f32 restatement, one more f32 evaluation, stays within the device bounds of float64"""
    for c in cases:
        total = c["slots"] * c["n_envs"]
        nxt = (c["idx"] + c["n_envs"]) % total
        fo = c["obs"].reshape(total, 4)
        na, m, q = X.target(c["target_params"], fo[nxt], c["rewards"].reshape(total)[nxt], c["term"].reshape(total)[nxt])
        far = ~c["close"]
        assert np.array_equal(na[far], c["next_actions"][far])
        same = na == c["next_actions"]
        assert np.abs(m - c["target_probs"])[same].max() <= X.BOUND_TARGET_PROBS_ABS and np.abs(q - c["q"]).max() <= X.BOUND_Q_ABS
        loss, g, p = X.loss_grad(c["params"], fo[c["idx"]], c["actions"].reshape(total)[c["idx"]], c["target_probs"])
        assert np.abs(p - c["probs"]).max() <= X.BOUND_PROBS_ABS
        assert abs(loss - c["loss"]) <= X.BOUND_LOSS_REL * abs(c["loss"]) and np.abs(g - c["grad"]).max() <= X.BOUND_GRAD_REL * np.abs(c["grad"]).max()
