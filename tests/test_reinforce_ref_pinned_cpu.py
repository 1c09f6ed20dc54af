"""The numpy restatement of REINFORCE (tests/_reinforce_ref.py) pinned to the UNMODIFIED reference reinforce.py (tests/golden/reinforce_ref_trace.npz, written by
tools/capture_reinforce_ref.py): env replay exact, and — each from the REFERENCE's inputs of that update, never chained — log-probs, normalised returns,
policy loss and gradients of all 100 updates; Adam chained over the reference's own gradient sequence.

Gradient -> Adam -> next gradient is deliberately NOT replayed as a chain: 224-357 of the 898 gradient elements are exactly 0 in an update (units dropped or
inactive on every row) and with eps = 1e-8 Adam turns rounding noise on those into steps of size lr (REINFORCE section).

Bounds are 4 x what this restatement measures against the fixture (the observed value stands beside each)."""
import numpy as np
import pytest

import _reinforce_ref as P
from oracle import cpu_ref as R


@pytest.fixture(scope="module")
def trace():
    return P.load_trace()


def test_fixture_shape(trace):
    t = trace
    assert len(t["lengths"]) == 100 and int(t["lengths"].sum()) == 7706 == len(t["actions"]) == len(t["obs"])
    assert t["init_params"].shape == (898,) and t["grads"].shape == t["params_after"].shape == (100, 898)
    assert int(t["lengths"].min()) == 13 and int(t["lengths"].max()) == 349
    assert np.array_equal(t["episode_global_step"], np.cumsum(t["lengths"])) and np.array_equal(t["episode_return"], t["lengths"].astype(np.float32))
    assert all(v.dtype.kind in "fiub" for v in t.values())
    keep = t["masks"].mean()
    assert abs(keep - 0.4) < 5 * np.sqrt(0.24 / t["masks"].size), keep   # torch's own dropout: 986,368 bits


def test_vectorised_philox_is_the_oracles():
    for s, e, i, st in [(1, 0, 0, 8), (1, 4095, 123456, 8), (2 ** 40 + 7, 3, 2 ** 33 + 5, 1), (7, 2 ** 35, 9, 0)]:
        assert np.array_equal(P.philox(s, e, i, st).reshape(4), R.philox(s, e, i, st))
    for step in (0, 1, 5, 2 ** 34 + 3):
        assert float(P.action_uniforms(3, 17, [step])[0]) == R.action_uniform(3, 17, step)
    M = P.keyed_masks(1, 0, np.arange(10000))
    assert abs(M.mean() - 0.4) < 5 * np.sqrt(0.24 / M.size)
    assert np.array_equal(P.words_to_masks(P.mask_words(M)), M)


@pytest.mark.parametrize("mode", ["libm", "fdlibm"])
def test_env_replay_is_exact_on_every_step(trace, mode):
    """the oracle stepper, teacher-forced with the reference's reset states and actions: all 7,706 observations and done flags, none left out"""
    R.set_sincos_mode(mode)
    try:
        total = 0
        for e in range(100):
            ep = P.episode(trace, e)
            obs, term, done, trunc = P.replay_episode(ep["reset"], ep["A"])
            assert len(obs) == ep["length"] and done[-1] and not done[:-1].any()
            assert np.array_equal(obs, ep["obs_after"]) and np.array_equal(term, ep["terminated"].astype(bool))
            total += len(obs)
        assert total == 7706
    finally:
        R.set_sincos_mode("libm")


def test_unchained_log_probs_returns_loss_and_gradients(trace):
    worst = dict(rn=0.0, lp=0.0, loss=0.0, g32=0.0, g64=0.0)
    for e in range(100):
        ep = P.episode(trace, e)
        n = ep["length"]
        _, Rn = P.returns_normalised(n)
        worst["rn"] = max(worst["rn"], float(np.abs(Rn - ep["b_returns"]).max()))
        _p, lp, _h = P.forward(ep["params"], ep["X"], ep["M"])
        lpa = lp[np.arange(n), ep["A"]]
        worst["lp"] = max(worst["lp"], float(np.abs(lpa - ep["b_log_probs"]).max()))
        terms = -lpa.astype(np.float64) * Rn.astype(np.float64)
        worst["loss"] = max(worst["loss"], abs(terms.sum() - ep["policy_loss"]) / np.abs(terms).sum())
        scale = np.abs(ep["grads"]).max()
        worst["g32"] = max(worst["g32"], float(np.abs(P.grad(ep["params"], ep["X"], ep["A"], ep["M"], ep["b_returns"]) - ep["grads"]).max() / scale))
        worst["g64"] = max(worst["g64"], float(np.abs(P.grad(ep["params"], ep["X"], ep["A"], ep["M"], ep["b_returns"], np.float64) - ep["grads"]).max() / scale))
    print("worst over 100 updates:", worst)
    assert worst["rn"] <= 4 * 7.2e-7      # observed 7.2e-7 absolute (backward recurrence vs the reference's O(T^2) accumulation)
    assert worst["lp"] <= 4 * 7.2e-7      # observed 7.2e-7 absolute
    assert worst["loss"] <= 4 * 4.2e-7    # observed 4.2e-7 of sum |log_prob * Rn| (the loss itself is a cancelling sum)
    assert worst["g32"] <= 4 * 4.4e-7     # observed 4.3e-7 of max |g|, f32
    assert worst["g64"] <= 4 * 4.4e-7     # observed 4.3e-7 of max |g|, f64 (the reference itself is f32)


def test_adam_chained_on_the_references_gradients(trace):
    p = trace["init_params"].copy(); m = np.zeros_like(p); v = np.zeros_like(p)
    worst = 0.0
    for e in range(100):
        P.adam_step(p, trace["grads"][e], m, v, e + 1)
        worst = max(worst, float(np.abs(p - trace["params_after"][e]).max()))
    print("adam chained, worst abs", worst)
    assert worst <= 4 * 1.8e-7            # observed 1.8e-7 absolute over 100 chained steps


def test_zero_gradient_elements_make_the_chain_ill_conditioned(trace):
    """the note in DESIGN.md: hundreds of exactly-zero gradient elements per update"""
    zeros = (trace["grads"] == 0).sum(axis=1)
    assert zeros.min() >= 100 and zeros.max() <= 600, (zeros.min(), zeros.max())
