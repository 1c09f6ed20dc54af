"""The conditions tests/test_gpu_eval.py rests on, shown on the float64 reference alone (tests/_eval_ref.py): for every network, seed and episode those tests use.
No GPU: the oracle steps the env bit for bit as the device does, the action values are the project's float64 restatements."""
import numpy as np
import pytest

import _eval_ref as E
import _timelimit_cases as T


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


def test_constants_are_the_first_from_one_upwards():
    assert E.SEED == 1 and E.EPISODES == (1, 5, 37) and E.E_MAX == 37 and E.ENV_BASE == 1 << 40
    assert set(E.NET_SEEDS) == set(E.KINDS) == set(E.CONTROLLERS) == set(E.NREAD)
    assert E.MAX_EXCLUDED == 0.01 and T.CONTROLLER_K == 16.0
    assert E.close("dueling") == 1e-4 and E.KINDS == ("dueling", "qr", "c51", "rainbow") and [E.KIND_ID[k] for k in E.KINDS] == [1, 2, 3, 4]
    import _c51_ref, _qrdqn_ref, _rainbow_ref
    assert E.close("c51") == _c51_ref.CLOSE_Q and E.close("qr") == _qrdqn_ref.CLOSE_Q and E.close("rainbow") == _rainbow_ref.CLOSE_Q["off"]


@pytest.mark.parametrize("kind", E.KINDS)
def test_every_controller_episode_reaches_the_limit_with_clear_decisions(kind):
    """500 steps, truncated, both actions — and the float64 gap reaches the family's close-value distance at all but at most 1 % of the steps, overall and in each
    of the prefixes E = 1, 5, 37 the GPU tests compare"""
    eps = E.reference_run("controller", kind)
    assert len(eps) == E.E_MAX
    for o in eps:
        assert o["length"] == 500 and o["truncated"] == 1 and o["ret"] == 500.0
        assert set(o["actions"].tolist()) == {0, 1}
        assert np.array_equal(o["actions"], o["greedy"])
    for n in E.EPISODES:
        gaps = np.concatenate([o["gaps"] for o in eps[:n]])
        left_out = float((gaps < E.close(kind)).mean())
        assert left_out <= E.MAX_EXCLUDED, (kind, n, left_out)


@pytest.mark.parametrize("kind", E.KINDS)
def test_every_default_init_episode_is_short_and_both_actions_occur(kind, R):
    eps = E.reference_run("default", kind)
    assert max(o["length"] for o in eps) < E.SHORT
    assert all(o["truncated"] == 0 and o["ret"] == float(o["length"]) for o in eps)
    assert set(np.concatenate([o["actions"] for o in eps]).tolist()) == {0, 1}
    # the seed is the first from 1 upwards that gives both: every smaller one runs past SHORT or repeats one action
    envs = [E.ENV_BASE + e for e in range(E.E_MAX)]
    for s in range(1, E.NET_SEEDS[kind]):
        d = E.run_episodes(R, E.default_params(kind, s), kind, E.SEED, envs)
        both = set(np.concatenate([o["actions"] for o in d]).tolist()) == {0, 1}
        assert max(o["length"] for o in d) >= E.SHORT or not both, (kind, s)


def test_the_builders_give_what_the_kinds_read():
    for kind in E.KINDS:
        for p in (E.controller(kind), E.default_params(kind)):
            assert p.dtype == np.float32 and p.size >= E.NREAD[kind] and np.isfinite(p).all()
    assert E.default_params("dueling").size == 11274 and E.default_params("rainbow").size == E.controller("rainbow").size == 36774
    assert not E.controller("rainbow")[23769:].any()
    # the QR controller's quantile mean gives q_1 - q_0 = K (w . obs) as the dueling controller does (both float64; they differ by the order of their sums
    # alone: a few ulps of values below 32, i.e. below 1e-13)
    x = E.reachable_box(np.random.default_rng(3), 64)
    dq, dd = E.q64("qr", E.controller("qr"), x), E.q64("dueling", E.controller("dueling"), x)
    assert np.abs((dq[:, 1] - dq[:, 0]) - (dd[:, 1] - dd[:, 0])).max() < 1e-13 and np.abs(dd[:, 1] - dd[:, 0]).max() < 32


def test_the_scripts_hold_every_ending(R):
    """rule: truncated at 500; rule then 0 from 490 / rule then 1 from 489: the pole falls on step 498, 499 or exactly on step 500 (terminated, NOT truncated);
    random: short episodes"""
    res = {name: E.scripts(name)[1] for name, _ in E.SCRIPTS}
    assert all(r == dict(length=500, ret=500.0, truncated=1) for r in res["rule"])
    late = res["rule_then_0_from_490"] + res["rule_then_1_from_489"]
    assert all(r["truncated"] == 0 and 490 < r["length"] <= 500 for r in late)
    assert {r["length"] for r in late} >= {499, 500}
    assert all(r["truncated"] == 0 and r["length"] < 100 for r in res["random"]) and len({r["length"] for r in res["random"]}) > 3
    acts = E.scripts("rule_then_1_from_489")[0]
    assert acts.shape == (E.SCRIPT_EPISODES, 500) and acts.dtype == np.uint8 and set(np.unique(acts)) == {0, 1}
    # a script replayed through run_episodes gives the script's own result (the network is evaluated, its action overridden)
    o = E.run_episode(R, E.default_params("dueling"), "dueling", E.SEED, E.ENV_BASE + 2, forced_actions=E.scripts("rule_then_0_from_490")[0][2])
    assert (o["length"], o["truncated"]) == (res["rule_then_0_from_490"][2]["length"], res["rule_then_0_from_490"][2]["truncated"])


def test_forced_starts_on_the_reference(R):
    """a start one step from the x threshold and moving out ends on step 1; the upright start at rest under the rule never leaves"""
    out = np.array([2.39, 1.0, 0.0, 0.0])
    with T._Mode(R):
        s, term = R.cartpole_step(out, 0)
    assert term and s[0] > 2.4
    o = E.run_episode(R, E.controller("dueling"), "dueling", E.SEED, E.ENV_BASE, forced_start=out)
    assert o["length"] == 1 and o["truncated"] == 0
    o = E.run_episode(R, E.controller("dueling"), "dueling", E.SEED, E.ENV_BASE, forced_start=np.array([0.0, 0.0, 0.01, 0.0]))
    assert o["length"] == 500 and o["truncated"] == 1
