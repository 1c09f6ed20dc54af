"""The TimeLimit cases of tests/_timelimit_cases.py contain what they claim, and their expected values are sensitive to the rule (CPU only).

The GPU comparisons of tests/test_gpu_timelimit.py are exact, against the expectations built here.  This file shows (a) that every case holds the edges: truncations,
terminations at length exactly 500 and 499, an env truncated twice, a truncation on the first, a middle and the last step of a launch under every call schedule, short
episodes beside long ones in a DQN workgroup; and (b) that four plausible bugs of a kernel's TimeLimit code — `terminated := done`, a limit of 499 or 501, `elapsed`
not zeroed after a termination — each change the expected `terminated` flags and observations of every case, so the exact comparison on the GPU fails for them.

The 520-step case (n1030) cannot hold an env truncated twice (that takes 1,000 steps), nor a truncation on the first step of a call of 50 (step 500 would end an
episode of ONE step); every other condition is asserted for it too.
"""
import numpy as np
import pytest

import _timelimit_cases as T

FORMS = (False, True)


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


def _long_envs(case):
    return [int(i) for i in np.flatnonzero(np.isin(case.kinds, T.LONG_KINDS))]


@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("name", T.NAMES)
def test_cases_contain_the_edges(R, name, forced):
    c = T.get(name, forced)
    envs = T.SHARED_1030 if name == "n1030" else None     # the 1,030-env case must hold its edges among the twelve envs that share a workgroup
    k = c.counts(envs)
    print(name, "forced" if forced else "keyed", c.counts(), "shared" if envs else "", k if envs else "")
    assert k["truncations"] >= 2 and k["terminated_at_500"] >= 1 and k["terminated_at_499"] >= 1
    if c.steps >= 2 * T.LIMIT:
        assert k["envs_truncated_twice"] >= 1
    for sched in T.SCHEDULES:
        assert max(T.calls(sched, c.steps)) <= 64 and sum(T.calls(sched, c.steps)) == c.steps
        want = {"first", "middle", "last"}
        if c.steps < 2 * T.LIMIT and sched == "50":
            want = {"middle", "last"}                     # (see the module docstring)
        assert want <= c.phases(sched), (sched, c.phases(sched), c.truncation_steps())
    # the kind-2 envs with a chosen start: their balanced episode begins there and is truncated 500 steps later
    for i, start in c.starts.items():
        assert c.done[start - 1, i] and c.trunc[start + T.LIMIT - 1, i] and c.fin_len[start + T.LIMIT - 1, i] == T.LIMIT
    # a truncation stores terminated = 0, return 500.0 and length 500, and the RESET observation in the successor slot
    for g, e in c.truncation_steps():
        assert c.terminated[g, e] == 0 and c.fin_ret[g, e] == 500.0 and c.fin_len[g, e] == T.LIMIT and c.elapsed[g + 1, e] == 0 and np.abs(c.obs[g + 1, e]).max() <= 0.05
        assert c.elapsed[g, e] == T.LIMIT - 1
    at500 = (c.terminated == 1) & (c.fin_len == T.LIMIT)
    assert not c.trunc[at500].any() and (c.elapsed[:-1][at500] == T.LIMIT - 1).all()
    if c.forced:
        assert (c.forced_resets[~c.done] == 0).all() and np.abs(c.forced_resets).max() <= 0.05 and (np.abs(c.forced_resets[c.done]).max(-1) > 0).all()
    else:
        assert c.forced_resets is None


@pytest.mark.parametrize("forced", FORMS)
def test_dqn_workgroups_mix_short_and_long_episodes(forced):
    """in each 16-env workgroup of the DQN case a short episode finishes inside the lifetime of an episode that reaches the limit, and the corner positions 0, 15,
    16 and 36 are long-episode envs"""
    c = T.get("dqn37", forced)
    assert all(c.kinds[i] in T.LONG_KINDS for i in (0, 15, 16, 36)) and c.n % 16 != 0
    for w in range((c.n + 15) // 16):
        envs = np.arange(16 * w, min(16 * w + 16, c.n))
        hit = False
        for g, e in zip(*np.nonzero((c.fin_len[:, envs] >= T.LIMIT - 1))):
            lo = g - c.fin_len[g, envs[e]] + 1
            short = c.done[lo:g, envs] & (c.fin_len[lo:g, envs] < 100)
            hit |= bool(short.any())
        assert hit, w


@pytest.mark.parametrize("name", T.NAMES)
def test_ring_view_is_the_oracles_acting_loop(R, name):
    """Case.ring / episodes / stats against R.dqn_act_steps_log itself, run in calls of 50 on a 16-slot ring (which wraps) and on a ring that holds the run"""
    c = T.get(name, True)
    for slots in (16, c.steps + 1):
        env = R.VecCartPole(c.n, seed=c.seed, env_id_base=c.base); st = R.ReplayStorage(slots, c.n)
        old = R.lib().ref_get_sincos_mode()
        R.set_sincos_mode("fdlibm")
        try:
            obs_cur = env.reset(); st.observations[0] = obs_cur
            g = 0
            for k in T.calls("50", c.steps):
                eps, cnt = R.dqn_act_steps_log(env, np.zeros(R.DQN_NPARAMS, np.float32), st, obs_cur, k, g, forced_actions=c.actions[g:g + k],
                                               forced_resets=c.forced_resets[g:g + k], max_ep=8192)
                assert [(e, s, r, l) for e, s, r, l in eps] == c.episodes(g, k) and cnt == c.stats(g, k)[0]
                g += k
                if slots == 16 or g == c.steps:
                    want = c.ring(g, slots)
                    for f in ("observations", "actions", "rewards", "terminated"):
                        assert np.array_equal(getattr(st, f), want[f]), (g, f)
                assert np.array_equal(obs_cur, c.obs[g]) and np.array_equal(env.state, c.state[g])
        finally:
            R.set_sincos_mode(old)


@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("name", T.NAMES)
def test_expectations_are_sensitive_to_the_rule(R, name, forced):
    c = T.get(name, forced)
    envs = _long_envs(c)
    assert set(T.SHARED_1030) <= set(envs) or name != "n1030"
    # the envs left out never come near the limit: whatever the rule, their flags are their terminations
    rest = np.setdiff1d(np.arange(c.n), envs)
    assert (c.fin_len[:, rest][c.done[:, rest]] < T.LIMIT - 50).all() if len(rest) else True
    term, obs = T.restate(R, c, envs)
    assert np.array_equal(term, c.terminated[:, envs]) and np.array_equal(obs, c.obs[:, envs])      # the restatement of the true rule is the oracle's
    for label, kw in T.WRONG_RULES.items():
        wt, wo = T.restate(R, c, envs, **kw)
        # `terminated := done` moves no state: it shows in the flags; the other three move a reset, which shows in the observations (and in the flags wherever the
        # displaced episode ends by termination inside the run)
        assert not np.array_equal(wt, term) if label == "terminated := done" else not np.array_equal(wo, obs), (name, label)


@pytest.mark.parametrize("algo", sorted(T.CONTROLLERS))
def test_controller_networks_decide_as_the_rule(R, algo):
    """the hand-built networks: q_1 - q_0 = K (w . obs) in float64, so the greedy action is the balancing rule's, and at CONTROLLER_K fewer than 1 % of the decisions
    of a balanced run lie inside the algorithm's close-value distance"""
    c = T.get("dqn37", False)
    obs = c.obs[:-1][:, c.kinds == T.K0].reshape(-1, 4)
    p = T.CONTROLLERS[algo](T.CONTROLLER_K)
    q = T.q64(algo, p, obs)
    d = q[:, 1] - q[:, 0]
    wo = obs.astype(np.float64) @ T.RULE_W
    if algo != "c51":
        assert np.abs(d - T.CONTROLLER_K * wo).max() <= 1e-6 * T.CONTROLLER_K      # f32 storage of w: 4 products of <= 6e-8 relative, |obs| of a balanced run < 3
    far = np.abs(d) >= T.close_q(algo)
    print(algo, "decisions", len(d), "inside close_q", int((~far).sum()))
    assert (~far).mean() < 0.01 / 2
    w32 = T.RULE_W.astype(np.float32).astype(np.float64)
    assert np.array_equal((d > 0)[far], (obs.astype(np.float64) @ w32 > 0)[far])
    assert np.count_nonzero(p) <= 16 + (64 if algo == "iqn" else 0)      # (IQN: the 64 embedding biases are 1)
