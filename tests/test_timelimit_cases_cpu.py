"""The TimeLimit cases of tests/_timelimit_cases.py contain what they claim, and their expected values are sensitive to the rule (CPU only).

The GPU comparisons of tests/test_gpu_timelimit.py are exact, against the expectations built here.  This file shows (a) that every case holds the edges: truncations,
terminations at length exactly 500 and 499, an env truncated twice, a truncation on the first, a middle and the last step of a launch under every call schedule, short
episodes beside long ones in a DQN workgroup; and (b) that four plausible bugs of a kernel's TimeLimit code — `terminated := done`, a limit of 499 or 501, `elapsed`
not zeroed after a termination — each change the expected `terminated` flags and observations of every case, so the exact comparison on the GPU fails for them.

The 520-step case (n1030) cannot hold an env truncated twice (that takes 1,000 steps), nor a truncation on the first step of a call of 50 (step 500 would end an
episode of ONE step); every other condition is asserted for it too.

PPO's view (tests/test_gpu_timelimit_ppo.py: rollout_q4_kernel keeps `elapsed` in a register for a launch of T steps and carries it from launch to launch through the
env handle): Case.ppo_storage is what the oracle's own rollout leaves, launch after launch, at T = 7, 50, 128 (the longest launch whose LDS ring does not wrap) and 300;
five wrong rules — a limit of 499 or 501, `elapsed` surviving a termination, `elapsed` lost between launches, a truncation neither flagged nor reset — each change the
`dones` or observations the GPU test compares; the controller network decides as the rule; and the bounds for the device's log-probs and values are measured on the
oracle.  The launches are the floor(steps / T) whole ones (T.ppo_launches); 1,030 envs x 520 steps at T = 300 would be ONE launch in which nothing can be truncated, so
there one more launch takes the 220 steps that are left.
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
    term, obs, _done = T.restate(R, c, envs)
    assert np.array_equal(term, c.terminated[:, envs]) and np.array_equal(obs, c.obs[:, envs])      # the restatement of the true rule is the oracle's
    for label, kw in T.WRONG_RULES.items():
        wt, wo, _wd = T.restate(R, c, envs, **kw)
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


# ---- PPO's view of the cases --------------------------------------------------------------------------------------
PPO_NAMES = ("n5", "dqn37", "ppo64", "n1030")
PPO_T = (7, 50, 128, 300)


def test_ppo64_is_the_grid_it_claims():
    c = T.get("ppo64", False)
    assert c.n == 64 and (c.n // 4) % 8 == 0 and c.n // 4 < 32 and "ppo64" in T.NAMES      # 16 workgroups: the env-group map permutes; below MI_STATS_PART_MIN
    assert all(c.kinds[i] in T.LONG_KINDS for i in (0, 3, 60, 61, 62))


@pytest.mark.parametrize("Tn", PPO_T)
@pytest.mark.parametrize("forced", FORMS, ids=["keyed", "forced"])
@pytest.mark.parametrize("name", PPO_NAMES)
def test_ppo_storage_is_the_oracles_rollout(R, name, forced, Tn):
    """R.rollout, launch after launch from a fresh VecCartPole under the case's actions (and reset states), leaves exactly Case.ppo_storage, the carried observation,
    the fp64 state, the episode list and the statistics of the linear record"""
    c = T.get(name, forced)
    launches = T.ppo_launches(c.steps, Tn)
    assert launches[:c.steps // Tn] == [Tn] * (c.steps // Tn) and sum(launches) <= c.steps
    old = R.lib().ref_get_sincos_mode()
    R.set_sincos_mode("fdlibm")
    try:
        env = R.VecCartPole(c.n, seed=c.seed, env_id_base=c.base)
        obs_cur = env.reset()
        assert np.array_equal(obs_cur, c.obs[0])
        params = np.zeros(R.NPARAMS, np.float32)      # teacher-forced: the actions do not depend on the network
        g = 0
        for k in launches:
            st = R.Storage(k, c.n)
            fr = None if c.forced_resets is None else c.forced_resets[g:g + k]
            eps, cnt = R.rollout(env, params, st, obs_cur, forced_actions=c.actions[g:g + k], forced_resets=fr, max_ep=k * c.n)
            want = c.ppo_storage(g, k)
            for f in ("observations", "actions", "rewards", "dones"):
                live = ~want["unwritten"][f]
                assert np.array_equal(getattr(st, f)[live], want[f][live]), (g, f)
            g += k
            assert np.array_equal(obs_cur, c.obs[g]) and np.array_equal(env.state, c.state[g]), g
            assert sorted(eps, key=lambda e: (e[1], e[0])) == c.episodes(g - k, k) and [cnt] == c.stats(g - k, k)[:1], g
            ln = [e[3] for e in eps]
            assert [len(ln), sum(ln), max(ln) if ln else 0] == c.stats(g - k, k), g
    finally:
        R.set_sincos_mode(old)
    # phases: T = 50 and T = 7 are test_cases_contain_the_edges' schedules; the long launches hold at least two truncations, and at T = 128 every long episode spans
    # at least three launch boundaries (`elapsed` crosses from launch to launch three times on its way to the limit)
    inside = [(gg, e) for gg, e in c.truncation_steps() if gg < g]
    assert len(inside) >= 2, (name, Tn, inside)
    if Tn == 128:
        for gg, e in c.truncation_steps():
            first = gg - T.LIMIT + 1
            assert gg // Tn - first // Tn >= 3, (gg, e)
        at_limit = np.argwhere((c.fin_len >= T.LIMIT - 1) & c.done)
        assert len(at_limit) > len(c.truncation_steps()) and all(gg // Tn - (gg - c.fin_len[gg, e] + 1) // Tn >= 3 for gg, e in at_limit)


_RESTATED = {}


def _restated(R, name, forced, **kw):
    """T.restate on the long-episode envs of a case, kept: four of the five wrong rules do not depend on the launch length"""
    key = (name, forced, tuple(sorted(kw.items())))
    if key not in _RESTATED:
        c = T.get(name, forced)
        _RESTATED[key] = T.restate(R, c, _long_envs(c), **kw)
    return _RESTATED[key]


@pytest.mark.parametrize("Tn", PPO_T)
@pytest.mark.parametrize("forced", FORMS, ids=["keyed", "forced"])
@pytest.mark.parametrize("name", T.NAMES)
def test_ppo_expectations_are_sensitive_to_the_rule(R, name, forced, Tn):
    """each wrong rule changes the `dones` or the observations that ppo_storage hands out for the long-episode envs inside the launches run"""
    c = T.get(name, forced)
    envs = _long_envs(c)
    G = sum(T.ppo_launches(c.steps, Tn))
    _term, obs, done = _restated(R, name, forced)
    assert np.array_equal(done, c.done[:, envs]) and np.array_equal(obs, c.obs[:, envs])      # the restatement of the true rule is the oracle's
    rules = T.ppo_wrong_rules(Tn)
    assert set(rules) == set(T.PPO_WRONG_RULES) and len(rules) == 5 and "terminated := done" not in rules and rules["elapsed not carried across launches"] == dict(carry_every=Tn)
    for label, kw in rules.items():
        _wt, wo, wd = _restated(R, name, forced, **kw)
        assert not (np.array_equal(wd[:G], done[:G]) and np.array_equal(wo[:G + 1], obs[:G + 1])), (name, Tn, label)


def test_ppo_controller_decides_as_the_rule(R):
    """controller_ppo(50, 6) in float64: l_1 - l_0 = K tanh(tanh(c w . obs)), whose sign is the rule's wherever |w . obs| > 1e-6; everything else in the actor is zero,
    the critic is not"""
    c = T.get("dqn37", False)
    obs = c.obs[:-1][:, c.kinds == T.K0].reshape(-1, 4)
    p = T.controller_ppo(50, 6)
    assert p.shape == (9155,) and p.dtype == np.float32 and np.count_nonzero(p[:T.PPO_CRITIC]) == 4 + 1 + 2 and np.count_nonzero(p[T.PPO_CRITIC:]) > 4000
    assert p[320] == 1 and p[4480] == -3 and p[4480 + 64] == 3 and np.array_equal(p[0:4], np.float32(50) * T.RULE_W.astype(np.float32))
    logits, logp, val = T.ppo64(p, obs)
    d = logits[:, 1] - logits[:, 0]
    wo = obs.astype(np.float64) @ T.RULE_W
    assert np.abs(d - 6 * np.tanh(np.tanh(50 * wo))).max() <= 1e-5      # f32 storage of c w: exact here (1, 5, 50, 25); the f64 sums differ by rounding only
    far = np.abs(wo) > 1e-6
    assert far.mean() > 0.999 and np.array_equal(np.sign(d[far]), np.where(T.rule(obs)[far] == 1, 1.0, -1.0))
    assert np.abs(logp).max() <= 4.6 and val.max() - val.min() > 1e-3      # (the values are no constants)


def _ppo_oracle_distance(R, p, obs):
    logits = R.actor(p, obs)
    nl, _p, _ent = R.categorical(logits)
    _l64, logp64, v64 = T.ppo64(p, obs)
    return float(np.abs(nl - logp64).max()), float(np.abs(R.critic(p, obs) - v64).max())


def test_ppo_logprob_and_value_bounds_rest_on_the_oracle(R):
    """the oracle's f32 log-probs and values against the float64 forward, for the two parameter vectors of the GPU tests (default init plus noise on the scripted cases'
    observations; the controller on the observations of its own run): the recorded figures are what is measured here, and the device bounds follow from them"""
    noisy, ctrl = T.ppo_noisy_params(), T.controller_ppo()
    obs_a = np.concatenate([T.get(n, f).obs.reshape(-1, 4) for n in ("n5", "dqn37", "ppo64") for f in FORMS] + [T.get("n1030", False).obs[::7].reshape(-1, 4)])
    old = R.lib().ref_get_sincos_mode()
    R.set_sincos_mode("fdlibm")
    try:
        env = R.VecCartPole(5, seed=5, env_id_base=300); obs_cur = env.reset(); st = R.Storage(128, 5)
        rows = []
        for _ in range(9):
            R.rollout(env, ctrl, st, obs_cur)
            rows.append(st.observations.copy())
    finally:
        R.set_sincos_mode(old)
    obs_c = np.concatenate(rows).reshape(-1, 4)
    la, va = _ppo_oracle_distance(R, noisy, obs_a)
    lc, vc = _ppo_oracle_distance(R, ctrl, obs_c)
    print("log-prob distance: noisy %.3e controller %.3e; value distance: noisy %.3e controller %.3e" % (la, lc, va, vc))
    logp, val = max(la, lc), max(va, vc)
    assert 0.5 * T.MEASURED_PPO_LOGP <= logp <= T.MEASURED_PPO_LOGP and 0.5 * T.MEASURED_PPO_VALUE <= val <= T.MEASURED_PPO_VALUE, (logp, val)
    bl, bv = T.ppo_bounds()
    assert bl == max(3e-6, 8 * T.MEASURED_PPO_LOGP) and bv == max(3e-6, 8 * T.MEASURED_PPO_VALUE) and bl < 1e-4 and bv < 1e-4
