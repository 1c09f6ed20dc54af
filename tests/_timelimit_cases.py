"""Teacher-forced cases that drive the acting kernels (dqn_act4_kernel, c51_act_kernel, iqn_act_kernel) into CartPole's 500-step TimeLimit — TEST INFRASTRUCTURE.

Everything here runs on the CPU oracle (oracle/cpu_ref.py) in its device-matched sin/cos mode.  `Sim` steps a `VecCartPole` one action row at a time and keeps the
LINEAR record of the run: obs[g] / state[g] / elapsed[g] in front of step g, action / done / truncated / terminated / finished return and length of step g.  A
`Case` answers from that record what an engine must hold after any number of steps on any ring (`ring`), and what one call must report (`episodes`, `stats`).

Scripts.  Every env follows a script keyed on its OWN episode step counter; the balancing rule is the one of tests/test_gpu_parity.py's
test_env_step_bit_exact_with_truncation, evaluated in float64 on the f32 observation: a = (theta + 0.5 theta_dot + 0.02 x + 0.1 x_dot) > 0.
  kind 0  the rule throughout: truncated at 500 and again 500 steps after every reset
  kind 1  the rule, then action 0 from episode step 490 (variant 1a)
  kind 4  the rule, then action 1 from episode step 489 (variant 1b): between them the pole falls on step 499 or exactly on step 500 (terminated = 1, no truncation)
  kind 2  random actions while global step < switch[env], then the rule: truncations out of phase with the other envs and with the call boundaries
  kind 3  random actions throughout: short episodes beside the long ones
CartPole's Euler step makes the successor's x and theta independent of that step's action, so "terminates or truncates on the limit step" is decided one step
EARLIER: kinds 0 and 1 / 4 differ only in their last ten actions.

Phases.  A truncation must fall on the first, a middle and the last step of a launch under each of the three call schedules (SCHEDULES).  Kind 0 truncates on steps
499 and 999 (0-based): the last step of calls of 50, the first of 49-then-50s, a middle one of calls of 7.  The other phases come from kind-2 envs whose balanced
episode starts at a chosen global step: for such an env the builder walks the sub-seeds of its random action stream until one ends an episode exactly in front of
that step (`_find_subseed`).  With 1,100 steps, starts 51 and 99 give everything else: 51 -> steps 550 (first of a 50-call, middle of 49+50s) and 1050 (first of a
7-call); 99 -> steps 598 (last of a 49+50s call, middle of a 50-call) and 1098 (last of a 7-call).
The 520-step case (1,030 envs) cannot hold an env that is truncated twice, nor a truncation on the first step of a 50-call (step 500: an episode of one step);
tests/test_timelimit_cases_cpu.py asserts every other condition for it.

PPO (tests/test_gpu_timelimit_ppo.py).  rollout_q4_kernel keeps `elapsed` in a register for a launch of T steps and carries it from launch to launch through the env
handle.  `Case.ppo_storage` is what the (T + 1, N) storage must hold after the launch that runs steps g0 ... g0 + T - 1; `ppo_launches` the launch lengths of a case
at a given T; `PPO_WRONG_RULES` the ways that copy of the rule can be wrong (restate: `carry_every`, `truncate`); `controller_ppo` an ActorCritic vector whose
stochastic policy balances the pole; `ppo64` the float64 forward; `MEASURED_PPO_*` the oracle's own f32 distance from it, from which the device bounds follow.
The case "ppo64" (64 envs) is PPO's grid of 16 four-env workgroups, a multiple of 8, on which the XCD-aware env-group map permutes.
"""
import functools

import numpy as np

LIMIT = 500
SCHEDULES = ("50", "7", "49+50")
RULE_W = np.array([0.02, 0.1, 1.0, 0.5])   # (x, x_dot, theta, theta_dot)
K0, K1A, K2, K3, K1B = 0, 1, 2, 3, 4
LONG_KINDS = (K0, K1A, K1B, K2)


def calls(schedule, steps):
    """the call lengths of a schedule over `steps` steps (each <= 64, the acting launches' limit); the last call takes what is left"""
    out = [49] if schedule == "49+50" else []
    k = 7 if schedule == "7" else 50
    while sum(out) < steps:
        out.append(min(k, steps - sum(out)))
    return out


def rule(obs):
    return (np.asarray(obs, np.float32).astype(np.float64) @ RULE_W > 0).astype(np.int64)


class _Mode:
    """the oracle's device-matched sin/cos inside, whatever was set before outside"""

    def __init__(self, R):
        self.R = R

    def __enter__(self):
        self.old = self.R.lib().ref_get_sincos_mode()
        self.R.set_sincos_mode("fdlibm")

    def __exit__(self, *a):
        self.R.set_sincos_mode(self.old)


class Sim:
    """a VecCartPole stepped row by row, keeping the linear record.  forced_table: None (keyed resets) or f64 [n][episodes][4], the state env i is reset to behind its
    k-th finished episode (k = 0 ...)."""

    def __init__(self, R, n, seed, base, forced_table=None):
        self.R, self.n, self.seed, self.base, self.forced_table = R, n, seed, base, forced_table
        self.env = R.VecCartPole(n, seed=seed, env_id_base=base)
        self.obs, self.state, self.elapsed = [], [], []
        self.actions, self.done, self.trunc, self.fin_ret, self.fin_len, self.forced_rows = [], [], [], [], [], []
        self.finished = np.zeros(n, np.int64)
        self.g = 0

    def reset(self):
        """env.reset() for all envs, as the engines' reset(): the observation in front of the next step is replaced, the TimeLimit counters start again"""
        with _Mode(self.R):
            o = self.env.reset()
        if self.g == len(self.obs):
            self.obs.append(None); self.state.append(None); self.elapsed.append(None)
        self.obs[self.g] = o.copy(); self.state[self.g] = self.env.state.copy(); self.elapsed[self.g] = np.zeros(self.n, np.int32)
        return o

    def step(self, a):
        a = np.asarray(a, np.int64)
        fr = None
        if self.forced_table is not None:
            fr = self.forced_table[np.arange(self.n), self.finished]
        with _Mode(self.R):
            o, _rew, d, tr, fret, flen = self.env.step(a, fr)
        d = d.astype(bool)
        self.actions.append(a.copy()); self.done.append(d); self.trunc.append(tr.astype(bool)); self.fin_ret.append(fret); self.fin_len.append(flen)
        self.forced_rows.append(None if fr is None else np.where(d[:, None], fr, 0.0))
        self.finished += d
        self.g += 1
        self.obs.append(o.copy()); self.state.append(self.env.state.copy())
        self.elapsed.append(np.where(d, 0, self.elapsed[-1] + 1).astype(np.int32))
        return o

    def case(self, **meta):
        return Case(self, **meta)


class Case:
    def __init__(self, sim, **meta):
        self.n, self.seed, self.base, self.steps = sim.n, sim.seed, sim.base, sim.g
        self.forced, self.forced_table = sim.forced_table is not None, sim.forced_table
        self.obs, self.state, self.elapsed = np.stack(sim.obs), np.stack(sim.state), np.stack(sim.elapsed)       # [steps + 1]
        self.actions, self.done, self.trunc = np.stack(sim.actions), np.stack(sim.done), np.stack(sim.trunc)     # [steps]
        self.terminated = (self.done & ~self.trunc).astype(np.uint8)                                              # reference: done and not info["TimeLimit.truncated"]
        self.fin_ret, self.fin_len = np.stack(sim.fin_ret), np.stack(sim.fin_len)
        self.forced_resets = np.stack(sim.forced_rows) if self.forced else None                                   # f64 [steps][n][4], zeros where no episode ends
        self.kinds = meta.pop("kinds", None)
        self.switch = meta.pop("switch", None)
        self.__dict__.update(meta)

    # ---- what an engine holds after G steps -----------------------------------------------------------------
    def ring(self, G, slots):
        """the four replay tensors after G steps on a `slots`-slot ring that was zero before reset(): the action of step g lies in slot g % slots; the successor
        observation, the reward and `terminated` in slot (g + 1) % slots; reset() wrote its observation into slot 0"""
        n = self.n
        obs = np.zeros((slots, n, 4), np.float32); act = np.zeros((slots, n), np.int64); rew = np.zeros((slots, n), np.float32); term = np.zeros((slots, n), np.uint8)
        lo = max(0, G - slots + 1)
        idx = np.arange(lo, G + 1)                      # the observation indices still in the ring
        obs[idx % slots] = self.obs[idx]
        w = idx[idx >= 1]
        rew[w % slots] = 1.0
        term[w % slots] = self.terminated[w - 1]
        # observation index 0 (reset) never carried a reward; a slot whose newest entry is index 0 keeps zeros
        ga = np.arange(max(0, G - slots), G)
        act[ga % slots] = self.actions[ga]
        return dict(observations=obs, actions=act, rewards=rew, terminated=term)

    def ppo_storage(self, g0, T):
        """what PPO's (T + 1, N) storage must hold after the rollout that runs steps g0 ... g0 + T - 1 (ppo.py:113-141): observations[r] = obs[g0 + r] (the row behind a
        done step holds the RESET observation), actions[r] = the action of step g0 + r, rewards[r] = 1 and dones[r] = done[g0 + r - 1] for r >= 1 — PPO stores `done`,
        truncations included, not `terminated`.  `unwritten`: per tensor the (T + 1,) mask of the rows a launch never writes (rewards[0], dones[0], actions[T],
        log_probs[T], as tests/test_gpu_poison.py has it); the values given here for those rows mean nothing"""
        n = self.n
        act = np.zeros((T + 1, n), np.int64); rew = np.zeros((T + 1, n), np.float32); dn = np.zeros((T + 1, n), np.float32)
        act[:T] = self.actions[g0:g0 + T]
        rew[1:] = 1.0
        dn[1:] = self.done[g0:g0 + T]
        first = np.arange(T + 1) == 0; last = np.arange(T + 1) == T; none = np.zeros(T + 1, bool)
        return dict(observations=self.obs[g0:g0 + T + 1].copy(), actions=act, rewards=rew, dones=dn,
                    unwritten=dict(observations=none, values=none, actions=last, log_probs=last, rewards=first, dones=first))

    def episodes(self, g0, k):
        """the episode log of the call that runs steps g0 ... g0 + k - 1: [(env, step in call, return, length)] in (step, env) order"""
        out = []
        for s in range(k):
            for e in np.flatnonzero(self.done[g0 + s]):
                out.append((int(e), s, float(self.fin_ret[g0 + s, e]), int(self.fin_len[g0 + s, e])))
        return out

    def stats(self, g0, k):
        """{finished episodes, sum of their lengths, longest} of that call"""
        d = self.done[g0:g0 + k]
        ln = self.fin_len[g0:g0 + k][d]
        return [int(d.sum()), int(ln.sum()), int(ln.max()) if ln.size else 0]

    # ---- what the case contains -----------------------------------------------------------------------------
    def truncation_steps(self):
        """[(global step, env)] of every truncation"""
        return [(int(g), int(e)) for g, e in zip(*np.nonzero(self.trunc))]

    def counts(self, envs=None):
        sel = np.ones(self.n, bool) if envs is None else np.isin(np.arange(self.n), envs)
        tr = self.trunc[:, sel]
        term = (self.terminated[:, sel] == 1)
        ln = self.fin_len[:, sel]
        return dict(truncations=int(tr.sum()), terminated_at_500=int((term & (ln == LIMIT)).sum()), terminated_at_499=int((term & (ln == LIMIT - 1)).sum()),
                    envs_truncated_twice=int((tr.sum(0) >= 2).sum()), short_episodes=int((term & (ln < LIMIT - 1)).sum()))

    def phases(self, schedule):
        """the set of {"first", "middle", "last"} positions in a call at which a truncation falls under `schedule`"""
        pos, g0 = {}, 0
        for k in calls(schedule, self.steps):
            for s in range(k):
                pos[g0 + s] = {"first"} if s == 0 and k > 1 else {"last"} if s == k - 1 and k > 1 else {"first", "last"} if k == 1 else {"middle"}
            g0 += k
        out = set()
        for g, _e in self.truncation_steps():
            out |= pos[g]
        return out


# ---- scripted cases ------------------------------------------------------------------------------------------
def _random_actions(seed, env, sub, steps):
    return np.random.default_rng([seed, env, sub]).integers(0, 2, steps).astype(np.int64)


def _forced_table(seed, n, episodes):
    """reset states inside +-0.05, as CartPole's own reset draws them: f64 [n][episodes][4]"""
    return np.random.default_rng([seed, 77]).uniform(-0.05, 0.05, (n, episodes, 4))


def _find_subseed(R, seed, base, i, start, forced_table, aseed):
    """the first sub-seed of env i's random action stream under which an episode ends on global step start - 1, so that the next one begins on `start`"""
    with _Mode(R):
        for sub in range(4000):
            acts = _random_actions(aseed, i, sub, start)
            s = R.reset_noise(seed, base + i, 0)
            k = 0
            for g in range(start):
                s, term = R.cartpole_step(s, int(acts[g]))
                if term:
                    if g == start - 1:
                        return sub
                    s = forced_table[i, k] if forced_table is not None else R.reset_noise(seed, base + i, k + 1)
                    k += 1
    raise AssertionError("no sub-seed ends an episode of env %d in front of step %d" % (i, start))


def scripted(R, n, steps, kinds, starts, forced, seed=5, base=300, aseed=11, switch_default=45):
    """kinds: i64 [n]; starts: {env: global step on which a kind-2 env's balanced episode must begin}"""
    kinds = np.asarray(kinds, np.int64)
    table = _forced_table(aseed, n, 2 + steps // 8) if forced else None
    switch = np.full(n, switch_default, np.int64)
    rand = np.zeros((steps, n), np.int64)
    for i in range(n):
        sub = 0
        if kinds[i] == K2 and i in starts:
            sub = _find_subseed(R, seed, base, i, starts[i], table, aseed)
            switch[i] = starts[i]
        if kinds[i] in (K2, K3):
            rand[:, i] = _random_actions(aseed, i, sub, steps)
    sim = Sim(R, n, seed, base, table)
    o = sim.reset()
    for g in range(steps):
        el = sim.elapsed[-1]
        ctrl = rule(o)
        a = ctrl.copy()
        a = np.where((kinds == K1A) & (el >= 490), 0, a)
        a = np.where((kinds == K1B) & (el >= 489), 1, a)
        a = np.where((kinds == K3) | ((kinds == K2) & (g < switch)), rand[g], a)
        o = sim.step(a)
    return sim.case(kinds=kinds, switch=switch, starts=dict(starts))


_FIVE = (K0, K1A, K1B, K2, K3)


def _spec(name):
    if name == "dqn37":     # 16-env workgroups with a ragged tail; positions 0, 15, 16 and 36 are long-episode envs (kinds 0, 0, 1a, 1a)
        return dict(n=37, steps=1100, kinds=[_FIVE[i % 5] for i in range(37)], starts={3: 51, 8: 99})
    if name == "ppo64":     # PPO's rollout launch: 16 workgroups of 4 envs — a multiple of 8, so the XCD-aware env-group map permutes — below MI_STATS_PART_MIN (32)
        return dict(n=64, steps=1100, kinds=[_FIVE[i % 5] for i in range(64)], starts={3: 51, 8: 99})
    if name == "n5":        # one env per workgroup: one of each long kind, the two kind-2 envs give the phases (their random stretch supplies the short episodes)
        return dict(n=5, steps=1100, kinds=[K0, K1A, K1B, K2, K2], starts={3: 51, 4: 99})
    if name == "n1030":     # the grid is capped at 1,024 workgroups: workgroups 0 - 5 walk envs (w, 1024 + w); those twelve are long-episode envs with different outcomes
        kinds = np.full(1030, K3, np.int64)
        kinds[:6] = [K0, K1A, K1B, K2, K2, K0]
        kinds[1024:] = [K1B, K2, K0, K1A, K2, K2]
        kinds[6:1024:97] = K0        # a few long ones among the single-env workgroups too
        return dict(n=1030, steps=520, kinds=kinds, starts={3: 12, 4: 13, 1025: 20, 1028: 19, 1029: 16})
    raise KeyError(name)


SHARED_1030 = tuple(range(6)) + tuple(range(1024, 1030))
NAMES = ("dqn37", "n5", "n1030", "ppo64")


@functools.lru_cache(maxsize=None)
def _get(name, forced):
    from oracle import cpu_ref
    return scripted(cpu_ref, forced=forced, **_spec(name))


def get(name, forced):
    """the cached case `name` in its keyed (forced = False) or forced-reset form"""
    return _get(name, bool(forced))


def replay(R, n, seed, base, actions, resets_at=()):
    """the oracle's run under a given action table (keyed resets); resets_at: global steps in front of which reset() is called again"""
    sim = Sim(R, n, seed, base)
    sim.reset()
    for g in range(len(actions)):
        if g in resets_at:
            sim.reset()
        sim.step(actions[g])
    return sim.case()


# ---- the limit rule restated, with the ways it can be wrong ---------------------------------------------------
def restate(R, case, envs, limit=LIMIT, terminated_is_done=False, zero_on_termination=True, carry_every=None, truncate=True):
    """TimeLimit + auto-reset around R.cartpole_step for the envs `envs` of `case` under its action table and its resets:
    -> (terminated u8 [steps][len(envs)], observations f32 [steps + 1][len(envs)][4], done bool [steps][len(envs)]).  The defaults are the true rule.
    carry_every = T: `elapsed` is zeroed in front of every T-th step (a rollout launch of T steps that does not carry it over from the launch before);
    truncate = False: `done := terminated`, a truncation neither flagged nor reset."""
    term_out = np.zeros((case.steps, len(envs)), np.uint8); obs_out = np.zeros((case.steps + 1, len(envs), 4), np.float32)
    done_out = np.zeros((case.steps, len(envs)), bool)
    table = case.forced_table
    with _Mode(R):
        for c, i in enumerate(envs):
            s = R.reset_noise(case.seed, case.base + i, 0)
            obs_out[0, c] = s
            elapsed, k = 0, 0
            for g in range(case.steps):
                if carry_every and g % carry_every == 0:
                    elapsed = 0
                s, term = R.cartpole_step(s, int(case.actions[g, i]))
                elapsed += 1
                trunc = truncate and (not term) and elapsed >= limit
                done = term or trunc
                term_out[g, c] = done if terminated_is_done else term
                done_out[g, c] = done
                if done:
                    s = table[i, k] if table is not None else R.reset_noise(case.seed, case.base + i, k + 1)
                    k += 1
                    if trunc or zero_on_termination:
                        elapsed = 0
                obs_out[g + 1, c] = s
    return term_out, obs_out, done_out


WRONG_RULES = {
    "terminated := done": dict(terminated_is_done=True),
    "limit 499": dict(limit=LIMIT - 1),
    "limit 501": dict(limit=LIMIT + 1),
    "elapsed not zeroed after a termination": dict(zero_on_termination=False),
}


# PPO's rollout launch (rollout_q4_kernel).  `terminated := done` is no wrong rule for it: PPO stores `done` (ppo.py:141).  `elapsed` lives in a register for a whole
# launch and crosses launches through the env handle: "T" stands for the launch length (ppo_wrong_rules)
PPO_WRONG_RULES = {
    "limit 499": dict(limit=LIMIT - 1),
    "limit 501": dict(limit=LIMIT + 1),
    "elapsed not zeroed after a termination": dict(zero_on_termination=False),
    "elapsed not carried across launches": dict(carry_every="T"),
    "done := terminated": dict(truncate=False),
}


def ppo_wrong_rules(T):
    """PPO_WRONG_RULES as restate() keywords for launches of T steps"""
    return {label: {k: (T if v == "T" else v) for k, v in kw.items()} for label, kw in PPO_WRONG_RULES.items()}


def ppo_launches(steps, T):
    """the launch lengths of PPO's view of a case: the floor(steps / T) whole rollouts; where those end in front of step 499, so that nothing can be truncated in them
    (1,030 envs x 520 steps at T = 300: ONE launch), one more launch takes the steps that are left"""
    out = [T] * (steps // T)
    if sum(out) < LIMIT and steps % T:
        out.append(steps % T)
    return out


# ---- controller networks: q_1 - q_0 = K (w . obs) ---------------------------------------------------------------
def controller_dqn(K):
    """QNetwork (4 -> 120 -> 84 -> 2): units 0 / 1 of layer 1 are relu(+-w . obs), carried through layer 2 to outputs 1 / 0 with weight K; everything else zero"""
    p = np.zeros(10934, np.float32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); W3 = p[10764:10932].reshape(2, 84)
    W1[0] = RULE_W; W1[1] = -RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    W3[1, 0] = K; W3[0, 1] = K
    return p


def controller_dueling(K):
    """DuelingQNetwork: the same two units into the advantage stream (q_1 - q_0 = a_1 - a_0); the value stream stays zero"""
    p = np.zeros(11019, np.float32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); Wa = p[10764 + 85:10764 + 85 + 168].reshape(2, 84)
    W1[0] = RULE_W; W1[1] = -RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    Wa[1, 0] = K; Wa[0, 1] = K
    return p


def controller_c51(K):
    """C51QNetwork (4 -> 120 -> 84 -> 2 x 101): the two units drive the logit of the top atom (z = +100) of actions 1 / 0; q_a grows with that logit"""
    p = np.zeros(27934, np.float32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); W3 = p[10764:27732].reshape(202, 84)
    W1[0] = RULE_W; W1[1] = -RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    W3[1 * 101 + 100, 0] = K; W3[0 * 101 + 100, 1] = K
    return p


def controller_iqn(K):
    """IQN: tau-embedding weights 0 and bias 1 (the quantiles do not depend on tau), the two units through the extractor and the head's first layer"""
    import _iqn_ref as Q
    p = np.zeros(Q.NPARAMS, np.float32)
    w = {k: p[Q.OFF[k]:Q.OFF[k] + int(np.prod(Q.SHAPES[k]))].reshape(Q.SHAPES[k]) for k in Q.ORDER}
    w["FW1"][0] = RULE_W; w["FW1"][1] = -RULE_W
    for name in ("FW2", "FW3", "QW1"):
        w[name][0, 0] = 1; w[name][1, 1] = 1
    w["CB"][:] = 1
    w["QW2"][1, 0] = K; w["QW2"][0, 1] = K
    return p


def mlp64(p, obs):
    """float64 forward of the 4 -> 120 -> 84 body on f32 inputs -> the features [rows][84]"""
    p = np.asarray(p, np.float32).astype(np.float64); X = np.asarray(obs, np.float32).astype(np.float64).reshape(-1, 4)
    h1 = np.maximum(X @ p[0:480].reshape(120, 4).T + p[480:600], 0)
    return np.maximum(h1 @ p[600:10680].reshape(84, 120).T + p[10680:10764], 0)


def q64(algo, p, obs):
    """float64 action values [rows][2] of a parameter vector of `algo` on f32 observations"""
    p = np.asarray(p, np.float32)
    if algo == "dqn":
        return mlp64(p, obs) @ p[10764:10932].astype(np.float64).reshape(2, 84).T + p[10932:10934].astype(np.float64)
    if algo == "dueling":
        f = mlp64(p, obs)
        v = f @ p[10764:10848].astype(np.float64).reshape(1, 84).T + np.float64(p[10848])
        a = f @ p[10849:11017].astype(np.float64).reshape(2, 84).T + p[11017:11019].astype(np.float64)
        return v + (a - a.mean(axis=1, keepdims=True))
    if algo == "c51":
        import _c51_ref as X
        return X.forward64(p, obs)[1]
    if algo == "iqn":
        import _iqn_ref as Q
        obs = np.asarray(obs, np.float32).reshape(-1, 4)
        return Q.forward(p, obs, np.full((len(obs), 32), 0.5, np.float32), np.float64)["q"]
    raise KeyError(algo)


def close_q(algo):
    """the distance below which the project leaves an action comparison out, per algorithm (tests/test_gpu_dqn.py, test_gpu_dueling.py: 1e-4; _c51_ref / _iqn_ref: CLOSE_Q)"""
    if algo in ("dqn", "dueling"):
        return 1e-4
    if algo == "c51":
        import _c51_ref as X
        return X.CLOSE_Q
    import _iqn_ref as Q
    return Q.CLOSE_Q


CONTROLLERS = {"dqn": controller_dqn, "dueling": controller_dueling, "c51": controller_c51, "iqn": controller_iqn}
CONTROLLER_K = 16.0   # |q_1 - q_0| = K |w . obs|: tests/test_timelimit_cases_cpu.py shows that under the rule fewer than 1 % of the decisions lie inside close_q


# ---- PPO: an ActorCritic (4 -> 64 -> 64 -> 2 | 4 -> 64 -> 64 -> 1, tanh) that follows the rule with a margin ---------------------------------------------------
PPO_NPARAMS, PPO_CRITIC = 9155, 4610      # include/mi_rl.h "Parameter layout": per net W1[unit][obs], b1, W2, b2, W3[out][unit], b3; the critic behind the actor
PPO_C, PPO_K = 50.0, 6.0


def _orthogonal(rng, rows, cols, gain):
    """torch.nn.init.orthogonal_'s construction (QR of a normal draw, signs of R's diagonal) from a numpy generator"""
    a = rng.normal(size=(max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    return (gain * (q if rows >= cols else q.T)).astype(np.float32)


def controller_ppo(c=PPO_C, K=PPO_K, critic_seed=17):
    """actor: unit 0 of layer 1 is tanh(c w . obs), carried through unit 0 of layer 2 (W2[0][0] = 1) to the logits -+K/2: l_1 - l_0 = K tanh(tanh(c w . obs)), every
    other actor weight zero.  It is a stochastic policy that takes the rule's action with probability >= 1 / (1 + exp(-K tanh(tanh(c |w . obs|)))) — about 10 % of
    the actions go against the rule without dropping the pole — and |log_prob| <= log(1 + exp(K tanh(tanh(inf)))) = 4.58.  The critic is a default-init draw
    (orthogonal, gains sqrt 2, sqrt 2, 1; zero biases: ppo.py:25-47) from a fixed seed, so that the values are no constants."""
    p = np.zeros(PPO_NPARAMS, np.float32)
    W1 = p[0:256].reshape(64, 4); W2 = p[320:4416].reshape(64, 64); W3 = p[4480:4608].reshape(2, 64)
    W1[0] = c * RULE_W
    W2[0, 0] = 1
    W3[1, 0] = K / 2; W3[0, 0] = -K / 2
    rng = np.random.default_rng(critic_seed)
    cr = p[PPO_CRITIC:]
    cr[0:256] = _orthogonal(rng, 64, 4, np.sqrt(2)).reshape(-1)
    cr[320:4416] = _orthogonal(rng, 64, 64, np.sqrt(2)).reshape(-1)
    cr[4480:4544] = _orthogonal(rng, 1, 64, 1.0).reshape(-1)
    return p


def ppo64(p, obs):
    """float64 forward of a flat ActorCritic vector on f32 observations -> (logits [rows][2], log-softmax [rows][2], values [rows])"""
    p = np.asarray(p, np.float32).astype(np.float64); X = np.asarray(obs, np.float32).astype(np.float64).reshape(-1, 4)

    def net(q, nout):
        h1 = np.tanh(X @ q[0:256].reshape(64, 4).T + q[256:320])
        h2 = np.tanh(h1 @ q[320:4416].reshape(64, 64).T + q[4416:4480])
        return h2 @ q[4480:4480 + 64 * nout].reshape(nout, 64).T + q[4480 + 64 * nout:4480 + 65 * nout]

    logits = net(p[:PPO_CRITIC], 2)
    m = logits.max(axis=1, keepdims=True)
    logp = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
    return logits, logp, net(p[PPO_CRITIC:], 1)[:, 0]


def ppo_noisy_params(seed=5):
    """default init plus noise, as tests/test_gpu_parity.py's test_rollout_production_rng_vs_oracle has it (a larger actor head: the log-probs are no constants);
    drawn with numpy, so that the CPU measurement and the GPU tests hold the same vector"""
    rng = np.random.default_rng([seed, 9155])
    p = np.zeros(PPO_NPARAMS, np.float32)
    for base, nout, gain in ((0, 2, 0.01), (PPO_CRITIC, 1, 1.0)):
        q = p[base:]
        q[0:256] = _orthogonal(rng, 64, 4, np.sqrt(2)).reshape(-1)
        q[320:4416] = _orthogonal(rng, 64, 64, np.sqrt(2)).reshape(-1)
        q[4480:4480 + 64 * nout] = _orthogonal(rng, nout, 64, gain).reshape(-1)
    idx = np.arange(PPO_NPARAMS)
    return (p + rng.normal(0, 0.3, PPO_NPARAMS) * (idx >= 4480) * (idx < PPO_CRITIC)).astype(np.float32)


# The oracle's f32 log-probs (R.actor -> R.categorical) and values (R.critic) against ppo64 on the observations each vector meets in the GPU tests (tests/test_timelimit_cases_cpu.py
# test_ppo_logprob_and_value_bounds_rest_on_the_oracle measures them again and holds them against these figures): the largest absolute distance over both parameter
# vectors.  The device bounds are max(3e-6, 8 x measured): 3e-6 is tests/test_gpu_parity.py's bound for values and log-probs at default-init scale, 8 the project's
# factor over a measured restatement distance.
MEASURED_PPO_LOGP = 1.2e-6     # measured 1.188e-06 (default init plus noise; the controller on its own run: 1.083e-06) -> device bound 9.6e-6
MEASURED_PPO_VALUE = 4.0e-7    # measured 3.906e-07 (default init plus noise; the controller's critic: 1.129e-07) -> device bound 3.2e-6


def ppo_bounds():
    return max(3e-6, 8 * MEASURED_PPO_LOGP), max(3e-6, 8 * MEASURED_PPO_VALUE)
