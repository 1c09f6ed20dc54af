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
NAMES = ("dqn37", "n5", "n1030")


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
def restate(R, case, envs, limit=LIMIT, terminated_is_done=False, zero_on_termination=True):
    """TimeLimit + auto-reset around R.cartpole_step for the envs `envs` of `case` under its action table and its resets:
    -> (terminated u8 [steps][len(envs)], observations f32 [steps + 1][len(envs)][4]).  The defaults are the true rule."""
    term_out = np.zeros((case.steps, len(envs)), np.uint8); obs_out = np.zeros((case.steps + 1, len(envs), 4), np.float32)
    table = case.forced_table
    with _Mode(R):
        for c, i in enumerate(envs):
            s = R.reset_noise(case.seed, case.base + i, 0)
            obs_out[0, c] = s
            elapsed, k = 0, 0
            for g in range(case.steps):
                s, term = R.cartpole_step(s, int(case.actions[g, i]))
                elapsed += 1
                trunc = (not term) and elapsed >= limit
                done = term or trunc
                term_out[g, c] = done if terminated_is_done else term
                if done:
                    s = table[i, k] if table is not None else R.reset_noise(case.seed, case.base + i, k + 1)
                    k += 1
                    if trunc or zero_on_termination:
                        elapsed = 0
                obs_out[g + 1, c] = s
    return term_out, obs_out


WRONG_RULES = {
    "terminated := done": dict(terminated_is_done=True),
    "limit 499": dict(limit=LIMIT - 1),
    "limit 501": dict(limit=LIMIT + 1),
    "elapsed not zeroed after a termination": dict(zero_on_termination=False),
}


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
