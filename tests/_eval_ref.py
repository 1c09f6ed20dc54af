"""Greedy evaluation episodes on the CPU oracle, and the networks the evaluation tests run — TEST INFRASTRUCTURE for libmirl_eval.so (include/mi_eval.h).

`run_episodes` steps single CartPole-v1 envs with the oracle's `reset_noise` / `cartpole_step` in its device-matched sin/cos mode ("fdlibm": bit for bit the
device's env) and takes the action values from the project's float64 restatements: `_timelimit_cases.q64` (dueling, C51), `_qrdqn_ref.forward64` (QR-DQN's
quantile mean) and `_rainbow_ref.forward` (the mean network).  The float64 argmax is the reference's greedy action; its gap |q_1 - q_0| says where a float32 device
may legitimately differ: only below the owning family's close-value distance (`CLOSE`).

Networks.  `controller(kind)` follows the balancing rule of `_timelimit_cases` with q_1 - q_0 growing with K (w . obs): the dueling and C51 controllers are that
module's, the QR and Rainbow ones are built the same way (two units carrying +-w . obs into the head).  `default_params(kind)` is the project's network class at
torch's default init under a fixed seed, built on the CPU.

The constants below are what tests/test_gpu_eval.py runs; tests/test_eval_ref_cpu.py shows on the reference alone that they meet the conditions those tests rest on.
"""
import functools
import types

import numpy as np

import _timelimit_cases as T

f32 = np.float32
LIMIT = T.LIMIT
KINDS = ("dueling", "qr", "c51", "rainbow")
KIND_ID = dict(dueling=1, qr=2, c51=3, rainbow=4)                         # MI_EV_DUELING .. MI_EV_RAINBOW; the plain QNetwork has no kind (include/mi_eval.h)
NREAD = dict(dueling=11019, qr=21644, c51=27934, rainbow=23769)   # the floats a kind reads
DEFAULT_SUPPORT = dict(c51=(-100.0, 100.0), rainbow=(0.0, 100.0))
ALT_SUPPORT = (0.0, 4.0)
# the seeds, the env ids and the episode counts the GPU tests use: chosen as the first from 1 upwards, none left out
SEED = 1
# torch.manual_seed of the default-init network, per kind: the first seed from 1 upwards under which every episode of SEED ends before SHORT steps and both actions
# occur (tests/test_eval_ref_cpu.py shows both, and that every smaller seed misses one of the two: a default-init CartPole policy often repeats one action)
NET_SEEDS = dict(dueling=7, qr=2, c51=4, rainbow=1)
SCRIPT_EPISODES = 12           # the env ids ENV_BASE .. ENV_BASE + 11 run every teacher-forced script: among them the pole falls on step 498, 499 and exactly on 500
ENV_BASE = 1 << 40
EPISODES = (1, 5, 37)
E_MAX = max(EPISODES)
MAX_EXCLUDED = 0.01            # the share of steps an action comparison may leave out (tests/test_timelimit_cases_cpu.py: CONTROLLER_K meets it)
SHORT = 200                    # every default-init episode ends before this many steps


def close(kind):
    """the owning family's close-value distance: below it the two action values are too close for an action comparison"""
    if kind == "dueling":
        return T.close_q("dueling")
    if kind == "c51":
        return T.close_q("c51")
    if kind == "qr":
        import _qrdqn_ref as Q
        return Q.CLOSE_Q
    import _rainbow_ref as B
    return B.CLOSE_Q["off"]   # the mean network: the family without noise


def atoms32(support, n):
    """z_j = v_min + dz * j in float32, dz = (v_max - v_min) / (n - 1): the header's expression"""
    lo, hi = f32(support[0]), f32(support[1])
    dz = f32(f32(hi - lo) / f32(n - 1))
    return (lo + (dz * np.arange(n, dtype=f32)).astype(f32)).astype(f32)


def q64(kind, params, obs, support=None):
    """float64 action values [rows][2] of the f32 parameters on f32 observations"""
    p = np.asarray(params, f32)
    obs = np.asarray(obs, f32).reshape(-1, 4)
    if kind == "dueling":
        return T.q64("dueling", p[:11019], obs)
    if kind == "qr":
        import _qrdqn_ref as Q
        return Q.forward64(p, obs)[1]
    if kind == "c51":
        if support is None or tuple(support) == DEFAULT_SUPPORT["c51"]:
            return T.q64("c51", p, obs)
        import _c51_ref as X
        return (X.forward64(p, obs)[0] * atoms32(support, 101).astype(np.float64)).sum(-1)
    import _rainbow_ref as B
    return B.forward(p, obs, tuple(support or DEFAULT_SUPPORT["rainbow"]))[1]


def run_episodes(R, params, kind, seed, envs, forced_actions=None, forced_starts=None, support=None):
    """the episodes of the env ids `envs`, stepped side by side -> a list of dicts: length, ret, truncated, actions i64 [length], obs f32 [length][4] (the
    observation each step's action was chosen at), gaps f64 [length] (|q_1 - q_0| in float64), greedy i64 [length] (the float64 argmax, ties to 0).
    forced_actions [len(envs)][500] / forced_starts f64 [len(envs)][4] as the device call takes them."""
    envs = [int(e) for e in envs]
    n = len(envs)
    with T._Mode(R):
        state = [np.asarray(forced_starts[i], np.float64).copy() if forced_starts is not None else R.reset_noise(seed, envs[i], 0) for i in range(n)]
        out = [dict(length=0, ret=f32(0), truncated=0, actions=[], obs=[], gaps=[], greedy=[]) for _ in range(n)]
        live = list(range(n))
        for t in range(LIMIT):
            x = np.stack([state[i] for i in live]).astype(f32)
            q = q64(kind, params, x, support)
            for r, i in enumerate(live):
                g = int(q[r, 1] > q[r, 0])
                a = g if forced_actions is None else int(forced_actions[i][t] != 0)
                o = out[i]
                o["obs"].append(x[r]); o["gaps"].append(abs(float(q[r, 1] - q[r, 0]))); o["greedy"].append(g); o["actions"].append(a)
                state[i], term = R.cartpole_step(state[i], a)
                o["length"] += 1; o["ret"] = f32(o["ret"] + f32(1))
                o["done"] = term or o["length"] >= LIMIT
                o["truncated"] = int(not term and o["length"] >= LIMIT)
            live = [i for i in live if not out[i]["done"]]
            if not live:
                break
    for o in out:
        o.pop("done")
        o["ret"] = float(o["ret"])
        o["actions"] = np.asarray(o["actions"], np.int64); o["greedy"] = np.asarray(o["greedy"], np.int64)
        o["obs"] = np.stack(o["obs"]).astype(f32); o["gaps"] = np.asarray(o["gaps"], np.float64)
    return out


def run_episode(R, params, kind, seed, env, forced_actions=None, forced_start=None, support=None):
    return run_episodes(R, params, kind, seed, [env], None if forced_actions is None else [forced_actions], None if forced_start is None else [forced_start], support)[0]


# ---- networks -----------------------------------------------------------------------------------------------------------------------------------------
def controller_qr(K):
    """QRQNetwork (4 -> 120 -> 84 -> 2 x 64): the two units into EVERY quantile of actions 1 / 0 with weight K, so that the quantile mean — the collapsed head, whose
    serial sum of 64 equal weights and 1 / 64 scale are exact — gives q_1 - q_0 = K (w . obs)"""
    p = np.zeros(21644, f32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); W3 = p[10764:21516].reshape(2, 64, 84)
    W1[0] = T.RULE_W; W1[1] = -T.RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    W3[1, :, 0] = K; W3[0, :, 1] = K
    return p


def controller_rainbow(K):
    """RainbowQNetwork (36,774 floats, the sigmas zero): the two units drive the ADVANTAGE logit of the top atom (z = v_max) of actions 1 / 0, as controller_c51
    drives C51's; the dueling rule halves and mirrors it (l[1][50] = -l[0][50] = K (w . obs) / 2) and q_a grows with that logit"""
    p = np.zeros(36774, f32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); Wa = p[15099:23667].reshape(2, 51, 84)
    W1[0] = T.RULE_W; W1[1] = -T.RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    Wa[1, 50, 0] = K; Wa[0, 50, 1] = K
    return p


CONTROLLERS = dict(dueling=T.controller_dueling, c51=T.controller_c51, qr=controller_qr, rainbow=controller_rainbow)


@functools.lru_cache(maxsize=None)
def controller(kind):
    p = CONTROLLERS[kind](T.CONTROLLER_K)
    p.setflags(write=False)
    return p


class _Spec:
    """what the network constructors read of an env"""
    observation_space = types.SimpleNamespace(shape=(4,))
    action_space = types.SimpleNamespace(n=2)
    device = "cpu"


def network_class(kind):
    """the project's class whose default init `default_params` draws.  DUELING: NoisyDuelingQNetwork, whose first 11,019 floats are a dueling network's (its means)
    — DuelingQNetwork itself packs its plain image on the device when it is built, so it has no CPU construction"""
    import deep_rl_amd as D
    return dict(dueling=D.NoisyDuelingQNetwork, qr=D.QRQNetwork, c51=D.C51QNetwork, rainbow=D.RainbowQNetwork)[kind]


@functools.lru_cache(maxsize=None)
def default_params(kind, seed=None):
    """the flat float32 vector of network_class(kind) at torch's default init under torch.manual_seed(seed or NET_SEEDS[kind]), built on the CPU (11,274 floats for "dueling" and 36,774
    for "rainbow": the kind reads the means in front)"""
    import torch

    gen = torch.random.get_rng_state()
    try:
        torch.manual_seed(NET_SEEDS[kind] if seed is None else seed)
        net = network_class(kind)(_Spec(), device="cpu")
        p = net.flat.detach().numpy().astype(f32).copy()
    finally:
        torch.random.set_rng_state(gen)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference_run(net, kind, n=E_MAX):
    """the unforced float64 episodes of SEED on the env ids ENV_BASE .. ENV_BASE + n - 1: net "controller" or "default"; computed once per process and shared"""
    from oracle import cpu_ref as R
    p = controller(kind) if net == "controller" else default_params(kind)
    return run_episodes(R, p, kind, SEED, [ENV_BASE + e for e in range(n)])


# ---- teacher-forced scripts (tests/_timelimit_cases.py's kinds, one episode each) --------------------------------------------------------------------------
SCRIPTS = (("rule", T.K0), ("rule_then_0_from_490", T.K1A), ("rule_then_1_from_489", T.K1B), ("random", T.K3))


def script(R, name, seed, env):
    """-> (actions u8 [500], dict of the oracle's length / ret / truncated) of one scripted episode from its keyed start; bytes behind the end are 0"""
    kind = dict(SCRIPTS)[name]
    rand = T._random_actions(11, env & 0xFFFF, 0, LIMIT)
    acts = np.zeros(LIMIT, np.uint8)
    with T._Mode(R):
        s = R.reset_noise(seed, env, 0)
        for t in range(LIMIT):
            a = int(T.rule(s.astype(f32)))
            if kind == T.K1A and t >= 490:
                a = 0
            if kind == T.K1B and t >= 489:
                a = 1
            if kind == T.K3:
                a = int(rand[t])
            acts[t] = a
            s, term = R.cartpole_step(s, a)
            if term or t + 1 >= LIMIT:
                return acts, dict(length=t + 1, ret=float(t + 1), truncated=int(not term))
    raise AssertionError("unreachable")


@functools.lru_cache(maxsize=None)
def scripts(name):
    """the script `name` on the env ids ENV_BASE .. ENV_BASE + SCRIPT_EPISODES - 1 -> (actions u8 [12][500], the oracle's results)"""
    from oracle import cpu_ref as R
    rows = [script(R, name, SEED, ENV_BASE + e) for e in range(SCRIPT_EPISODES)]
    return np.stack([r[0] for r in rows]), [r[1] for r in rows]


def reachable_box(rng, n):
    """n observations drawn over the env's reachable box: |x| <= 2.4, |theta| <= 0.21 and velocities of the size an episode shows (|x_dot| <= 3, |theta_dot| <= 3.5)"""
    hi = np.array([2.4, 3.0, 0.21, 3.5])
    return rng.uniform(-hi, hi, (n, 4)).astype(f32)
