"""Cases that drive the acting kernels of the two noisy libraries — nz_act_kernel (mi_noisy.hip) and rb_act_kernel (mi_rainbow.hip) — into CartPole's 500-step
TimeLimit, onto workgroups that walk two envs and through exploring steps beside the noise — TEST INFRASTRUCTURE (tests/test_noisy_acting_cases_cpu.py validates it,
tests/test_gpu_noisy_timelimit.py uses it).  CPU only: the oracle (oracle/cpu_ref.py) in its device-matched sin/cos mode through tests/_timelimit_cases.py, the
draw as tests/_noisy_ref.py and tests/_rainbow_ref.py restate it.

THE KEY.  A greedy step of env n (env id env_id_base + n) whose step counter is ctr evaluates the head of the sample (seed, env id, ctr, stream 13).  ctr is the
env's step_ctr: it counts every step, exploring and teacher-forced ones included, and is never zeroed; on an engine built fresh and reset once it is the global
step.  `keys(variant, ...)` gives the key of every (step, env) of a run; `variant` names a deliberately WRONG reading, used only to show that the cases tell it from
the right one (VARIANTS):
  workgroup_index_for_env_id   the sample of env n % 1,024 (the grid is capped at 1,024 workgroups: env 1,024 + w is the second env of workgroup w)
  env_index_without_base       the env's index where its id (env_id_base + index) belongs
  step_in_launch_for_ctr       the step inside the acting call
  elapsed_for_ctr              the TimeLimit's per-episode counter: the same number until the env's first episode ends
  greedy_count_for_ctr         the number of greedy steps the env has taken: the same number while nothing explores
  stream_14_for_13             the learning stream

FLOAT64 FORWARDS.  `q64(algo, params, obs, xi)` are the action values of the mean network (xi None) or of every row under ITS OWN sample (xi [rows][171] or
[rows][321], float32: the restatement's or the device's own factors), in float64 numpy: tests/_noisy_ref.forward / tests/_rainbow_ref.forward over many rows at once
(the CPU test holds the two against each other).  For the noisy dueling head the element noise is the float64 product of the factors, for Rainbow the float32
product, as those two modules have it.

CONTROLLERS.  controller_noisy(K) / controller_rainbow(K): hand-made networks whose MEAN decides as tests/_timelimit_cases.rule, with a sigma block behind them.
`live_params` is the jittered random network of the live-acting tests, `random_params` a random non-zero vector with non-zero sigmas for the teacher-forced runs
(a forced step that wrongly ran the network or the draw would otherwise cost nothing visible).

TRAJECTORIES.  `run(...)` predicts a live run on the CPU: the oracle's envs, every greedy action (q_1 > q_0) of q64 under the float32 restatement's sample for the
right key, every exploring action the keyed random action (tests/_c51_ref.explore_draws, stream 3; `explore_table` restates mi_u32_to_uniform against the table of
rg_eps_fill).  `expected(...)` evaluates a run's observations under the keys of a variant; `caught(...)` says in how many envs the FIRST decision a wrong reading
changes lies outside CLOSE_Q under both keys — up to there a kernel with that reading walks the same trajectory, so there the GPU comparison fails.
"""
import functools

import numpy as np

import _dqn_cases as D
import _noisy_ref as Z
import _rainbow_ref as RZ
import _timelimit_cases as T
from _c51_ref import explore_draws

f32 = np.float32
SEED, BASE, GRID = 5, 300, 1024
ALGOS = ("noisy", "rainbow")
REF = {"noisy": Z, "rainbow": RZ}
NPARAMS = {"noisy": Z.NP, "rainbow": RZ.NP}
NXI = {"noisy": Z.NXI, "rainbow": RZ.NXI}
SUPPORT = (0.0, 100.0)                      # the engines' default support
STREAM_ACT = 13
VARIANTS = ("workgroup_index_for_env_id", "env_index_without_base", "step_in_launch_for_ctr", "elapsed_for_ctr", "greedy_count_for_ctr", "stream_14_for_13")

CONTROLLER_K = T.CONTROLLER_K               # 16: |q_1 - q_0| = K |w . obs| under the mean network
# the sigma block of the controllers is default_sigma(SIGMA_SCALE): tests/test_noisy_acting_cases_cpu.py shows that under it every env of the live noisy run is
# truncated twice, that the noise flips hundreds of the 5,500 decisions against the mean network and that far fewer than 1 % of them lie inside CLOSE_Q
SIGMA_SCALE = 4.0
LIVE_N, LIVE_STEPS, LIVE_SCHEDULE = 5, 1100, "49+50"
# two envs per workgroup, live: 1,030 envs, two calls of 4 steps; the compared envs are the twelve that share a workgroup and every 8th of the others
SHARED_N, SHARED_CALLS = 1030, (4, 4)
SHARED_COMPARED = tuple(T.SHARED_1030) + tuple(i for i in range(SHARED_N) if i not in T.SHARED_1030)[::8]
# epsilon and learning_starts beside the noise: the start falls inside the second call of 7
EXPLORE_N, EXPLORE_STEPS, EXPLORE_CALL, EXPLORE_EPS, EXPLORE_STARTS = 5, 60, 7, 0.5, 13
# the parameter seeds of live_params for the two cases above: the first from 1 under which the conditions of the CPU test hold (shared_conditions / explore_conditions)
SHARED_PARAM_SEED = {"noisy": 1, "rainbow": 1}
EXPLORE_PARAM_SEED = {"noisy": 1, "rainbow": 1}


def close_q(algo, family="default"):
    return REF[algo].CLOSE_Q[family]


# ---- parameter vectors ---------------------------------------------------------------------------------------------------------------
def controller_noisy(K=CONTROLLER_K, sigma_scale=SIGMA_SCALE):
    """NoisyDuelingQNetwork (11,274 floats): tests/_timelimit_cases.controller_dueling(K) followed by the sigma block default_sigma(sigma_scale)"""
    return np.concatenate([T.controller_dueling(K), Z.default_sigma(sigma_scale)]).astype(f32)


def controller_rainbow(K=CONTROLLER_K, sigma_scale=SIGMA_SCALE):
    """RainbowQNetwork (36,774 floats): units 0 / 1 of layer 1 are relu(+-w . obs), carried through layer 2 into the advantage row of the top atom (z = v_max) of
    actions 1 / 0 with weight K; the value stream is zero; the sigma block is default_sigma(sigma_scale)"""
    p = np.zeros(RZ.NP, f32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); Wa = p[RZ.WA:RZ.BA].reshape(2 * RZ.NA, RZ.H2)
    W1[0] = T.RULE_W; W1[1] = -T.RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    Wa[1 * RZ.NA + RZ.NA - 1, 0] = K; Wa[0 * RZ.NA + RZ.NA - 1, 1] = K
    p[RZ.SIGMA:] = RZ.default_sigma(sigma_scale)
    return p


CONTROLLERS = {"noisy": controller_noisy, "rainbow": controller_rainbow}


def live_params(algo, seed):
    """the jittered random network of the live-acting tests (tests/test_gpu_noisy.py, tests/test_gpu_rainbow.py: _live_params)"""
    if algo == "noisy":
        rng = np.random.default_rng([seed, 2018, 13])
        return np.concatenate([D.init_params(rng)[1].astype(f32), Z.default_sigma(2.0) * rng.uniform(0.5, 1.5, Z.NHEAD).astype(f32)])
    rng = np.random.default_rng([seed, 2018, 22])
    return RZ.vector(D.init_params(rng)[1], rng, sigma_scale=2.0, jitter=True)


def random_params(algo, seed=3):
    """a random non-zero vector with non-zero sigmas"""
    rng = np.random.default_rng([seed, NPARAMS[algo]])
    p = rng.normal(0, 0.05, NPARAMS[algo]).astype(f32)
    sg = REF[algo].SIGMA
    p[sg:] = REF[algo].default_sigma() * rng.uniform(0.5, 1.5, NPARAMS[algo] - sg).astype(f32)
    assert p.all()
    return p


# ---- the draw over many keys ---------------------------------------------------------------------------------------------------------
def xi32(algo, a, b, stream=STREAM_ACT, seed=SEED):
    """the float32 restatement's factors of the samples (seed, a, b, stream); a and b broadcast -> (..., 171) or (..., 321)"""
    return REF[algo].xi(seed, a, b, stream)


def _rb_eps_rows(x):
    """_rainbow_ref.eps_of(*_rainbow_ref.factors(x)) for x [rows][321]: the element noise [rows][13,005], float32 products"""
    x = np.asarray(x, f32)
    fin = x[:, RZ._FI[:, None] + np.arange(RZ.H2)[None, :]]                        # [rows][153][84]
    fout = x[:, RZ._FO]                                                            # [rows][153]
    w = fout[:, :, None] * fin
    assert w.dtype == f32
    rows = len(x)
    return np.concatenate([w[:, :RZ.NA].reshape(rows, -1), fout[:, :RZ.NA], w[:, RZ.NA:].reshape(rows, -1), fout[:, RZ.NA:]], axis=1)


def _nz_eps_rows(x):
    """_noisy_ref.eps_of for x [rows][171] in float64: the element noise [rows][255], float64 products (as _noisy_ref.forward forms them)"""
    x = np.asarray(x, f32).astype(np.float64)
    w = Z._CI >= 0
    return np.where(w[None, :], x[:, Z._CO] * x[:, np.where(w, Z._CI, 0)], x[:, Z._CO])


# ---- float64 forwards ----------------------------------------------------------------------------------------------------------------
def _q64_noisy(p, obs, xi):
    p = np.asarray(p, f32)
    if xi is None:
        return T.q64("dueling", p[:Z.NP_MEAN], obs)
    f = T.mlp64(p, obs)
    p = p.astype(np.float64)
    head = p[None, Z.HEAD:Z.SIGMA] + p[None, Z.SIGMA:] * _nz_eps_rows(xi)       # [rows][255]: Wv, bv, Wa[2][84], ba[2]
    H = Z.H2
    v = (head[:, :H] * f).sum(1) + head[:, H]
    a = np.stack([(head[:, H + 1 + j * H:H + 1 + (j + 1) * H] * f).sum(1) + head[:, 2 * H + 1 + H + j] for j in range(2)], axis=1)
    return v[:, None] + (a - a.mean(axis=1, keepdims=True))


def _q64_rainbow(p, obs, xi, support=SUPPORT, chunk=256):
    p = np.asarray(p, f32)
    f = T.mlp64(p, obs)
    p = p.astype(np.float64)
    rows, NA, H = len(f), RZ.NA, RZ.H2
    lo, hi = np.float64(f32(support[0])), np.float64(f32(support[1]))
    z = lo + (hi - lo) / (NA - 1) * np.arange(NA)
    mu, sg = p[RZ.HEAD:RZ.SIGMA], p[RZ.SIGMA:]
    o_bv, o_wa, o_ba = RZ.BV - RZ.HEAD, RZ.WA - RZ.HEAD, RZ.BA - RZ.HEAD
    q = np.zeros((rows, 2))
    for r0 in range(0, rows, chunk):
        fr = f[r0:r0 + chunk]
        head = np.broadcast_to(mu, (len(fr), RZ.NHEAD)) if xi is None else mu[None, :] + sg[None, :] * _rb_eps_rows(xi[r0:r0 + chunk]).astype(np.float64)
        v = np.einsum("rjk,rk->rj", head[:, :o_bv].reshape(-1, NA, H), fr) + head[:, o_bv:o_wa]
        adv = (np.einsum("rjk,rk->rj", head[:, o_wa:o_ba].reshape(-1, 2 * NA, H), fr) + head[:, o_ba:]).reshape(-1, 2, NA)
        logit = v[:, None, :] + (adv - 0.5 * (adv[:, 0] + adv[:, 1])[:, None, :])
        e = np.exp(logit - logit.max(axis=-1, keepdims=True))
        q[r0:r0 + chunk] = ((e / e.sum(axis=-1, keepdims=True)) * z).sum(-1)
    return q


def q64(algo, params, obs, xi=None):
    """float64 action values [rows][2] on f32 observations: the mean network (xi None) or row r under the sample whose factors are xi[r]"""
    obs = np.asarray(obs, f32).reshape(-1, 4)
    if xi is not None:
        xi = np.asarray(xi, f32).reshape(-1, NXI[algo])
        assert len(xi) == len(obs)
    return _q64_noisy(params, obs, xi) if algo == "noisy" else _q64_rainbow(params, obs, xi)


# ---- exploring steps -----------------------------------------------------------------------------------------------------------------
def eps_table(steps, start_e, end_e, exploration_fraction=0.5, total_timesteps=100_000):
    """rg_eps_fill over global steps 0 ... steps - 1: max(slope * g + start_e, end_e), one product, one sum, one compare, in double"""
    slope = (np.float64(end_e) - np.float64(start_e)) / (np.float64(exploration_fraction) * np.float64(total_timesteps))
    return np.maximum(slope * np.arange(steps, dtype=np.float64) + np.float64(start_e), np.float64(end_e))


def explore_table(n, steps, start_e, end_e, learning_starts, base=BASE, seed=SEED):
    """-> (explores bool [steps][n], random_action i64 [steps][n]) of envs whose step counter is the global step: rg_act_loop's clause
    `global_step < learning_starts or (double) mi_u32_to_uniform(w0) < epsilon(global_step)`, the action w1 & 1"""
    g = np.arange(steps, dtype=np.uint64)
    u, ra = zip(*[explore_draws(seed, base + i, g) for i in range(n)])
    u, ra = np.stack(u, axis=1), np.stack(ra, axis=1)
    assert np.array_equal(u, u.astype(f32).astype(np.float64))      # mi_u32_to_uniform: (float)(w >> 8) * 2^-24 is exact in float32
    before = (np.arange(steps) < learning_starts)[:, None] if learning_starts > 0 else np.zeros((steps, 1), bool)
    return before | (u < eps_table(steps, start_e, end_e)[:, None]), ra


# ---- the keys ------------------------------------------------------------------------------------------------------------------------
def keys(variant, n, call_list, elapsed=None, explores=None, base=BASE):
    """-> (a u64 [steps][n], b u64 [steps][n], stream) of every (step, env) of a run in calls of call_list on an engine built fresh and reset once.  elapsed
    [steps][n]: the TimeLimit counter in front of each step; explores bool [steps][n] (None: every step is greedy)"""
    assert variant is None or variant in VARIANTS
    steps = int(sum(call_list))
    env = np.arange(n, dtype=np.uint64)
    a = np.broadcast_to(np.uint64(base) + env, (steps, n)).copy()
    b = np.broadcast_to(np.arange(steps, dtype=np.uint64)[:, None], (steps, n)).copy()
    stream = STREAM_ACT
    if variant == "workgroup_index_for_env_id":
        a[:] = np.uint64(base) + env % np.uint64(min(n, GRID))
    elif variant == "env_index_without_base":
        a[:] = env
    elif variant == "step_in_launch_for_ctr":
        b[:] = np.concatenate([np.arange(k) for k in call_list]).astype(np.uint64)[:, None]
    elif variant == "elapsed_for_ctr":
        b[:] = np.asarray(elapsed)[:steps].astype(np.uint64)
    elif variant == "greedy_count_for_ctr":
        greedy = np.ones((steps, n), bool) if explores is None else ~np.asarray(explores, bool)
        b[:] = (np.cumsum(greedy, axis=0) - greedy).astype(np.uint64)
    elif variant == "stream_14_for_13":
        stream = 14
    return a, b, stream


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
def run(algo, params, n, call_list, noisy=True, explore=None):
    """the live run on the CPU under the float32 restatement's samples for the right keys.  explore: None (epsilon 0, no learning_starts) or
    (start_e, end_e, learning_starts) -> dict(case, actions [steps][n], q [steps][n][2], xi [steps][n][NXI] or None, explores [steps][n], random [steps][n])"""
    from oracle import cpu_ref as R
    steps = int(sum(call_list))
    explores, ra = (np.zeros((steps, n), bool), np.zeros((steps, n), np.int64)) if explore is None else explore_table(n, steps, *explore)
    xi = None
    if noisy:
        a, b, stream = keys(None, n, call_list)
        xi = xi32(algo, a, b, stream)
    sim = T.Sim(R, n, SEED, BASE)
    o = sim.reset()
    qs = []
    for g in range(steps):
        q = q64(algo, params, o, None if xi is None else xi[g])
        qs.append(q)
        o = sim.step(np.where(explores[g], ra[g], (q[:, 1] > q[:, 0]).astype(np.int64)))
    case = sim.case()
    return dict(case=case, actions=case.actions, q=np.stack(qs), xi=xi, explores=explores, random=ra, call_list=list(call_list))


def expected(algo, params, r, variant):
    """the greedy actions a kernel with the reading `variant` of the key would take at the observations of the run r -> (actions [steps][n], |q_1 - q_0| [steps][n])"""
    case = r["case"]
    a, b, stream = keys(variant, case.n, r["call_list"], case.elapsed, r["explores"])
    q = q64(algo, params, case.obs[:-1], xi32(algo, a, b, stream)).reshape(case.steps, case.n, 2)
    return (q[..., 1] > q[..., 0]).astype(np.int64), np.abs(q[..., 1] - q[..., 0])


def caught(act, gap, act_wrong, gap_wrong, greedy, close, envs=None):
    """the envs in which the FIRST greedy decision that differs between the right and a wrong reading lies at least `close` outside a tie under both"""
    out = []
    for e in (range(act.shape[1]) if envs is None else envs):
        d = np.flatnonzero(greedy[:, e] & (act[:, e] != act_wrong[:, e]))
        if d.size and gap[d[0], e] >= close and gap_wrong[d[0], e] >= close:
            out.append(int(e))
    return out


def partner(n):
    """the other env of env n's workgroup in the 1,030-env case (n in SHARED_1030)"""
    return n + GRID if n < GRID else n - GRID


def gaps(q):
    q = np.asarray(q)
    return np.abs(q[..., 1] - q[..., 0])


@functools.lru_cache(maxsize=None)
def live_run(algo, noisy):
    """sections 3 / 4: the controller through 1,100 steps of 5 envs in calls of 49 + 50s"""
    return run(algo, CONTROLLERS[algo](), LIVE_N, T.calls(LIVE_SCHEDULE, LIVE_STEPS), noisy=noisy)


@functools.lru_cache(maxsize=None)
def shared_run(algo, param_seed=None):
    """section 5: 1,030 envs of a jittered random network, two calls of 4 steps"""
    seed = SHARED_PARAM_SEED[algo] if param_seed is None else param_seed
    return run(algo, live_params(algo, seed), SHARED_N, SHARED_CALLS)


@functools.lru_cache(maxsize=None)
def explore_run(algo, param_seed=None):
    """section 6: 5 envs, epsilon 0.5 throughout, learning_starts 13, 60 steps in calls of 7"""
    seed = EXPLORE_PARAM_SEED[algo] if param_seed is None else param_seed
    return run(algo, live_params(algo, seed), EXPLORE_N, T.calls("7", EXPLORE_STEPS), explore=(EXPLORE_EPS, EXPLORE_EPS, EXPLORE_STARTS))


def shared_conditions(algo, r, params):
    """what the 1,030-env case must hold -> dict: the excluded share of the compared decisions; the envs 1,024 + w in which the sample of env w (the first env of the
    same workgroup) would first have chosen another action, outside CLOSE_Q under both"""
    c = close_q(algo)
    sel = list(SHARED_COMPARED)
    gap = gaps(r["q"])
    aw, gw = expected(algo, params, r, "workgroup_index_for_env_id")
    greedy = ~r["explores"]
    return dict(excluded=float((gap[:, sel] < c).mean()), told_apart=caught(r["actions"], gap, aw, gw, greedy, c, envs=[i for i in T.SHARED_1030 if i >= GRID]))


def explore_conditions(algo, r, params):
    """what the epsilon case must hold -> dict"""
    c = close_q(algo)
    ex = r["explores"]
    gap = gaps(r["q"])
    ag, gg = expected(algo, params, r, "greedy_count_for_ctr")
    return dict(both_branches=bool((ex.any(0) & (~ex).any(0)).all()), greedy_after_exploring=bool((ex[:-1] & ~ex[1:]).any()),
                exploring_after_greedy=bool((~ex[:-1] & ex[1:]).any()), excluded=float((gap[~ex] < c).mean()),
                greedy_count_caught=caught(r["actions"], gap, ag, gg, ~ex, c))
