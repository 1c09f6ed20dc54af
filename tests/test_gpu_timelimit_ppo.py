"""The 500-step TimeLimit inside PPO's rollout launch — rollout_q4_kernel (mi_rollout.hip) through PPOEngine.rollout / rollout_gae and the C ABI — against the CPU oracle.

The kernel reads `elapsed` from the env handle, keeps it in a register for the T steps of a launch and stores it back, so a 500-step episode crosses several launches
(four at T = 128).  The tests drive it to the limit in every launch form: FORCED (teacher-forced actions, keyed or forced resets) and production (in-launch Philox
draws), EPLOG with atomics (`ppo_log`) and statistics kept per workgroup in the handle (`ppo_lazy`), the buffer-plus-reduce route, non-ringed (T <= 128) and ringed
(T = 300), the fused GAE tail; on grids of 2 workgroups (one of them three quarters shadow lanes), a ragged one, one whose env-group map permutes and 258 workgroups.

Exact (np.array_equal; the oracle runs its device-matched sin/cos): the four storage tensors the rule decides (Case.ppo_storage), the rows a launch never writes, the
carried observation, fp64 env state, `elapsed`, statistics and the episode log.  `values` and `log_probs` lie within T.ppo_bounds() of the oracle's rollout on the same
inputs (bounds measured on the oracle: tests/test_timelimit_cases_cpu.py); advantages / returns equal the oracle's GAE on the device's own inputs bit for bit.
tests/test_timelimit_cases_cpu.py shows on the CPU that a limit of 499 or 501, an `elapsed` that survives a termination or is lost between launches, or a truncation
neither flagged nor reset would change these expectations.

What each run compared goes to timelimit_gpu_compared.json in the tests' results directory."""
import functools

import numpy as np
import pytest

import _timelimit_cases as T
from test_gpu_timelimit import _check_call, _np, _record, _reset_case, _snapshot, _start

pytestmark = pytest.mark.gpu

MAX_EP = {"ppo_log": 8192, "ppo_lazy": 0}      # EPLOG = true with atomics | statistics per workgroup in the handle, summed by mi_env_episode_stats
KINDS = list(MAX_EP)
FORMS = pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
STORED = ("observations", "actions", "rewards", "dones")
ALL8 = ("observations", "values", "actions", "log_probs", "rewards", "dones", "advantages", "returns")
PATTERN = {"rewards": -3.25, "dones": -5.5, "actions": -1234567, "log_probs": -7.75}      # what the never-written rows hold from before the first launch


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


def _make(dev, kind, n, Tn, params, seed=5, base=300):
    import deep_rl_amd as D
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    agent = D.ActorCritic(env)
    agent.load_flat(np.zeros(T.PPO_NPARAMS, np.float32) if params is None else params)
    eng = D.PPOEngine(env, agent, D.ClipAdam(agent, lr=2.5e-4, eps=1e-5, max_grad_norm=0.5), num_steps=Tn, n_minibatch=1, max_episodes_logged=MAX_EP[kind])
    assert eng._lazy_stats == (kind == "ppo_lazy") and eng.max_ep == MAX_EP[kind]
    for f, v in PATTERN.items():
        getattr(eng, f)[Tn if f in ("actions", "log_probs") else 0] = v
    return eng


class _Upto:
    """the first G steps of a case, for Case.counts: what the whole launches of a run contain"""
    counts = T.Case.counts

    def __init__(self, case, G):
        self.n, self.trunc, self.terminated, self.fin_len = case.n, case.trunc[:G], case.terminated[:G], case.fin_len[:G]


def _check_storage(eng, case, g0, Tn, tag):
    want = case.ppo_storage(g0, Tn)
    got = {f: _np(getattr(eng, f)) for f in STORED + ("log_probs",)}
    for f in STORED:
        live = ~want["unwritten"][f]
        assert np.array_equal(got[f][live], want[f][live]), (tag, g0, f)
    for f, v in PATTERN.items():
        rows = got[f][want["unwritten"][f]]
        assert rows.shape == (1, case.n) and (rows == v).all(), (tag, g0, f, "a row the launch never writes was written")


def _check_gae(R, eng, tag):
    """advantages / returns against the oracle's GAE on the device's OWN rewards, dones and values: bit for bit"""
    st = R.Storage(eng.T, eng.N)
    for f in ("rewards", "dones", "values"):
        getattr(st, f)[...] = _np(getattr(eng, f))
    R.gae(st, eng.gamma, eng.gae_lambda)
    assert np.array_equal(_np(eng.advantages), st.advantages) and np.array_equal(_np(eng.returns), st.returns), (tag, "gae")
    return st


def _check_nets(eng, ref_values, ref_logp, tag):
    bl, bv = T.ppo_bounds()
    dv = float(np.abs(_np(eng.values) - ref_values).max()); dl = float(np.abs(_np(eng.log_probs)[:eng.T] - ref_logp).max())
    assert dv <= bv and dl <= bl, (tag, "values", dv, bv, "log_probs", dl, bl)
    return dl, dv


@functools.lru_cache(maxsize=None)
def _oracle_forced(name, forced, Tn):
    """values and log_probs[:T] of the oracle's rollout, launch after launch, under the case's actions and resets and the noisy default-init parameters: computed once,
    shared by the engine kinds, never written to"""
    from oracle import cpu_ref as R
    case = T.get(name, forced)
    params = T.ppo_noisy_params()
    out = []
    with T._Mode(R):
        env = R.VecCartPole(case.n, seed=case.seed, env_id_base=case.base)
        obs_cur = env.reset()
        g = 0
        for k in T.ppo_launches(case.steps, Tn):
            st = R.Storage(k, case.n)
            R.rollout(env, params, st, obs_cur, forced_actions=case.actions[g:g + k], forced_resets=None if case.forced_resets is None else case.forced_resets[g:g + k])
            assert np.array_equal(st.observations, case.obs[g:g + k + 1])
            v, lp = st.values.copy(), st.log_probs[:k].copy()
            v.setflags(write=False); lp.setflags(write=False)
            out.append((v, lp))
            g += k
    assert float(np.std(np.concatenate([lp.reshape(-1) for _v, lp in out]))) > 0.01      # (the log-probs are no constants)
    return tuple(out)


def _forced_inputs(case, g, k):
    import torch
    fr = None if case.forced_resets is None else torch.from_numpy(case.forced_resets[g:g + k])
    return torch.from_numpy(case.actions[g:g + k]), fr


def _run_forced(R, eng, case, name, Tn, tag, buffered=None):
    """teacher-forced: the case's actions (and reset states) through eng.rollout in whole launches of Tn steps; everything compared after every launch.
    buffered: a second engine driven through mi_ppo_rollout itself with a statistics buffer and max_ep = 0 (the buffer-plus-reduce route at >= 32 workgroups)"""
    import torch

    from deep_rl_amd import _native as N
    launches = T.ppo_launches(case.steps, Tn)
    assert launches == [Tn] * (case.steps // Tn)
    ref = _oracle_forced(name, case.forced, Tn)
    buf = torch.full((4,), 77, dtype=torch.int32, device=eng.device)
    g, worst = 0, (0.0, 0.0)
    for u, k in enumerate(launches):
        fa, fr = _forced_inputs(case, g, k)
        eng.rollout(forced_actions=fa, forced_resets=fr)
        _check_storage(eng, case, g, k, tag)
        _check_call(_snapshot(eng), case, g, k, tag)
        worst = tuple(max(a, b) for a, b in zip(worst, _check_nets(eng, ref[u][0], ref[u][1], tag)))
        eng.compute_gae()
        _check_gae(R, eng, tag)
        if buffered is not None:
            b = buffered
            fa, fr = fa.to(b.device), None if fr is None else fr.to(b.device)
            N.check(N.lib().mi_ppo_rollout(b.env.handle, N.ptr(b.agent.flat), b.T, N.ptr(b.observation), N.ptr(b.observations), N.ptr(b.values), N.ptr(b.actions),
                                           N.ptr(b.log_probs), N.ptr(b.rewards), N.ptr(b.dones), N.ptr(fa), None, N.ptr(fr), None, N.ptr(buf), 0,
                                           N.stream_ptr(b.device)), "mi_ppo_rollout")
            st, el = b.env.get_state()
            stats = buf.tolist()
            assert stats[3] == 0, stats
            _check_call(dict(observation=_np(b.observation).copy(), state=_np(st), elapsed=_np(el), stats=stats), case, g, k, tag + ("buffer",))
            for f in ALL8[:6]:
                assert np.array_equal(_np(getattr(b, f)), _np(getattr(eng, f))), (tag, g, f, "buffer route")
        g += k
    print(tag, "launches", len(launches), "largest log-prob / value distance from the oracle %.3e / %.3e" % worst, "bounds %.3e / %.3e" % T.ppo_bounds())
    return g


# ---- a. teacher-forced at the limit -------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn", [7, 50, 128, 300])
@FORMS
@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_rollouts_at_the_limit(dev, R, kind, forced, Tn):
    """the 5-env case: two workgroups, the second one env 4 (a long-episode env) plus three lanes that shadow it and must store nothing.  1,099 / 1,100 / 1,024 / 900
    steps in launches of 7 / 50 / 128 / 300 (the last one on the wrapped LDS ring)"""
    case = T.get("n5", forced)
    assert case.kinds[4] in T.LONG_KINDS
    eng = _make(dev, kind, case.n, Tn, T.ppo_noisy_params())
    _start(eng, case)
    G = _run_forced(R, eng, case, "n5", Tn, (kind, forced, Tn))
    k = _Upto(case, G).counts()
    assert k["truncations"] >= 2 and (Tn != 128 or k["envs_truncated_twice"] >= 1), k
    _record("ppo_a_teacher_forced_T%d" % Tn, kind, _Upto(case, G))


# ---- b. grid shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Tn", [("dqn37", 50), ("ppo64", 50), ("n1030", 7), ("n1030", 128)])
@FORMS
@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_rollouts_on_other_grids(dev, R, kind, forced, name, Tn):
    """37 envs: a ragged last workgroup.  64 envs: 16 workgroups, a multiple of 8, so the XCD-aware env-group map permutes.  1,030 envs: 258 workgroups, where the
    lazy kind keeps its statistics per workgroup at scale; beside the lazy engine a second one is driven through mi_ppo_rollout with a statistics buffer and
    max_ep = 0 (>= 32 workgroups: per workgroup, then summed into the buffer) and must report the same integers and store the same tensors"""
    case = T.get(name, forced)
    params = T.ppo_noisy_params()
    eng = _make(dev, kind, case.n, Tn, params)
    _start(eng, case)
    buffered = None
    if name == "n1030" and kind == "ppo_lazy":
        buffered = _make(dev, "ppo_lazy", case.n, Tn, params)
        _start(buffered, case)
    grid = (case.n + 3) // 4
    assert {"dqn37": case.n % 4 != 0, "ppo64": grid % 8 == 0 and grid < 32, "n1030": grid >= 32 and grid % 8 != 0}[name]
    G = _run_forced(R, eng, case, name, Tn, (kind, forced, name, Tn), buffered)
    envs = T.SHARED_1030 if name == "n1030" else None
    assert _Upto(case, G).counts(envs)["truncations"] >= 2
    _record("ppo_b_grid_%s_T%d" % (name, Tn), kind, _Upto(case, G), envs)


# ---- c. the production path runs into the limit -------------------------------------------------------------------
def _production_run(dev, R, kind, Tn, rollouts, fused=False):
    """FORCED = false under the controller network; -> (engine, per-rollout copies of everything, the oracle's case replayed from the device's own actions)"""
    n = 5
    eng = _make(dev, kind, n, Tn, T.controller_ppo(T.PPO_C, T.PPO_K))
    eng.reset()
    runs = []
    for _ in range(rollouts):
        (eng.rollout_gae if fused else eng.rollout)()
        runs.append(dict(snap=_snapshot(eng), **{f: _np(getattr(eng, f)).copy() for f in ALL8}))
    actions = np.concatenate([r["actions"][:Tn] for r in runs])
    assert set(np.unique(actions).tolist()) == {0, 1}
    return eng, runs, T.replay(R, n, 5, 300, actions)


@pytest.mark.parametrize("Tn,rollouts", [(128, 9), (300, 4)])
@pytest.mark.parametrize("kind", KINDS)
def test_production_rollouts_run_into_the_limit(dev, R, kind, Tn, rollouts):
    """the controller (l_1 - l_0 = 6 tanh(tanh(50 w . obs))) draws its own actions for 1,152 / 1,200 steps: T = 128 takes the uniforms the critic wave drew up front,
    T = 300 the in-loop Philox on the wrapped ring.  The device's actions are replayed on the oracle: storage, state, `elapsed`, statistics and log exact; every
    action is u >= p0 with the contract's uniform and the oracle's probability (steps with |u - p0| < 1e-5 left out, at most 1 %)"""
    params = T.controller_ppo(T.PPO_C, T.PPO_K)
    eng, runs, case = _production_run(dev, R, kind, Tn, rollouts)
    k = case.counts()
    assert k["truncations"] >= 2 and k["envs_truncated_twice"] >= 1, k
    uu = np.array([[R.action_uniform(5, 300 + e, g) for e in range(case.n)] for g in range(case.steps)], np.float32)
    left_out = 0
    with T._Mode(R):
        env = R.VecCartPole(case.n, seed=5, env_id_base=300)
        obs_cur = env.reset()
        st = R.Storage(Tn, case.n)
        for u, r in enumerate(runs):
            g = u * Tn
            tag = (kind, Tn, u)
            R.rollout(env, params, st, obs_cur, forced_actions=r["actions"][:Tn])
            want = case.ppo_storage(g, Tn)
            for f in STORED:
                live = ~want["unwritten"][f]
                assert np.array_equal(r[f][live], want[f][live]) and np.array_equal(getattr(st, f)[live], want[f][live]), (tag, f)
            for f, v in PATTERN.items():
                assert (r[f][want["unwritten"][f]] == v).all(), (tag, f)
            _check_call(r["snap"], case, g, Tn, tag)
            bl, bv = T.ppo_bounds()
            dv, dl = np.abs(r["values"] - st.values).max(), np.abs(r["log_probs"][:Tn] - st.log_probs[:Tn]).max()
            print(tag, "log-prob / value distance from the oracle %.3e / %.3e" % (dl, dv), "bounds %.3e / %.3e" % (bl, bv))
            assert dv <= bv and dl <= bl, (tag, dv, dl)
            _nl, p, _ent = R.categorical(R.actor(params, st.observations[:Tn].reshape(-1, 4)))
            p0 = p[:, 0].reshape(Tn, case.n)
            near = np.abs(uu[g:g + Tn] - p0) < 1e-5
            left_out += int(near.sum())
            assert np.array_equal(r["actions"][:Tn][~near], (uu[g:g + Tn] >= p0).astype(np.int64)[~near]), tag
    assert left_out <= 0.01 * case.steps * case.n, left_out
    against = float((case.actions != T.rule(case.obs[:-1].reshape(-1, 4)).reshape(case.actions.shape)).mean())
    assert 0.02 < against < 0.3, against      # a stochastic policy: the draws matter (about 10 % of the actions go against the rule)
    print(kind, Tn, "draws", case.steps * case.n, "left out", left_out, "against the rule %.3f" % against, k)
    _record("ppo_c_production_T%d" % Tn, kind, case)


# ---- d. fused GAE at a truncation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fused_gae_at_a_truncation(dev, R, kind):
    """rollout_gae() (the rollout workgroups scan their own envs from the LDS ring) against rollout() + compute_gae() on identical envs, 5 rollouts of 128 steps
    under the controller: all eight storage tensors bit-identical, the advantages the oracle's GAE on the device's inputs, and a truncated step does not bootstrap:
    its advantage is reward - value, the gamma * (1 - done) * (...) term being zero"""
    Tn, rollouts = 128, 5
    fused, fr, case = _production_run(dev, R, kind, Tn, rollouts, fused=True)
    plain = _make(dev, kind, 5, Tn, T.controller_ppo(T.PPO_C, T.PPO_K))
    plain.reset()
    checked = with_truncation = 0
    for u in range(rollouts):
        plain.rollout(); plain.compute_gae()
        for f in ALL8:
            assert np.array_equal(_np(getattr(plain, f)), fr[u][f]), (kind, u, f)
        _check_storage(plain, case, u * Tn, Tn, (kind, u))
        _check_call(fr[u]["snap"], case, u * Tn, Tn, (kind, u, "fused"))
        st = _check_gae(R, plain, (kind, u))
        assert np.array_equal(fr[u]["advantages"], st.advantages) and np.array_equal(fr[u]["returns"], st.returns)
        tr = case.trunc[u * Tn:(u + 1) * Tn]
        with_truncation += bool(tr.any())
        for t, e in zip(*np.nonzero(tr)):
            v, rew, adv = fr[u]["values"], fr[u]["rewards"], fr[u]["advantages"]
            assert fr[u]["dones"][t + 1, e] == 1.0 and v[t + 1, e] != 0.0      # (the reset observation has a value: bootstrapping from it would show)
            last = adv[t + 1, e] if t + 1 < Tn else np.float32(0)
            a = np.float32(0.99) * (np.float32(1.0) - fr[u]["dones"][t + 1, e])
            b = v[t + 1, e] + np.float32(0.95) * last
            want = np.float32(np.float32(rew[t + 1, e] + a * b) - v[t, e])      # the kernel's expression order; a = 0
            assert a == 0 and adv[t, e] == want == np.float32(np.float32(1.0) - v[t, e]), (kind, u, t, e, adv[t, e], want)
            assert fr[u]["returns"][t, e] == np.float32(adv[t, e] + v[t, e])
            checked += 1
    assert with_truncation >= 1 and checked >= 1, (with_truncation, checked)
    _record("ppo_d_fused_gae", kind, case)


# ---- e. checkpoint inside a long episode, reset() inside an episode ----------------------------------------------
def _rollouts(R, eng, case, g0, steps, tag):
    g = g0
    for _ in range(steps // eng.T):
        fa, fr = _forced_inputs(case, g, eng.T)
        eng.rollout(forced_actions=fa, forced_resets=fr)
        _check_storage(eng, case, g, eng.T, tag)
        _check_call(_snapshot(eng), case, g, eng.T, tag)
        g += eng.T
    return g


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_inside_a_long_episode(dev, R, kind, tmp_path):
    """saved at step 300 (six rollouts of 50), loaded into a fresh engine (zeroed parameters; its env first driven somewhere else: other state, `elapsed`, episode and
    step counters) and continued to step 650: storage, `elapsed`, log and statistics equal the uninterrupted run bit for bit, and the truncation comes at step 499"""
    import torch

    from deep_rl_amd import checkpoint
    Tn = 50
    case = T.get("n5", False)
    assert {T.K0, T.K1A, T.K1B} <= set(case.kinds.tolist()) and case.trunc[499].any() and not case.trunc[300:499].any()
    a = _make(dev, kind, case.n, Tn, np.random.default_rng(3).normal(0, 0.05, T.PPO_NPARAMS).astype(np.float32))
    _start(a, case)
    assert _rollouts(R, a, case, 0, 300, (kind, "before")) == 300
    path = checkpoint.save(str(tmp_path / kind), a)
    b = _make(dev, kind, case.n, Tn, None)
    b.reset()
    b.rollout(forced_actions=torch.zeros((Tn, case.n), dtype=torch.int64))
    assert not np.array_equal(_np(b.env.get_state()[1]), case.elapsed[300])
    checkpoint.load(path, b)
    assert np.array_equal(_np(b.agent.flat), _np(a.agent.flat)) and np.array_equal(_np(b.env.get_state()[1]), case.elapsed[300]) and (case.elapsed[300] > 0).any()
    for eng, tag in ((a, "uninterrupted"), (b, "resumed")):
        assert _rollouts(R, eng, case, 300, 200, (kind, tag)) == 500
        # the launch of steps 450 - 499 has just run: the truncation lies in its last row, `elapsed` starts again
        tr = case.trunc[499]
        assert (_np(eng.dones)[Tn][tr] == 1).all() and (_np(eng.env.get_state()[1])[tr] == 0).all() and (_np(eng.dones)[1:Tn][:, tr] == 0).all()
        assert _rollouts(R, eng, case, 500, 150, (kind, tag)) == 650
    for f in ALL8[:6] + ("observation",):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), f
    for x, y in zip(a.env.get_state(), b.env.get_state()):
        assert np.array_equal(_np(x), _np(y))
    _record("ppo_e_checkpoint", kind, _Upto(case, 650))


@pytest.mark.parametrize("kind", KINDS)
def test_reset_inside_an_episode_restarts_the_limit(dev, R, kind):
    """300 balanced steps, reset(), 500 more in rollouts of 50: no truncation at step 499, every env truncated at step 799, as the oracle's reset() has it"""
    Tn = 50
    case = _reset_case(R, 5)
    assert case.truncation_steps() == [(799, e) for e in range(case.n)] and (case.fin_len[799] == 500).all() and (case.elapsed[500] == 200).all()
    eng = _make(dev, kind, case.n, Tn, T.ppo_noisy_params())
    _start(eng, case)
    # the record holds the observation reset() left in front of step 300; the one the 300th step produced is checked here
    g = 0
    for _ in range(300 // Tn):
        eng.rollout(forced_actions=_forced_inputs(case, g, Tn)[0])
        g += Tn
    assert (_np(eng.env.get_state()[1]) == 300).all()
    assert np.array_equal(_np(eng.reset()), case.obs[300]) and (_np(eng.env.get_state()[1]) == 0).all()
    assert _rollouts(R, eng, case, 300, 200, (kind, "after reset")) == 500
    assert not _np(eng.dones)[1:].any() and (_np(eng.env.get_state()[1]) == 200).all()      # steps 450 - 499: nothing ends at 499
    assert _rollouts(R, eng, case, 500, 300, (kind, "after reset")) == 800
    assert (_np(eng.dones)[Tn] == 1).all() and (_np(eng.env.get_state()[1]) == 0).all()
    _record("ppo_e_reset", kind, _Upto(case, 800))
