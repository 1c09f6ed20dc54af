"""The acting kernels of the two noisy libraries — nz_act_kernel (mi_noisy.hip, through NoisyDQNEngine) and rb_act_kernel (mi_rainbow.hip, through RainbowEngine) —
at CartPole's 500-step TimeLimit, teacher-forced (FORCED = true, with and without NOISY), on workgroups that walk two envs, over 1,100 live steps under the mean
network and under the noise, and with exploring steps beside the noise.  The cases come from tests/_timelimit_cases.py and tests/_noisy_acting_cases.py (validated on
the CPU by tests/test_timelimit_cases_cpu.py and tests/test_noisy_acting_cases_cpu.py), the helpers from tests/test_gpu_timelimit.py as
tests/test_gpu_ddqn_timelimit.py uses them.

Ring, carried observation, fp64 env state, `elapsed`, per-call statistics and the episode log are compared exactly (np.array_equal) against the oracle in its
device-matched sin/cos mode.  A live action is compared with (q_1 > q_0) of the float64 forward of the stored observation — under the DEVICE'S OWN sample for
(env_id_base + n, step counter, 13) from mi_nz_noise / mi_rb_noise where the noise acts — wherever |q_1 - q_0| is at least CLOSE_Q of tests/_noisy_ref.py /
tests/_rainbow_ref.py; the decisions left out are counted and capped at 1 %.  The step counter of the key is the env's step_ctr, which counts every step and is never
zeroed: every engine here is built fresh and reset once, so it is the global step.

What each test compared goes to noisy_acting_gpu_compared.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest

import _noisy_acting_cases as A
import _timelimit_cases as T
from test_gpu_timelimit import _check_call, _check_ring, _checkpoint_inside_a_long_episode, _np, _reset_case, _reset_inside_an_episode, _run_forced, _snapshot, _start

pytestmark = pytest.mark.gpu
f32 = np.float32


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


def _cases_module(algo):
    if algo == "noisy":
        import test_gpu_noisy_cases as M
    else:
        import test_gpu_rainbow_cases as M
    return M


def _make(dev, algo, n, slots, params=None, **kw):
    """the engine as test_gpu_noisy_cases.make_engine / test_gpu_rainbow_cases.make_engine build it, seed 5, env_id_base 300.  params: the flat vector of both
    networks (default: a random non-zero vector with non-zero sigmas — a teacher-forced step that wrongly ran the network or the draw would show)"""
    import deep_rl_amd as D
    p = A.random_params(algo) if params is None else np.asarray(params, f32)
    assert p.size == A.NPARAMS[algo]
    kw.setdefault("prioritized", False)
    kw.setdefault("max_episodes_logged", 8192)
    eng = _cases_module(algo).make_engine(dev, n, slots, params=p, target=p, seed=A.SEED, base=A.BASE, **kw)
    assert type(eng) is {"noisy": D.NoisyDQNEngine, "rainbow": D.RainbowEngine}[algo] and np.array_equal(_np(eng.q.flat), p)
    return eng


def _device_xi(dev, algo, a, b, stream=A.STREAM_ACT):
    """the factors [rows][171] / [rows][321] of the samples (5, a[r], b[r], stream) as the device forms them"""
    M = _cases_module(algo)
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    out = np.stack([M.device_sample(dev, A.SEED, int(x), int(y), stream)[0] for x, y in zip(a, b)])
    if algo == "rainbow":       # the element noise the forward forms from these factors is the device's own element noise
        assert np.array_equal(A._rb_eps_rows(out[:1])[0].view(np.uint32), M.device_eps(dev, A.SEED, int(a[0]), int(b[0]), stream).view(np.uint32))
    assert np.isfinite(out).all()
    return out


_COMPARED = {}
_SUMS = ("runs", "truncations", "envs_truncated_twice", "decisions_checked", "decisions_excluded", "noise_chosen", "told_apart")


def _record(test, algo, case, envs=None, checked=0, excluded=0, noise_chosen=0, told_apart=0, smallest_gap=None):
    """noise_chosen: decisions the mean network would have taken otherwise; told_apart: second envs of a workgroup the first env's sample would have steered otherwise"""
    import _c51_ref as X
    k = case.counts(envs)
    rec = _COMPARED.setdefault(test, {}).setdefault(algo, dict({f: 0 for f in _SUMS}, smallest_gap=None))
    for f, v in (("runs", 1), ("truncations", k["truncations"]), ("envs_truncated_twice", k["envs_truncated_twice"]), ("decisions_checked", checked),
                 ("decisions_excluded", excluded), ("noise_chosen", noise_chosen), ("told_apart", told_apart)):
        rec[f] += int(v)
    if smallest_gap is not None:
        rec["smallest_gap"] = float(smallest_gap) if rec["smallest_gap"] is None else min(rec["smallest_gap"], float(smallest_gap))
    path = os.path.join(X.results_dir(), "noisy_acting_gpu_compared.json")
    try:
        with open(path) as f:
            old = json.load(f)
    except (OSError, ValueError):
        old = {}
    for t, by_algo in _COMPARED.items():
        old.setdefault(t, {}).update(by_algo)
    with open(path, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
    print("compared", test, algo, json.dumps(rec))


def _truncated_steps_hold_the_reset_observation(eng, case):
    """on a ring that holds the whole run: the stored flag is `terminated`, not `done` — the two differ exactly on the truncated steps, behind which lies the RESET
    observation"""
    differ = _np(eng.terminated)[1:] != case.done.astype(np.uint8)
    assert np.array_equal(differ, case.trunc) and differ.sum() == case.counts()["truncations"] >= 2
    trunc_step, trunc_env = np.nonzero(case.trunc)
    assert not _np(eng.terminated)[1:][trunc_step, trunc_env].any()
    assert np.array_equal(_np(eng.observations)[1:][trunc_step, trunc_env], case.obs[1:][trunc_step, trunc_env])


def _decisions(dev, algo, params, obs, actions, a, b, tag):
    """stored actions against the float64 forward under the device's sample of each row's key -> (q [rows][2], far bool [rows]); at most 1 % inside CLOSE_Q"""
    xi = _device_xi(dev, algo, a, b)
    q = A.q64(algo, params, obs, xi)
    far = A.gaps(q) >= A.close_q(algo)
    assert (~far).mean() <= 0.01, (tag, int((~far).sum()), far.size)
    want = (q[:, 1] > q[:, 0]).astype(np.int64)
    bad = np.flatnonzero(far & (np.asarray(actions).reshape(-1) != want))
    assert bad.size == 0, (tag, "rows", bad[:8].tolist(), "of", far.size, "q", q[bad[:4]].tolist())
    return q, far, xi


# ---- 1. teacher-forced acting at the limit ------------------------------------------------------------------------------------------
_FORCED_RUNS = [(True, forced, schedule) for forced in (False, True) for schedule in T.SCHEDULES] + [(False, False, "49+50"), (False, True, "7")]


@pytest.mark.parametrize("noisy,forced,schedule", _FORCED_RUNS, ids=["%s-%s-%s" % ("noisy" if z else "mean", "forced" if f else "keyed", s) for z, f, s in _FORCED_RUNS])
@pytest.mark.parametrize("algo", A.ALGOS)
def test_teacher_forced_acting_at_the_limit(dev, algo, noisy, forced, schedule):
    """FORCED = true with NOISY on (every form and schedule) and off (one schedule per form): 1,100 steps of the scripted 5-env case, once on a ring that holds the whole
    run, compared at the end, once on 16 slots, compared after every call"""
    case = T.get("n5", forced)
    call_list = T.calls(schedule, case.steps)
    for slots, every in ((case.steps + 1, False), (16, True)):
        eng = _make(dev, algo, case.n, slots, noisy=noisy)
        assert eng.noisy == noisy
        _start(eng, case)
        _run_forced(eng, case, call_list, slots, every, (algo, noisy, forced, schedule, slots))
        if slots > case.steps:
            _truncated_steps_hold_the_reset_observation(eng, case)
        _record("1_teacher_forced" + ("" if noisy else "_mean"), algo, case)


@pytest.mark.parametrize("algo", A.ALGOS)
def test_teacher_forced_acting_marks_the_priorities(dev, algo):
    """the 5-env case through a prioritized engine on 64 slots in calls of 7: the ring exact after every call; the rows that hold a transition — every row this call
    wrote among them — hold max_priority, the write head holds 0 (the invariant of tests/test_gpu_pdd.py, as mi_per_mark_sums leaves them)"""
    import torch
    case = T.get("n5", False)
    S = 64
    eng = _make(dev, algo, case.n, S, prioritized=True)
    assert eng.prioritized and eng.noisy
    _start(eng, case)
    g = 0
    for k in T.calls("7", case.steps):
        eng.act(k, forced_actions=torch.from_numpy(case.actions[g:g + k]))
        _check_call(_snapshot(eng), case, g, k, (algo, "prioritized"))
        g += k
        _check_ring(eng, case, g, S, (algo, "prioritized"))
        prio = _np(eng.priorities)
        written = [s % S for s in range(max(0, g - (S - 1)), g)]
        assert set((g - 1 - s) % S for s in range(k)) <= set(written)
        assert (prio[written] == f32(1e-2)).all() and (prio[g % S] == 0).all(), (g, "priorities after act")
    assert eng.global_step == g == case.steps and float(eng.max_priority.item()) == float(f32(1e-2))
    _record("1_teacher_forced_prioritized", algo, case)


# ---- 2. two envs per workgroup, teacher-forced --------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
@pytest.mark.parametrize("algo", A.ALGOS)
def test_two_envs_per_workgroup_at_the_limit(dev, algo, forced, schedule):
    """1,030 envs on a grid capped at 1,024 workgroups: workgroups 0 - 5 walk two long-episode envs each; all 1,030 envs and the statistics summed over them"""
    case = T.get("n1030", forced)
    assert case.n > A.GRID and all(case.kinds[i] in T.LONG_KINDS for i in T.SHARED_1030)
    slots, every = (16, True) if schedule == "7" else (case.steps + 1, False)
    eng = _make(dev, algo, case.n, slots)
    _start(eng, case)
    _run_forced(eng, case, T.calls(schedule, case.steps), slots, every, (algo, forced, schedule, slots))
    _record("2_two_envs_per_workgroup", algo, case, T.SHARED_1030)


# ---- 3. / 4. the controller runs into the limit, under the mean network and under the noise ------------------------------------------------
def _live(dev, R, algo, params, n, call_list, slots, **kw):
    """a live run of a fresh engine -> (engine, the oracle's replay of the device's own actions), everything but the actions compared exactly"""
    steps = int(sum(call_list))
    eng = _make(dev, algo, n, slots, params=params, **kw)
    eng.reset()
    snaps = []
    for k in call_list:
        eng.act(k)
        snaps.append(_snapshot(eng))
    assert eng.global_step == steps <= slots
    actions = _np(eng.actions)[:steps]
    assert set(np.unique(actions).tolist()) == {0, 1}
    case = T.replay(R, n, A.SEED, A.BASE, actions)
    g = 0
    for k, snap in zip(call_list, snaps):
        _check_call(snap, case, g, k, algo)
        g += k
    _check_ring(eng, case, steps, slots, algo)
    return eng, case


@pytest.mark.parametrize("algo", A.ALGOS)
def test_mean_network_controller_runs_into_the_limit(dev, R, algo):
    """FORCED = false, NOISY = false: the hand-made controller acts for 1,100 steps of 5 envs.  Ring, flags, `elapsed`, statistics and log exact on the replay of the
    device's own actions; every action (q_1 > q_0) of the float64 mean forward wherever the gap is at least CLOSE_Q["off"]; an env truncated twice"""
    params = A.CONTROLLERS[algo]()
    eng, case = _live(dev, R, algo, params, A.LIVE_N, T.calls(A.LIVE_SCHEDULE, A.LIVE_STEPS), A.LIVE_STEPS + 1, noisy=False, learning_starts=0)
    assert not eng.noisy and eng.start_e == eng.end_e == 0.0
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    q = A.q64(algo, params, case.obs[:-1])
    far = A.gaps(q) >= A.close_q(algo, "off")
    assert (~far).mean() <= 0.01, int((~far).sum())
    assert np.array_equal(case.actions.reshape(-1)[far], (q[:, 1] > q[:, 0]).astype(np.int64)[far])
    _record("3_mean_network_live", algo, case, checked=far.sum(), excluded=(~far).sum(), smallest_gap=A.gaps(q).min())


@pytest.mark.parametrize("algo", A.ALGOS)
def test_noisy_controller_runs_into_the_limit(dev, R, algo):
    """FORCED = false, NOISY = true: every one of the 5 x 1,100 decisions is (q_1 > q_0) of the float64 forward of the stored observation under the device's own sample
    for (300 + n, g, 13), g the global step, unless |q_1 - q_0| < CLOSE_Q (at most 1 %); the replay gives ring, `elapsed`, statistics and log exactly; an env is
    truncated twice; the noise, not the mean network, chose some of the actions"""
    params = A.CONTROLLERS[algo]()
    call_list = T.calls(A.LIVE_SCHEDULE, A.LIVE_STEPS)
    eng, case = _live(dev, R, algo, params, A.LIVE_N, call_list, A.LIVE_STEPS + 1, learning_starts=0)
    assert eng.noisy and eng.start_e == eng.end_e == 0.0
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    a, b, stream = A.keys(None, case.n, call_list)
    assert stream == 13
    obs = case.obs[:-1].reshape(-1, 4)
    q, far, _ = _decisions(dev, algo, params, obs, case.actions, a, b, algo)
    qm = A.q64(algo, params, obs)
    chosen = far & (A.gaps(qm) >= A.close_q(algo)) & ((qm[:, 1] > qm[:, 0]).astype(np.int64) != case.actions.reshape(-1))
    assert chosen.sum() >= 1
    assert far.size == 5500
    _record("4_noisy_live", algo, case, checked=far.sum(), excluded=(~far).sum(), noise_chosen=chosen.sum(), smallest_gap=A.gaps(q).min())


# ---- 5. noise keys when a workgroup walks two envs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", A.ALGOS)
def test_noise_keys_when_a_workgroup_walks_two_envs(dev, R, algo):
    """1,030 envs of a jittered random network, epsilon 0, two calls of 4 steps: the head copy (nz_policy's `cur`, rb_policy's sm.xi) carries from a workgroup's first
    env to its second and from launch to launch.  The twelve envs that share a workgroup and every 8th of the others take the float64 argmax under the device sample
    for (300 + n, g, 13) at every step; all 1,030 rings are the oracle's replay; envs w and 1,024 + w drew different samples, and for at least one env 1,024 + w the
    sample of env w would have chosen otherwise"""
    params = A.live_params(algo, A.SHARED_PARAM_SEED[algo])
    calls = list(A.SHARED_CALLS)
    steps = sum(calls)
    eng, case = _live(dev, R, algo, params, A.SHARED_N, calls, 16, learning_starts=0)
    assert eng.noisy and case.n == 1030
    sel = np.array(A.SHARED_COMPARED)
    a, b, _ = A.keys(None, case.n, calls)
    obs, act = case.obs[:steps][:, sel], case.actions[:, sel]
    q, far, xi = _decisions(dev, algo, params, obs.reshape(-1, 4), act, a[:, sel], b[:, sel], algo)
    xi = xi.reshape(steps, len(sel), -1)
    col = {int(n): c for c, n in enumerate(sel)}
    for w in range(6):
        assert not np.array_equal(xi[:, col[w]], xi[:, col[A.GRID + w]])
    # the second env of each shared workgroup under the FIRST one's sample (the device's own, drawn above)
    second = [n for n in T.SHARED_1030 if n >= A.GRID]
    cs, cp = [col[n] for n in second], [col[A.partner(n)] for n in second]
    qw = A.q64(algo, params, obs[:, cs].reshape(-1, 4), xi[:, cp].reshape(-1, xi.shape[-1])).reshape(steps, len(second), 2)
    gap = A.gaps(q).reshape(steps, len(sel))[:, cs]
    told = A.caught(act[:, cs], gap, (qw[..., 1] > qw[..., 0]).astype(np.int64), A.gaps(qw), np.ones((steps, len(second)), bool), A.close_q(algo))
    assert len(told) >= 1
    _record("5_two_envs_per_workgroup_live", algo, case, list(sel), checked=far.sum(), excluded=(~far).sum(), told_apart=len(told), smallest_gap=A.gaps(q).min())


# ---- 6. epsilon and learning_starts beside the noise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", A.ALGOS)
def test_epsilon_and_learning_starts_beside_the_noise(dev, R, algo):
    """start_e = end_e = 0.5 and learning_starts = 13 with noisy = True, 60 steps in calls of 7: a step with g < 13 or u < 0.5 stores the keyed random action exactly;
    every other step the float64 argmax under the sample of (env id, step counter) — the counter of ALL steps, not of the greedy ones"""
    params = A.live_params(algo, A.EXPLORE_PARAM_SEED[algo])
    call_list = T.calls("7", A.EXPLORE_STEPS)
    eng, case = _live(dev, R, algo, params, A.EXPLORE_N, call_list, A.EXPLORE_STEPS + 1, learning_starts=A.EXPLORE_STARTS, start_e=A.EXPLORE_EPS, end_e=A.EXPLORE_EPS)
    assert eng.noisy and eng.learning_starts == 13 and eng.start_e == eng.end_e == 0.5
    ex, ra = A.explore_table(case.n, case.steps, A.EXPLORE_EPS, A.EXPLORE_EPS, A.EXPLORE_STARTS)
    assert ex[:A.EXPLORE_STARTS].all() and (ex.any(0) & (~ex).any(0)).all()                       # both branches in every env
    assert (ex[:-1] & ~ex[1:]).any() and (~ex[:-1] & ex[1:]).any()                                # a greedy step directly behind an exploring one, and the reverse
    assert np.array_equal(case.actions[ex], ra[ex])
    a, b, _ = A.keys(None, case.n, call_list)
    greedy = ~ex
    q, far, _ = _decisions(dev, algo, params, case.obs[:-1][greedy], case.actions[greedy], a[greedy], b[greedy], algo)
    _record("6_epsilon_beside_the_noise", algo, case, checked=far.sum() + ex.sum(), excluded=(~far).sum(), smallest_gap=A.gaps(q).min())


# ---- 7. checkpoint and reset inside a long episode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", A.ALGOS)
def test_checkpoint_inside_a_long_episode(dev, algo, tmp_path):
    """saved at global step 300 of the 5-env case, loaded into a fresh engine whose env was driven somewhere else, continued to step 620 (the body of
    tests/test_gpu_timelimit.py's test)"""
    assert A.NPARAMS[algo] == {"noisy": 11274, "rainbow": 36774}[algo]
    _checkpoint_inside_a_long_episode(lambda n, slots, params=None: _make(dev, algo, n, slots, params=params), T.get("n5", False), A.NPARAMS[algo],
                                      str(tmp_path / algo), algo)


@pytest.mark.parametrize("algo", A.ALGOS)
def test_reset_inside_an_episode_restarts_the_limit(dev, R, algo):
    """300 balanced steps, reset(), 520 more: no truncation at step 500, every env truncated 500 steps after the reset"""
    case = _reset_case(R, 5)
    _reset_inside_an_episode(lambda n, slots: _make(dev, algo, n, slots), case, algo)
    _record("7_reset", algo, case)
