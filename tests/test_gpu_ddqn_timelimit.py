"""The 500-step TimeLimit inside ddqn_act_kernel: the cases of tests/_timelimit_cases.py (validated on the CPU by tests/test_timelimit_cases_cpu.py) through
DoubleDQNEngine, with the helpers of tests/test_gpu_timelimit.py as tests/test_gpu_qrdqn_cases.py uses them.  Truncation at elapsed = 500 stores terminated = 0 and
the reset observation; `elapsed`, the episode log and the launch statistics follow the oracle across calls, ring wraps, a checkpoint and a reset()."""
import numpy as np
import pytest

import _timelimit_cases as T
from test_gpu_timelimit import _check_call, _check_ring, _checkpoint_inside_a_long_episode, _np, _reset_case, _reset_inside_an_episode, _run_forced, _snapshot, _start

pytestmark = pytest.mark.gpu
f32 = np.float32
NPARAMS = 10934


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _tl_make(dev, n, slots, params=None, greedy=False):
    """params: the flat parameter vector (default: zeros — the teacher-forced paths run no forward); greedy: epsilon 0 and no learning_starts from step 0"""
    import deep_rl_amd as D
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=5, env_id_base=300)
    q, tgt = D.QNetwork(env), D.QNetwork(env)
    q.load_flat(np.zeros(NPARAMS, f32) if params is None else params)
    tgt.load_state_dict(q.state_dict())
    kw = dict(learning_starts=0, start_e=0.0, end_e=0.0) if greedy else {}
    return D.DoubleDQNEngine(env, q, tgt, D.Adam(q, lr=2.5e-4), slots=slots, max_episodes_logged=8192, **kw)


@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
def test_teacher_forced_acting_at_the_limit(dev, forced, schedule):
    """1,100 steps of the scripted 5-env case: one run on a ring that holds the whole run, compared at the end; one on 16 slots, compared after every call"""
    case = T.get("n5", forced)
    call_list = T.calls(schedule, case.steps)
    for slots, every in ((case.steps + 1, False), (16, True)):
        eng = _tl_make(dev, case.n, slots)
        _start(eng, case)
        _run_forced(eng, case, call_list, slots, every, ("ddqn", forced, schedule, slots))
        if slots > case.steps:      # the stored flag is `terminated`, not `done`: the two differ exactly on the truncated steps
            differ = _np(eng.terminated)[1:] != case.done.astype(np.uint8)
            assert np.array_equal(differ, case.trunc) and differ.sum() == case.counts()["truncations"] >= 2
            trunc_step, trunc_env = np.nonzero(case.trunc)      # a truncated step leaves terminated = 0 and the RESET observation in the next slot
            assert not _np(eng.terminated)[1:][trunc_step, trunc_env].any()
            assert np.array_equal(_np(eng.observations)[1:][trunc_step, trunc_env], case.obs[1:][trunc_step, trunc_env])


@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
def test_two_envs_per_workgroup_at_the_limit(dev, forced, schedule):
    """1,030 envs on a grid capped at 1,024 workgroups: workgroups 0 - 5 walk two long-episode envs each; all 1,030 envs are compared"""
    case = T.get("n1030", forced)
    slots, every = (16, True) if schedule == "7" else (case.steps + 1, False)
    eng = _tl_make(dev, case.n, slots)
    _start(eng, case)
    _run_forced(eng, case, T.calls(schedule, case.steps), slots, every, ("ddqn", forced, schedule, slots))


def test_greedy_controller_runs_into_the_limit(dev):
    """FORCED = false: DQN's hand-built controller network (q_1 - q_0 = K w . obs) acts greedily for 1,100 steps.  The device's own actions are replayed on the
    oracle: ring, flags, statistics, log and `elapsed` exact; the action is (q_1 > q_0) of a float64 forward wherever the two values are at least DQN's close-value
    distance apart (at most 1 % left out); at least one env is truncated twice."""
    from oracle import cpu_ref as R
    n, steps = 5, 1100
    slots = steps + 1
    params = T.CONTROLLERS["dqn"](T.CONTROLLER_K)
    eng = _tl_make(dev, n, slots, params=params, greedy=True)
    eng.reset()
    snaps, call_list = [], T.calls("49+50", steps)
    for k in call_list:
        eng.act(k)
        snaps.append(_snapshot(eng))
    actions = _np(eng.actions)[:steps]
    assert set(np.unique(actions).tolist()) == {0, 1}
    case = T.replay(R, n, 5, 300, actions)
    g = 0
    for k, snap in zip(call_list, snaps):
        _check_call(snap, case, g, k, "ddqn")
        g += k
    _check_ring(eng, case, steps, slots, "ddqn")
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    q = T.q64("dqn", params, case.obs[:-1].reshape(-1, 4))
    far = np.abs(q[:, 1] - q[:, 0]) >= T.close_q("dqn")
    assert (~far).mean() <= 0.01, int((~far).sum())
    assert np.array_equal(actions.reshape(-1)[far], (q[:, 1] > q[:, 0]).astype(np.int64)[far])


def test_checkpoint_inside_a_long_episode(dev, tmp_path):
    """saved at global step 300 of the 5-env case, loaded into a fresh engine whose env was driven somewhere else, continued to step 620: ring, `elapsed`, log and
    statistics equal the uninterrupted run bit for bit, and the truncation comes at step 500 (the body of tests/test_gpu_timelimit.py's test)"""
    _checkpoint_inside_a_long_episode(lambda n, slots, params=None: _tl_make(dev, n, slots, params=params), T.get("n5", False), NPARAMS, str(tmp_path / "ddqn"), "ddqn")


def test_reset_inside_an_episode_restarts_the_limit(dev):
    """300 balanced steps, reset(), 520 more: no truncation at step 500, every env truncated 500 steps after the reset"""
    from oracle import cpu_ref as R
    _reset_inside_an_episode(lambda n, slots: _tl_make(dev, n, slots), _reset_case(R, 5), "ddqn")
