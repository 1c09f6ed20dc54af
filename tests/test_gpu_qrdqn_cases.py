"""The QR-DQN kernels on the synthetic cases of tests/_qrdqn_cases.py (validated on the CPU by tests/test_qrdqn_cases_cpu.py) against float64 — terminated rows,
successors across the ring's end down to slots = 2, 1 and 3 envs, batches of 1, 5, 129 and 300 rows (the last two walk several rows per workgroup) — the loss stage
alone at the edges of the Huber function, acting at 4,096 envs, and the 500-step TimeLimit cases of tests/_timelimit_cases.py through QRDQNEngine.

The reference has no qrdqn.py; the expectations here are float64 restatements of include/mi_qr.h and the CPU oracle's CartPole.  Bounds: those of tests/_qrdqn_ref.py
(8 x the f32 restatement's measured distance from torch's evaluation); nothing is excluded from a gradient comparison, action comparisons leave out the rows with
close action values (none in these cases, by their seeds)."""
import ctypes as C

import numpy as np
import pytest

import _qrdqn_cases as K
import _qrdqn_ref as X
import _timelimit_cases as T
from test_gpu_qrdqn import _make, _np, _record
from test_gpu_timelimit import _check_call, _check_ring, _checkpoint_inside_a_long_episode, _reset_case, _reset_inside_an_episode, _run_forced, _snapshot, _start

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.mark.parametrize("i", range(len(K.SHAPES)))
def test_update_on_a_synthetic_case_against_float64(i):
    import torch
    c = K.make_case(i)
    eng = _make(n=c["n_envs"], slots=c["slots"], batch_size=c["batch"], params=c["params"], target=c["target_params"])
    eng.observations.copy_(torch.from_numpy(c["obs"])); eng.actions.copy_(torch.from_numpy(c["actions"]))
    eng.rewards.copy_(torch.from_numpy(c["rewards"])); eng.terminated.copy_(torch.from_numpy(c["term"]))
    eng.global_step = c["slots"]
    eng.sample(c["idx"])
    eng.grad()
    na, tg, cur, g, loss = _np(eng.next_actions), _np(eng.target_quantiles), _np(eng.current), _np(eng.grads), float(eng.loss.item())
    far = ~c["close"]
    assert np.array_equal(na[far], c["next_actions"][far])
    same = na == c["next_actions"]
    fig = {"batch": c["batch"], "target": float(np.abs(tg - c["target"])[same].max()), "current": float(np.abs(cur - c["current"]).max()),
           "loss": abs(loss - c["loss"]) / abs(c["loss"]), "grad": float(np.abs(g - c["grad"]).max() / np.abs(c["grad"]).max()), "actions_differ": int((~same).sum())}
    _record("case_%d" % i, fig)
    assert fig["target"] <= X.BOUND_TARGET_ABS and fig["current"] <= X.BOUND_QUANT_ABS
    assert fig["loss"] <= X.BOUND_LOSS_REL and fig["grad"] <= X.BOUND_GRAD_REL
    # the fused call on the same batch steps the parameters by Adam on exactly this gradient
    p0 = c["params"].copy(); m = np.zeros_like(p0); v = np.zeros_like(p0)
    X.adam_step(p0, g, m, v, 1)
    eng.train_step(c["idx"])
    assert np.array_equal(_np(eng.grads), g) and np.abs(_np(eng.q.flat) - p0).max() <= 1e-6


def test_loss_stage_alone_at_the_edges_of_the_huber_function():
    """mi_qr_quantile_huber at u in {0, +-1, +-(1 + 2^-20), large}: the stage has no fma and a fixed order, so the f32 restatement gives its bits; float64 agrees
    to rounding — the continuous Huber has no jump at kappa or at 0 for an f32 evaluation to fall across"""
    import torch

    from deep_rl_amd import _native_qr as Q
    eps = 2.0 ** -20
    vals = np.array([0.0, 1.0, -1.0, 1.0 + eps, -(1.0 + eps), 1.0 - eps, -(1.0 - eps), 1000.0, -1000.0, 0.25, -0.25, 3.0e4], f32)
    B = 7
    cur = np.zeros((B, 64), f32)
    cur[1] = 0.5; cur[2] = -2.0                        # exactly representable shifts: u = target - current stays on the listed values
    cur[5] = np.linspace(-1, 1, 64).astype(f32)        # and two ordinary rows
    tgt = np.stack([np.roll(np.resize(vals, 64), b) for b in range(B)]).astype(f32)
    tgt[1] += f32(0.5); tgt[2] -= f32(2.0)
    tgt[6] = np.linspace(-3, 3, 64).astype(f32)
    u = tgt[:, None, :] - cur[:, :, None]
    for v in (0.0, 1.0, -1.0, 1.0 + eps, -(1.0 + eps), 1000.0, -1000.0):
        assert (u == f32(v)).any(), v
    dev = torch.device("cuda", 0)
    d_cur, d_tgt = torch.from_numpy(cur).to(dev), torch.from_numpy(tgt).to(dev)
    loss, dcur = torch.zeros(1, device=dev), torch.zeros((B, 64), device=dev)
    Q.check(Q.lib().mi_qr_quantile_huber(Q.ptr(d_cur), Q.ptr(d_tgt), B, Q.ptr(loss), Q.ptr(dcur), Q.stream_ptr(dev)), "mi_qr_quantile_huber")
    rl, d = X.huber_rows(cur, tgt)
    want = f32(X.sum_rows_ascending(rl) * (f32(1.0) / f32(B * 64)))
    assert f32(loss.item()) == want and np.array_equal(_np(dcur), d)
    l64, d64 = X.huber64(cur, tgt)
    assert abs(float(loss.item()) - l64) <= 1e-6 * l64 and np.abs(_np(dcur) - d64).max() <= 1e-6 * np.abs(d64).max()
    # one row, one target value: the gradient of quantile i at u = 0 is 0, at |u| >= 1 it is -+ w / (B * 64) per target
    one_c, one_t = torch.zeros((1, 64), device=dev), torch.full((1, 64), 1.0, device=dev)
    l1, d1 = torch.zeros(1, device=dev), torch.zeros((1, 64), device=dev)
    Q.check(Q.lib().mi_qr_quantile_huber(Q.ptr(one_c), Q.ptr(one_t), 1, Q.ptr(l1), Q.ptr(d1), Q.stream_ptr(dev)), "mi_qr_quantile_huber")
    assert np.array_equal(_np(d1)[0], -X.TAUS) and f32(l1.item()) == f32(0.5 * X.TAUS.astype(np.float64).sum())    # u = 1: L = 0.5, c = 1, w = tau_i; 64 targets / 64
    Q.check(Q.lib().mi_qr_quantile_huber(Q.ptr(one_c), Q.ptr(one_c), 1, Q.ptr(l1), Q.ptr(d1), Q.stream_ptr(dev)), "mi_qr_quantile_huber")
    assert not _np(d1).any() and l1.item() == 0.0


def _episode_figures(term):
    """(steps,) terminated flags of one env that started a fresh episode at step 0 -> (finished episodes, sum of their lengths, longest)"""
    ends = np.flatnonzero(term)
    lens = np.diff(np.concatenate([[-1], ends]))
    return len(ends), int(lens.sum()), int(lens.max()) if len(ends) else 0


def test_acting_at_4096_envs_matches_single_env_engines():
    """the scaled acting size: 4,096 envs share 1,024 workgroups (each walks four envs); spot-checked envs act exactly as N = 1 engines keyed with their ids, and the
    launch's episode statistics are the sums over the envs of what the ring itself shows.  32 steps from fresh episodes: no TimeLimit truncation"""
    p = X.load_ckpt(4000)["params_before"]
    S, Ts, g0 = 34, 32, 13_160
    kw = dict(slots=S, params=p)
    big = _make(n=4096, **kw)
    big.global_step = g0
    big.reset()
    big.act(Ts)
    A, O, Tm = _np(big.actions), _np(big.observations), _np(big.terminated)
    term = Tm[(g0 + 1 + np.arange(Ts)) % S]                 # step s's flag lies in slot (g0 + s + 1) % slots
    per_env = np.array([_episode_figures(term[:, E]) for E in range(4096)])
    for E in (0, 1023, 1024, 4095):
        one = _make(n=1, env_id_base=E, **kw)
        one.global_step = g0
        one.reset()
        one.act(Ts)
        assert np.array_equal(_np(one.actions)[:, 0], A[:, E]) and np.array_equal(_np(one.observations)[:, 0], O[:, E])
        assert _np(one.episode_stats)[:3].tolist() == per_env[E].tolist()
    st = _np(big.episode_stats).tolist()
    assert per_env[:, 0].sum() >= 400                      # the case has episodes to count
    assert st[:3] == [int(per_env[:, 0].sum()), int(per_env[:, 1].sum()), int(per_env[:, 2].max())] and st[3] == 0   # (no episode log at this size)
    assert big.global_step == g0 + Ts


# ---- the 500-step TimeLimit (tests/_timelimit_cases.py) through QRDQNEngine ---------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def _tl_make(dev, n, slots, params=None, greedy=False):
    import deep_rl_amd as D
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=5, env_id_base=300)
    q, tgt = D.QRQNetwork(env), D.QRQNetwork(env)
    q.load_flat(np.zeros(X.NPARAMS, f32) if params is None else params)
    tgt.load_state_dict(q.state_dict())
    kw = dict(start_e=0.0, end_e=0.0) if greedy else {}
    return D.QRDQNEngine(env, q, tgt, D.Adam(q, lr=2.5e-4, eps=0.01 / 128), slots=slots, max_episodes_logged=8192, **kw)


@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
def test_teacher_forced_acting_at_the_limit(dev, forced, schedule):
    """1,100 steps of the scripted 5-env case: one run on a ring that holds the whole run, compared at the end; one on 16 slots, compared after every call"""
    case = T.get("n5", forced)
    call_list = T.calls(schedule, case.steps)
    for slots, every in ((case.steps + 1, False), (16, True)):
        eng = _tl_make(dev, case.n, slots)
        _start(eng, case)
        _run_forced(eng, case, call_list, slots, every, ("qrdqn", forced, schedule, slots))
        if slots > case.steps:      # the stored flag is `terminated`, not `done`: the two differ exactly on the truncated steps
            differ = _np(eng.terminated)[1:] != case.done.astype(np.uint8)
            assert np.array_equal(differ, case.trunc) and differ.sum() == case.counts()["truncations"] >= 2


@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
def test_two_envs_per_workgroup_at_the_limit(dev, forced, schedule):
    """1,030 envs on a grid capped at 1,024 workgroups: workgroups 0 - 5 walk two long-episode envs each; all 1,030 envs are compared"""
    case = T.get("n1030", forced)
    slots, every = (16, True) if schedule == "7" else (case.steps + 1, False)
    eng = _tl_make(dev, case.n, slots)
    _start(eng, case)
    _run_forced(eng, case, T.calls(schedule, case.steps), slots, every, ("qrdqn", forced, schedule, slots))


def controller_qr(Kc):
    """QRQNetwork: units 0 / 1 of layer 1 are relu(+-w . obs), carried through layer 2 to all 64 quantiles of actions 1 / 0 with weight K: q_1 - q_0 = K (w . obs)"""
    p = np.zeros(X.NPARAMS, f32)
    W1 = p[0:480].reshape(120, 4); W2 = p[600:10680].reshape(84, 120); W3 = p[10764:21516].reshape(128, 84)
    W1[0] = T.RULE_W; W1[1] = -T.RULE_W
    W2[0, 0] = 1; W2[1, 1] = 1
    W3[64:128, 0] = Kc; W3[0:64, 1] = Kc
    return p


def test_greedy_controller_runs_into_the_limit(dev):
    """FORCED = false: a hand-built controller network acts greedily (through the collapsed head) for 1,100 steps.  The device's own actions are replayed on the
    oracle: ring, flags, statistics, log and `elapsed` exact; the action is (q_1 > q_0) of a float64 forward wherever the two values are at least CLOSE_Q apart (at
    most 1 % left out); at least one env is truncated twice."""
    from oracle import cpu_ref as R
    n, steps = 5, 1100
    slots = steps + 1
    params = controller_qr(T.CONTROLLER_K)
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
        _check_call(snap, case, g, k, "qrdqn")
        g += k
    _check_ring(eng, case, steps, slots, "qrdqn")
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    q = X.forward64(params, case.obs[:-1].reshape(-1, 4))[1]
    far = np.abs(q[:, 1] - q[:, 0]) >= X.CLOSE_Q
    assert (~far).mean() <= 0.01, int((~far).sum())
    assert np.array_equal(actions.reshape(-1)[far], (q[:, 1] > q[:, 0]).astype(np.int64)[far])


def test_checkpoint_inside_a_long_episode(dev, tmp_path):
    """saved at global step 300 of the 5-env case, loaded into a fresh engine whose env was driven somewhere else, continued to step 620: ring, `elapsed`, log and
    statistics equal the uninterrupted run bit for bit, and the truncation comes at step 500 (the body of tests/test_gpu_timelimit.py's test)"""
    _checkpoint_inside_a_long_episode(lambda n, slots, params=None: _tl_make(dev, n, slots, params=params), T.get("n5", False), X.NPARAMS, str(tmp_path / "qrdqn"), "qrdqn")


def test_reset_inside_an_episode_restarts_the_limit(dev):
    """300 balanced steps, reset(), 520 more: no truncation at step 500, every env truncated 500 steps after the reset"""
    from oracle import cpu_ref as R
    _reset_inside_an_episode(lambda n, slots: _tl_make(dev, n, slots), _reset_case(R, 5), "qrdqn")
