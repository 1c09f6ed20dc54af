"""QR-DQN on the MI355X (libmirl_qr.so, include/mi_qr.h) against the fixtures (tests/golden/qrdqn_ref_*.npz) and the numpy restatement (tests/_qrdqn_ref.py).

The reference has no qrdqn.py: the fixtures are the run of the same algorithm written as a plain torch script (tools/capture_qrdqn_ref.py), torch standing in for it.

Tolerances.  The fixtures are torch's own f32 evaluation; the restatement and the device are two more f32 evaluations in other summation orders.
tests/test_qrdqn_ref_cpu.py measures the restatement against the fixtures at every checkpoint (the MEASURED_* constants of tests/_qrdqn_ref.py); each device bound
is 8 x its figure.  Action comparisons leave out rows whose two action values are closer than twice the q bound, at most 1 % of a case's rows; gradient comparisons
leave out nothing.  Observed maxima go to qrdqn_gpu_maxima.json in the tests' results directory (committed as profiles/qrdqn_gpu_maxima.json)."""
import json
import os

import numpy as np
import pytest

import _qrdqn_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32
T = X.T_STEPS


def _record(key, value):
    path = os.path.join(X.results_dir(), "qrdqn_gpu_maxima.json")
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec[key] = value
    json.dump(rec, open(path, "w"), indent=1)
    print(key, json.dumps(value))


def _np(t):
    return t.detach().cpu().numpy()


def _make(n=1, slots=T + 1, seed=1, env_id_base=0, batch_size=128, params=None, target=None, **kw):
    import torch

    import deep_rl_amd as D

    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=env_id_base)
    torch.manual_seed(seed)
    q = D.QRQNetwork(env, n_quantiles=64)
    opt = D.Adam(q, lr=2.5e-4, eps=0.01 / 128)
    tq = D.QRQNetwork(env, n_quantiles=64)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    kw.setdefault("total_timesteps", T)
    return D.QRDQNEngine(env, q, tq, opt, slots=slots, batch_size=batch_size, **kw)


@pytest.fixture(scope="module")
def trace():
    return X.load_trace()


@pytest.fixture(scope="module")
def ringv(trace):
    return X.ring(trace)


@pytest.fixture(scope="module")
def ckpts():
    return {k: X.load_ckpt(k) for k in X.CHECKPOINTS}


def _load_ring(eng, ringv, global_step=T):
    import torch
    obs, actions, rewards, term = ringv
    eng.observations.copy_(torch.from_numpy(obs).reshape(eng.observations.shape))
    eng.actions.copy_(torch.from_numpy(actions).reshape(eng.actions.shape))
    eng.rewards.copy_(torch.from_numpy(rewards).reshape(eng.rewards.shape))
    eng.terminated.copy_(torch.from_numpy(term).reshape(eng.terminated.shape))
    eng.global_step = global_step


@pytest.fixture(scope="module")
def ring_engine(ringv):
    eng = _make()
    _load_ring(eng, ringv)
    return eng


def test_initial_weights_and_forward_against_the_checkpoints(trace, ringv, ckpts):
    """the seeded network is the fixture's; with a checkpoint's parameters the forward API gives torch's `current` within the quantile bound and, through the
    collapsed head, float64's action values within the q bound (and the mean of its own quantiles)"""
    import torch
    eng = _make()
    assert np.array_equal(_np(eng.q.flat), trace["init_params"]) and np.array_equal(_np(eng.target_network.flat), trace["init_params"])
    assert eng.q.flat.numel() == 21_644 and [tuple(p.shape) for p in eng.q.parameters()] == [(120, 4), (120,), (84, 120), (84,), (128, 84), (128,)]
    worst = {"quant": 0.0, "q": 0.0, "q_vs_mean": 0.0}
    for k, c in ckpts.items():
        Xb, A, _Xn, _Rw, _Tm = X.batch_of(ringv, c["batch_inds"])
        eng.q.load_flat(c["params_before"])
        th = _np(eng.q.get_quantiles(torch.from_numpy(Xb)))
        q = _np(eng.q.get_q_values(torch.from_numpy(Xb)))
        assert th.shape == (128, 2, 64) and q.shape == (128, 2)
        th64, q64, _z1, _z2 = X.forward64(c["params_before"], Xb)
        worst["quant"] = max(worst["quant"], float(np.abs(th[np.arange(128), A] - c["current"]).max()), float(np.abs(th - th64).max()))
        worst["q"] = max(worst["q"], float(np.abs(q - q64).max()))
        worst["q_vs_mean"] = max(worst["q_vs_mean"], float(np.abs(q - th.astype(np.float64).mean(-1)).max()))
    _record("forward", dict(worst, quant_bound=X.BOUND_QUANT_ABS, q_bound=X.BOUND_Q_ABS))
    assert worst["quant"] <= X.BOUND_QUANT_ABS and worst["q"] <= X.BOUND_Q_ABS and worst["q_vs_mean"] <= X.BOUND_Q_ABS


def test_teacher_forced_acting_reproduces_the_ring_and_every_printed_line(trace, ringv):
    """the trace's first 3,000 steps under its actions and reset states: the ring bit for bit, every printed line"""
    import torch
    t, n = trace, 3_000
    eng = _make(max_episodes_logged=40)
    eng.reset(torch.from_numpy(t["reset_states"][0].reshape(1, 4)))
    fa = torch.from_numpy(t["actions"][:n].astype(np.int64)).reshape(-1, 1).to(eng.device)
    fr = torch.from_numpy(X.forced_resets(t)[:n]).reshape(-1, 1, 4).to(eng.device)
    lines = []
    for g in range(0, n, 10):
        eng.act(10, forced_actions=fa[g:g + 10], forced_resets=fr[g:g + 10])
        for _e, s, r, _l in eng.drain_episodes()[1]:
            lines.append("global_step=%d, episodic_return=%s" % (g + s + 1, r))
    obs, actions, rewards, term = ringv
    assert np.array_equal(_np(eng.observations)[:n + 1, 0], obs[:n + 1]) and np.array_equal(_np(eng.actions)[:n, 0], actions[:n])
    assert np.array_equal(_np(eng.rewards)[:n + 1, 0], rewards[:n + 1]) and np.array_equal(_np(eng.terminated)[:n + 1, 0], term[:n + 1])
    assert not _np(eng.observations)[n + 1:].any()
    want = ["global_step=%d, episodic_return=%s" % (int(s), float(r)) for s, r in zip(t["episode_global_step"], t["episode_return"]) if s <= n]
    assert lines == want and len(lines) > 100 and lines[0].endswith(".0") and lines[0].split("=")[-1].count(".") == 1
    assert np.array_equal(_np(eng.observation)[0], obs[n])


def test_production_exploration_draws_follow_the_keyed_stream(ckpts):
    """env E of an N = 5 engine acts exactly as an N = 1 engine with env_id_base = E, and every step is the keyed split of the contract (stream 3, idx = the env step
    counter): an exploring step takes the keyed random action, a greedy one exactly the argmax of the forward API's action values on the ring's observation"""
    kw = dict(slots=70, params=ckpts[4000]["params_before"])
    big = _make(n=5, **kw)
    g0 = 13_160                                  # epsilon = 1 - 0.95 * 13,160 / 25,000 = 0.49992
    big.global_step = g0
    big.reset()
    big.act(64)
    A5, O5, T5 = _np(big.actions), _np(big.observations), _np(big.terminated)
    slots = (g0 + np.arange(64)) % 70
    n_explore = n_greedy = 0
    for E in range(5):
        one = _make(n=1, env_id_base=E, **kw)
        one.global_step = g0
        one.reset()
        one.act(64)
        assert np.array_equal(_np(one.actions)[:, 0], A5[:, E]) and np.array_equal(_np(one.observations)[:, 0], O5[:, E]) and np.array_equal(_np(one.terminated)[:, 0], T5[:, E])
        assert np.array_equal(_np(one.observation)[0], _np(big.observation)[E])
        u, ra = X.explore_draws(1, E, np.arange(64))
        explore = u < np.maximum(-0.95 / 25_000 * (g0 + np.arange(64)) + 1.0, 0.05)
        q = _np(big.q.get_q_values(big.observations[slots, E]))
        assert np.array_equal(A5[slots, E], np.where(explore, ra, (q[:, 1] > q[:, 0]).astype(np.int64)))
        n_explore += int(explore.sum()); n_greedy += int((~explore).sum())
    assert n_explore >= 5 * 64 * 0.3 and n_greedy >= 5 * 64 * 0.3


@pytest.mark.parametrize("k", X.CHECKPOINTS)
def test_checkpoint_target_and_gradient(k, ring_engine, ringv, ckpts):
    eng, c = ring_engine, ckpts[k]
    eng.q.load_flat(c["params_before"]); eng.target_network.load_flat(c["target_params"])
    eng.sample(c["batch_inds"].astype(np.int64))
    eng.target()
    tg_alone, na_alone = _np(eng.target_quantiles).copy(), _np(eng.next_actions).copy()
    eng.grad()
    tg, na, cur, g, loss = _np(eng.target_quantiles), _np(eng.next_actions), _np(eng.current), _np(eng.grads), float(eng.loss.item())
    assert np.array_equal(tg, tg_alone) and np.array_equal(na, na_alone)            # mi_qr_target is the gradient launch's first pass
    Xb, A, Xn, Rw, Tm = X.batch_of(ringv, c["batch_inds"])
    q64 = X.forward64(c["target_params"], Xn)[1]
    far = np.abs(q64[:, 0] - q64[:, 1]) >= X.CLOSE_Q
    assert (~far).mean() <= X.MAX_EXCLUDED and np.array_equal(na[far], c["next_actions"][far])
    same = na == c["next_actions"]
    fig = {"target": float(np.abs(tg - c["target"])[same].max()), "current": float(np.abs(cur - c["current"]).max()),
           "loss": abs(loss - c["loss"][0]) / abs(c["loss"][0]), "grad": float(np.abs(g - c["grads"]).max() / np.abs(c["grads"]).max()),
           "rows_excluded": int((~far).sum()), "actions_differ": int((~same).sum())}
    # the loss stage has no fma: from the device's own current and target the restatement gives the device's loss bit for bit
    rl, _d = X.huber_rows(cur, tg)
    fig["loss_bit_exact"] = bool(f32(X.sum_rows_slabs(rl) * (f32(1.0) / f32(128 * 64))) == f32(loss))
    _record("checkpoint_%d" % k, fig)
    assert fig["target"] <= X.BOUND_TARGET_ABS and fig["current"] <= X.BOUND_QUANT_ABS
    assert fig["loss"] <= X.BOUND_LOSS_REL
    assert fig["grad"] <= X.BOUND_GRAD_REL
    assert fig["loss_bit_exact"]


def test_first_51_updates_chained_on_the_device(trace, ringv, ckpts):
    """from the initial parameters, the fixture's batch_inds, across the target syncs at global_step 10,000 and 10,500: every loss and the parameters behind update 50"""
    eng = _make()
    _load_ring(eng, ringv)
    worst = 0.0
    for k in range(51):
        eng.train_step(trace["batch_inds"][k].astype(np.int64))
        worst = max(worst, abs(float(eng.loss.item()) - trace["loss"][k]) / abs(trace["loss"][k]))
        if k == 0:
            assert np.abs(_np(eng.q.flat) - ckpts[0]["params_after"]).max() <= X.BOUND_PARAMS_ABS
        if (10_000 + 10 * k) % 500 == 0:
            eng.sync_target()
    dp = float(np.abs(_np(eng.q.flat) - ckpts[50]["params_after"]).max())
    _record("chain_51", {"loss_rel": worst, "loss_bound": X.BOUND_CHAIN_LOSS_REL, "params_abs": dp, "params_bound": X.BOUND_PARAMS_ABS})
    assert eng.optimizer.step_count == 51 and np.array_equal(_np(eng.target_network.flat), _np(eng.q.flat))
    assert worst <= X.BOUND_CHAIN_LOSS_REL and dp <= X.BOUND_PARAMS_ABS


def test_fused_update_is_bitwise_the_unfused_sequence_and_repeatable(ringv):
    """mi_qr_update (in-launch index draw, Adam on the slab sum) against sample() (libmirl's mi_dqn_sample) + grad() + deep_rl_amd.Adam.step over 4 updates with a
    target sync between them; the same four updates once more give the same bits"""
    a, b = _make(), _make()
    for eng in (a, b):
        _load_ring(eng, ringv, global_step=15_000)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        assert np.array_equal(_np(a.batch_inds), _np(b.batch_inds)) and _np(a.batch_inds).max() < 15_000   # the in-launch draw is mi_dqn_sample's
        for x, y in ((a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
                     (a.target_quantiles, b.target_quantiles), (a.current, b.current), (a.next_actions, b.next_actions)):
            assert np.array_equal(_np(x), _np(y))
        if u == 1:
            a.sync_target(); b.sync_target()
    assert a.optimizer.step_count == b.optimizer.step_count == 4 and a.update_index == 4
    assert not np.array_equal(_np(a.q.flat), _np(a.target_network.flat)) and np.isfinite(_np(a.q.flat)).all()
    c = _make()
    _load_ring(c, ringv, global_step=15_000)
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat)) and np.array_equal(_np(c.grads), _np(a.grads)) and np.array_equal(_np(c.loss), _np(a.loss))


def test_checkpoint_resume_is_bit_exact(tmp_path, ringv):
    from deep_rl_amd import checkpoint
    a = _make()
    _load_ring(a, ringv, global_step=15_000)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "qrdqn"), a)
    b = _make()
    b.reset()
    checkpoint.load(path, b)
    assert b.global_step == a.global_step == 15_030 and b.update_index == 3 and b.optimizer.step_count == 3
    for u in range(3):
        for eng in (a, b):
            eng.act(10); eng.train_step()
            if u == 1:
                eng.sync_target()
    for x, y in ((a.q.flat, b.q.flat), (a.target_network.flat, b.target_network.flat), (a.observations, b.observations), (a.actions, b.actions), (a.terminated, b.terminated),
                 (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.observation, b.observation)):
        assert np.array_equal(_np(x), _np(y))


def test_errors_are_loud():
    import torch

    import deep_rl_amd as D
    from deep_rl_amd import _native as N
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=1, device=dev, seed=1)
    with pytest.raises(N.MiError):
        D.QRQNetwork(env, n_quantiles=32)
    with pytest.raises(N.MiError):
        D.QRQNetwork(D.make("Pendulum-v1", num_envs=1, device=dev, seed=1))
    eng = _make()
    eng.reset()
    with pytest.raises(N.MiError):
        eng.train_step()                         # empty ring
    with pytest.raises(N.MiError):
        eng.act(65)
