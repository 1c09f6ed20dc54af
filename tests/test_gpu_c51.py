"""C51 on the MI355X (libmirl_c51.so, include/mi_c51.h) against the unmodified reference (tests/golden/c51_ref_trace.npz, c51_ref_ckpt*.npz) and the numpy
restatement (tests/_c51_ref.py).

Tolerances.  The fixtures are the reference's own f32 evaluation; the restatement and the device are two more f32 evaluations in other summation orders.
tests/test_c51_ref_pinned_cpu.py measures the restatement against the fixtures at every checkpoint (the MEASURED_* constants of tests/_c51_ref.py); each device
bound is 8 x its figure.  Action comparisons leave out rows whose two action values are closer than twice the q bound, at most 1 % of a case's rows; gradient
comparisons leave out nothing.  Observed maxima go to c51_gpu_maxima.json in the tests' results directory and into docs/LEDGER.md."""
import json
import os

import numpy as np
import pytest

import _c51_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32


def _record(key, value):
    path = os.path.join(X.results_dir(), "c51_gpu_maxima.json")
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec[key] = value
    json.dump(rec, open(path, "w"), indent=1)
    print(key, json.dumps(value))


def _np(t):
    return t.detach().cpu().numpy()


def _make(n=1, slots=20_001, seed=1, env_id_base=0, batch_size=128, params=None, target=None, **kw):
    import torch

    import deep_rl_amd as D

    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=env_id_base)
    torch.manual_seed(seed)
    q = D.C51QNetwork(env, n_atoms=101)
    opt = D.Adam(q, lr=2.5e-4, eps=0.01 / 128)
    tq = D.C51QNetwork(env, n_atoms=101)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    kw.setdefault("total_timesteps", 20_000)
    return D.C51Engine(env, q, tq, opt, slots=slots, batch_size=batch_size, **kw)


@pytest.fixture(scope="module")
def trace():
    return X.load_trace()


@pytest.fixture(scope="module")
def ringv(trace):
    return X.ring(trace)


def _load_ring(eng, ringv, global_step=20_000):
    import torch
    obs, actions, rewards, term = ringv
    eng.observations.copy_(torch.from_numpy(obs).reshape(eng.observations.shape))
    eng.actions.copy_(torch.from_numpy(actions).reshape(eng.actions.shape))
    eng.rewards.copy_(torch.from_numpy(rewards).reshape(eng.rewards.shape))
    eng.terminated.copy_(torch.from_numpy(term).reshape(eng.terminated.shape))
    eng.global_step = global_step


def test_initial_weights_are_the_references(trace):
    eng = _make()
    assert np.array_equal(_np(eng.q.flat), trace["init_params"]) and np.array_equal(_np(eng.target_network.flat), trace["init_params"])
    assert eng.q.flat.numel() == 27_934 and [tuple(p.shape) for p in eng.q.parameters()] == [(120, 4), (120,), (84, 120), (84,), (202, 84), (202,)]
    p = eng.q.get_probs(eng.reset())
    assert tuple(p.shape) == (1, 2, 101) and np.abs(_np(p).sum(-1) - 1).max() < 1e-5


def test_teacher_forced_acting_reproduces_the_ring_and_every_printed_line(trace, ringv):
    import torch
    t = trace
    eng = _make(max_episodes_logged=40)
    eng.reset(torch.from_numpy(t["reset_states"][0].reshape(1, 4)))
    fa = torch.from_numpy(t["actions"].astype(np.int64)).reshape(-1, 1).to(eng.device)
    fr = torch.from_numpy(X.forced_resets(t)).reshape(-1, 1, 4).to(eng.device)
    lines = []
    for g in range(0, 20_000, 10):
        eng.act(10, forced_actions=fa[g:g + 10], forced_resets=fr[g:g + 10])
        for _e, s, r, _l in eng.drain_episodes()[1]:
            lines.append("global_step=%d, episodic_return=%s" % (g + s + 1, r))
    obs, actions, rewards, term = ringv
    assert np.array_equal(_np(eng.observations)[:, 0], obs) and np.array_equal(_np(eng.actions)[:, 0], actions)
    assert np.array_equal(_np(eng.rewards)[:, 0], rewards) and np.array_equal(_np(eng.terminated)[:, 0], term)
    want = ["global_step=%d, episodic_return=%s" % (int(s), float(r)) for s, r in zip(t["episode_global_step"], t["episode_return"])]
    assert lines == want and len(lines) == 1504 and lines[0].split("=")[-1].count(".") == 1 and lines[0].endswith(".0")   # the reference prints 22.0, not 22.00
    assert np.array_equal(_np(eng.observation)[0], obs[20_000])


def _greedy_cases(trace, k):
    c = X.load_ckpt(k)
    g0 = 10_000 + 10 * k
    greedy = np.flatnonzero(trace["greedy"])
    return [(c["params_before"], greedy[(greedy >= g0 - 10) & (greedy < g0)]), (c["params_after"], greedy[(greedy >= g0) & (greedy < g0 + 10)])]


def test_greedy_decisions_at_the_checkpoints(trace, ringv):
    """with the reference's online parameters loaded, the device decides as the reference did wherever it acted greedily (the chunk in front of and behind every
    checkpoint update)"""
    import torch
    eng = _make()
    obs = ringv[0]
    n = close = 0
    worst_q = 0.0
    for k in X.CHECKPOINTS:
        for params, steps in _greedy_cases(trace, k):
            if len(steps) == 0:
                continue
            eng.q.load_flat(params)
            q = _np(eng.q.get_q_values(torch.from_numpy(obs[steps])))
            q64 = X.forward64(params, obs[steps])[1]
            worst_q = max(worst_q, float(np.abs(q - q64).max()))
            far = np.abs(q64[:, 0] - q64[:, 1]) >= X.CLOSE_Q
            assert np.array_equal((q[:, 1] > q[:, 0])[far], trace["actions"][steps][far] == 1)
            n += len(steps); close += int((~far).sum())
    _record("greedy", {"rows": n, "excluded": close, "q_abs": worst_q, "q_bound": X.BOUND_Q_ABS})
    assert n >= 50 and close <= X.MAX_EXCLUDED * n
    assert worst_q <= X.BOUND_Q_ABS


def test_acting_kernel_greedy_branch_decides_as_the_reference(trace, ringv):
    """the acting launch's OWN greedy branch (epsilon = 0: start_e = end_e = 0): one env per greedy decision of the reference around the checkpoints, started in that
    decision's observation.  Step 0 must be the fixture's action (close-value exclusion); every one of the 4 steps must be, exactly and with nothing left out, the
    argmax of the forward API's action values on the observation the ring holds for that step — a stale or foreign observation in the carried state would show"""
    import torch
    obs = ringv[0]
    n = close = 0
    for k in X.CHECKPOINTS:
        for params, steps in _greedy_cases(trace, k):
            if len(steps) == 0:
                continue
            eng = _make(n=len(steps), slots=6, params=params, start_e=0.0, end_e=0.0)
            eng.reset(torch.from_numpy(obs[steps].astype(np.float64)))       # f32 -> f64 -> f32 is exact: the env's observation is the fixture's
            assert np.array_equal(_np(eng.observation), obs[steps])
            eng.act(4)
            A = _np(eng.actions)
            far = np.abs(np.subtract(*X.forward64(params, obs[steps])[1].T)) >= X.CLOSE_Q
            assert np.array_equal(A[0][far], trace["actions"][steps][far])
            for s in range(4):
                q = _np(eng.q.get_q_values(eng.observations[s]))
                assert np.array_equal(A[s], (q[:, 1] > q[:, 0]).astype(np.int64))
            assert np.array_equal(_np(eng.observation), _np(eng.observations[4]))
            n += len(steps); close += int((~far).sum())
    assert n >= 50 and close <= X.MAX_EXCLUDED * n


@pytest.fixture(scope="module")
def ring_engine(ringv):
    eng = _make()
    _load_ring(eng, ringv)
    return eng


@pytest.mark.parametrize("k", X.CHECKPOINTS)
def test_checkpoint_update_from_the_references_parameters(k, ring_engine, ringv):
    eng = ring_engine
    c = X.load_ckpt(k)
    eng.q.load_flat(c["params_before"]); eng.target_network.load_flat(c["target_params"])
    eng.sample(c["batch_inds"].astype(np.int64))
    eng.target()
    tp_alone, na_alone = _np(eng.target_probs).copy(), _np(eng.next_actions).copy()
    eng.grad()
    tp, na, pr, g, loss = _np(eng.target_probs), _np(eng.next_actions), _np(eng.probs), _np(eng.grads), float(eng.loss.item())
    assert np.array_equal(tp, tp_alone) and np.array_equal(na, na_alone)            # mi_c51_target is the gradient launch's first pass
    Xb, A, Xn, Rw, Tm = X.batch_of(ringv, c["batch_inds"])
    q64 = X.forward64(c["target_params"], Xn)[1]
    far = np.abs(q64[:, 0] - q64[:, 1]) >= X.CLOSE_Q
    assert (~far).mean() <= X.MAX_EXCLUDED and np.array_equal(na[far], c["next_actions"][far])
    same = na == c["next_actions"]
    fig = {
        "target_probs": float(np.abs(tp - c["target_probs"])[same].max()), "probs": float(np.abs(pr - c["probs"]).max()),
        "loss": abs(loss - c["loss"][0]) / abs(c["loss"][0]), "grad": float(np.abs(g - c["grads"]).max() / np.abs(c["grads"]).max()),
        "sum_target_probs": float(np.abs(tp.sum(-1) - 1).max()), "rows_excluded": int((~far).sum()), "actions_differ": int((~same).sum()),
    }
    # the f32 restatement's own error on the same update, through its own targets
    _a, m32, _q = X.target(c["target_params"], Xn, Rw, Tm)
    _l, g32, _p = X.loss_grad(c["params_before"], Xb, A, m32)
    fig["grad_restated"] = float(np.abs(g32 - c["grads"]).max() / np.abs(c["grads"]).max())
    # the restatement's path through the device's own next_probs: the projection alone
    _record("checkpoint_%d" % k, fig)
    assert fig["target_probs"] <= X.BOUND_TARGET_PROBS_ABS and fig["probs"] <= X.BOUND_PROBS_ABS
    assert fig["loss"] <= X.BOUND_LOSS_REL
    assert fig["grad"] <= X.BOUND_GRAD_REL
    assert fig["grad"] <= 8 * fig["grad_restated"]
    assert fig["sum_target_probs"] < 1e-5


def test_device_projection_is_the_restatements_bit_for_bit(ring_engine, ringv):
    """the device's target_probs are project() of the device's own next_probs, bit for bit: the projection has no fma and a fixed accumulation order"""
    import torch
    eng = ring_engine
    c = X.load_ckpt(500)
    eng.target_network.load_flat(c["target_params"])
    eng.sample(c["batch_inds"].astype(np.int64))
    eng.target()
    _Xb, _A, Xn, Rw, Tm = X.batch_of(ringv, c["batch_inds"])
    p = _np(eng.target_network.get_probs(torch.from_numpy(Xn)))
    q = _np(eng.target_network.get_q_values(torch.from_numpy(Xn)))
    a = (q[:, 1] > q[:, 0]).astype(np.int64)
    assert np.array_equal(a, _np(eng.next_actions)) and Tm.any()
    assert np.array_equal(X.project(p[np.arange(128), a], Rw, Tm)[0], _np(eng.target_probs))


def test_fused_update_is_bitwise_the_unfused_sequence(ringv):
    """mi_c51_update (in-kernel sampling, Adam on the slab sum) against sample() + grad() + deep_rl_amd.Adam.step over 4 updates with a target sync between them"""
    from deep_rl_amd import _native as N
    a, b = _make(), _make()
    for eng in (a, b):
        _load_ring(eng, ringv, global_step=15_000)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        assert np.array_equal(_np(a.batch_inds), _np(b.batch_inds)) and _np(a.batch_inds).max() < 15_000
        for x, y in ((a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
                     (a.target_probs, b.target_probs), (a.probs, b.probs)):
            assert np.array_equal(_np(x), _np(y))
        if u == 1:
            a.sync_target(); b.sync_target()
    assert a.optimizer.step_count == b.optimizer.step_count == 4 and a.update_index == 4
    assert not np.array_equal(_np(a.q.flat), _np(a.target_network.flat)) and np.isfinite(_np(a.q.flat)).all()
    # twice the same update from the same state: the same bits (no floating-point atomics)
    c = _make()
    _load_ring(c, ringv, global_step=15_000)
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat))
    assert N.lib().mi_version() == N.ABI_VERSION


def test_env_count_invariance():
    """env E of an N = 5 engine acts exactly as an N = 1 engine with env_id_base = E: 64 steps at epsilon ~ 0.5, exploring and greedy steps both present"""
    t = X.load_ckpt(1000)
    kw = dict(slots=70, params=t["params_before"], total_timesteps=20_000)
    big = _make(n=5, **kw)
    big.global_step = 5_260                      # epsilon = 1 - 0.95 * 5,260 / 10,000 = 0.5003 (c51.py:48,93)
    big.reset()
    big.act(64)
    A5, O5, T5 = _np(big.actions), _np(big.observations), _np(big.terminated)
    greedy_rows = 0
    for E in range(5):
        one = _make(n=1, env_id_base=E, **kw)
        one.global_step = 5_260
        one.reset()
        one.act(64)
        assert np.array_equal(_np(one.actions)[:, 0], A5[:, E]) and np.array_equal(_np(one.observations)[:, 0], O5[:, E]) and np.array_equal(_np(one.terminated)[:, 0], T5[:, E])
        assert np.array_equal(_np(one.observation)[0], _np(big.observation)[E])
        # the greedy steps: where the action is not the keyed random one it must be the argmax of the forward API's action values
        slots = (5_260 + np.arange(64)) % 70
        q = _np(one.q.get_q_values(one.observations[slots, 0]))
        greedy_rows += int(((q[:, 1] > q[:, 0]) == (A5[slots, E] == 1)).sum())
    assert len(set(A5[(5_260 + np.arange(64)) % 70].ravel().tolist())) == 2
    assert greedy_rows > 5 * 64 * 0.6            # about half the steps are greedy and agree; of the exploring half about half agree by chance
    # exploring and greedy steps are both present, by the contract's own split (mi_c51.h: stream 3, idx = the env step counter, which starts at 0 here): an exploring
    # step takes the keyed random action, a greedy one exactly the argmax of the forward API's action values on the ring's observation of that step
    n_explore = n_greedy = 0
    for E in range(5):
        u, ra = X.explore_draws(1, E, np.arange(64))
        explore = u < np.maximum(-0.95 / 10_000 * (5_260 + np.arange(64)) + 1.0, 0.05)
        slots = (5_260 + np.arange(64)) % 70
        q = _np(big.q.get_q_values(big.observations[slots, E]))
        assert np.array_equal(A5[slots, E], np.where(explore, ra, (q[:, 1] > q[:, 0]).astype(np.int64)))
        n_explore += int(explore.sum()); n_greedy += int((~explore).sum())
    assert n_explore >= 5 * 64 * 0.3 and n_greedy >= 5 * 64 * 0.3


def test_checkpoint_resume_is_bit_exact(tmp_path, ringv):
    from deep_rl_amd import checkpoint
    a = _make(slots=20_001)
    _load_ring(a, ringv, global_step=15_000)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "c51"), a)
    b = _make(slots=20_001)
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
        D.C51QNetwork(env, n_atoms=51)
    with pytest.raises(N.MiError):
        D.C51QNetwork(D.make("Pendulum-v1", num_envs=1, device=dev, seed=1))
    eng = _make()
    eng.reset()
    with pytest.raises(N.MiError):
        eng.train_step()                         # empty ring
    with pytest.raises(N.MiError):
        eng.act(65)
