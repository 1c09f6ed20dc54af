"""Noisy-net n-step prioritized dueling Double DQN on the MI355X (libmirl_noisy.so, include/mi_noisy.h through NoisyDQNEngine): with noisy=False the engine IS
NStepDQNEngine bit for bit through acting and training; LIVE noisy acting, where every stored action is the float64 argmax under the device's own sample for that
(env, step) on a trajectory the CPU predicted; two envs at one observation and step draw different heads; 51 chained prioritized updates against the float64
restatement (tests/_noisy_ref.py) fed the device's samples; the fused train_step against the unfused sequence; checkpoint / resume; loud errors.

The bounds are _noisy_ref.BOUND / BOUND_CHAIN: max(8 x what the float32 evaluation measures against float64, the bar the suite holds DQN to).  Observed maxima go
to noisy_gpu_maxima.json in the tests' results directory."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dqn_cases as D
import _noisy_ref as Z
from test_gpu_noisy_cases import _np, device_sample, make_engine, record

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    cpu_ref.lib().ref_set_num_threads(8)
    return cpu_ref


@pytest.fixture(scope="module")
def chain(R):
    """the ring of the chained-update tests, computed once on the CPU"""
    R.set_sincos_mode("fdlibm")
    try:
        ring, indices, weights, params, target, _ = Z.chain_data(R)
    finally:
        R.set_sincos_mode("libm")
    return dict(ring=ring, params=params, target=target)


def _chain_engine(dev, chain, prioritized=True, **kw):
    """every transition of the CPU-built ring stored; prioritized: each at the initial max_priority, as acting would have left them"""
    kw.setdefault("n_step", Z.CHAIN_N)
    eng = make_engine(dev, 1, Z.CHAIN_STEPS + 1, params=chain["params"], target=chain["target"], seed=Z.CHAIN_SEED, batch_size=Z.CHAIN_BATCH, prioritized=prioritized, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(chain["ring"][name]))
    eng.global_step = Z.CHAIN_STEPS
    if prioritized:
        eng.priorities[:Z.CHAIN_STEPS] = 1e-2
        eng.refresh_sums()
    return eng


@pytest.mark.parametrize("prioritized", [True, False], ids=["prioritized", "uniform"])
def test_engine_with_noisy_off_is_the_nstep_engine_bit_for_bit(dev, prioritized):
    """the same seed and the same first 11,019 floats through 200 acting steps of 3 envs on a 64-slot ring (it wraps three times, learning_starts and the epsilon
    schedule inside) and 20 train_steps with a target sync; the sigmas, whose gradient is exact zeros, never move"""
    import deep_rl_amd as A
    import test_gpu_nstep_cases as TN

    kw = dict(seed=11, batch_size=64, learning_starts=45, total_timesteps=400, max_episodes_logged=0, prioritized=prioritized, n_step=3, start_e=1.0, end_e=0.05)
    b = TN.make_engine(dev, 3, 64, **kw)
    ext = lambda t, s: np.concatenate([_np(t), Z.default_sigma(s)])   # noqa: E731
    a = make_engine(dev, 3, 64, params=ext(b.q.flat, 1.0), target=ext(b.target_network.flat, 3.0), noisy=False, **kw)
    assert type(a) is A.NoisyDQNEngine and type(b) is A.NStepDQNEngine and a.K is not b.K and not a.noisy
    sig0 = _np(a.q.flat)[Z.SIGMA:].copy()
    a.reset(); b.reset()
    for u in range(20):
        for eng in (a, b):
            eng.act(10); eng.train_step()
            if u == 9:
                eng.sync_target()
        assert not _np(a.grads)[Z.SIGMA:].any()
    assert a.global_step == b.global_step == 200 and a.optimizer.step_count == b.optimizer.step_count == 20
    head = lambda t: t[:Z.NP_MEAN]   # noqa: E731
    pairs = [(head(a.q.flat), b.q.flat), (head(a.target_network.flat), b.target_network.flat), (head(a.optimizer.exp_avg), b.optimizer.exp_avg),
             (head(a.optimizer.exp_avg_sq), b.optimizer.exp_avg_sq), (a.observations, b.observations), (a.actions, b.actions), (a.rewards, b.rewards),
             (a.terminated, b.terminated), (a.observation, b.observation), (a.batch_inds, b.batch_inds), (a.loss, b.loss), (head(a.grads), b.grads),
             (a.target_values, b.target_values), (a.current, b.current), (a.td_abs, b.td_abs), (a.next_actions, b.next_actions), (a.horizon, b.horizon),
             (a.episode_stats, b.episode_stats)]
    if prioritized:
        pairs += [(a.priorities, b.priorities), (a.max_priority, b.max_priority), (a.weights, b.weights)]
    for k, (x, y) in enumerate(pairs):
        assert np.array_equal(_np(x), _np(y)), k
    assert np.array_equal(_np(a.q.flat)[Z.SIGMA:], sig0) and np.array_equal(_np(a.target_network.flat)[Z.SIGMA:], sig0)       # (the sync copied the online sigmas)
    assert not np.array_equal(_np(a.q.flat), _np(a.target_network.flat)) and np.isfinite(_np(a.q.flat)).all()
    obs = torch.from_numpy(_np(a.observations).reshape(-1, 4))
    assert np.array_equal(_np(a.forward(obs)), _np(b.forward(obs)))


LIVE_N, LIVE_S, LIVE_STEPS, LIVE_BASE = 3, 16, 40, 5


def _live_params(seed):
    rng = np.random.default_rng([seed, 2018, 13])
    return np.concatenate([D.init_params(rng)[1].astype(f32), Z.default_sigma(2.0) * rng.uniform(0.5, 1.5, Z.NHEAD).astype(f32)])


def _predict(R, seed):
    """the trajectory on the CPU: the oracle's envs (device-matched sin / cos), every action the float64 argmax under the float32 restatement's sample for
    (env id, step) -> (observations [steps][N][4] the actions were taken from, actions [steps][N], the smallest |q0 - q1|)"""
    params = _live_params(seed)
    R.set_sincos_mode("fdlibm")
    try:
        env = R.VecCartPole(LIVE_N, seed=seed, env_id_base=LIVE_BASE)
        obs = env.reset()
        seen, acts, gap = [], [], np.inf
        for g in range(LIVE_STEPS):
            q = np.stack([Z.forward(params, obs[n], Z.xi(seed, LIVE_BASE + n, g, Z.STREAM_ACT))[0] for n in range(LIVE_N)])
            gap = min(gap, float(np.abs(q[:, 0] - q[:, 1]).min()))
            a = (q[:, 1] > q[:, 0]).astype(np.int64)
            seen.append(obs.copy()); acts.append(a)
            obs = env.step(a)[0]
    finally:
        R.set_sincos_mode("libm")
    return np.stack(seen), np.stack(acts), gap


@pytest.fixture(scope="module")
def live(R):
    """the first seed from 1 whose predicted trajectory keeps |q0 - q1| >= CLOSE_Q at all 120 steps and takes both actions: chosen on the CPU, none left out"""
    for seed in range(1, 40):
        seen, acts, gap = _predict(R, seed)
        if gap >= Z.CLOSE_Q["default"] and 0 < acts.sum() < acts.size:
            return dict(seed=seed, seen=seen, acts=acts, gap=gap)
    raise RuntimeError("no seed")


def test_live_noisy_acting_takes_the_float64_argmax_under_the_device_sample_at_every_step(dev, live):
    """3 envs x 16 slots, 40 steps in chunks of 8 (the ring wraps twice), epsilon 0: every one of the 120 stored actions"""
    seed = live["seed"]
    params = _live_params(seed)
    eng = make_engine(dev, LIVE_N, LIVE_S, params=params, target=params, seed=seed, base=LIVE_BASE, batch_size=8, learning_starts=0, max_episodes_logged=0, prioritized=False)
    assert eng.noisy and eng.start_e == eng.end_e == 0.0
    eng.reset()
    checked, worst = 0, np.inf
    for g0 in range(0, LIVE_STEPS, 8):
        eng.act(8)
        obs, act = _np(eng.observations), _np(eng.actions)
        for g in range(g0, g0 + 8):
            for n in range(LIVE_N):
                x, a = obs[g % LIVE_S, n], int(act[g % LIVE_S, n])
                assert np.array_equal(x, live["seen"][g, n]), "the observation of step %d, env %d is not the predicted one" % (g, n)
                xi, _ = device_sample(dev, seed, LIVE_BASE + n, g, Z.STREAM_ACT)
                q = Z.forward(params, x, xi)[0]
                worst = min(worst, abs(q[0] - q[1]))
                assert abs(q[0] - q[1]) >= Z.CLOSE_Q["default"] and a == int(q[1] > q[0]) == int(live["acts"][g, n]), (g, n, q, a)
                checked += 1
    assert checked == 120 and eng.global_step == 40
    record("live_acting", dict(steps=checked, smallest_gap=float(worst), close_q=Z.CLOSE_Q["default"], seed=seed))
    # the mean network would have acted otherwise somewhere: the noise is what chose
    mean = np.stack([[int(np.argmax(Z.forward(params, live["seen"][g, n])[0])) for n in range(LIVE_N)] for g in range(LIVE_STEPS)])
    assert (mean != live["acts"]).any()
    # forward under an acting key is what the acting launch evaluated
    x = torch.from_numpy(live["seen"][7])
    q = _np(eng.forward(x[1], noise=(LIVE_BASE + 1, 7, Z.STREAM_ACT))).astype(np.float64)
    assert np.abs(q - Z.forward(params, live["seen"][7, 1], device_sample(dev, seed, LIVE_BASE + 1, 7, Z.STREAM_ACT)[0])[0]).max() <= Z.BOUND["default"]["q"]


def test_two_envs_at_the_same_observation_and_step_draw_different_heads(dev):
    state = np.tile(np.array([[0.01, -0.02, 0.03, 0.01]]), (2, 1))
    params = _live_params(2)
    eng = make_engine(dev, 2, 8, params=params, target=params, seed=9, batch_size=4, learning_starts=0, max_episodes_logged=0, prioritized=False)
    eng.reset(torch.from_numpy(state))
    x = _np(eng.observations)[0]
    assert np.array_equal(x[0], x[1])
    eng.act(1)
    s0, s1 = device_sample(dev, 9, 0, 0, Z.STREAM_ACT)[0], device_sample(dev, 9, 1, 0, Z.STREAM_ACT)[0]
    assert not np.array_equal(s0, s1) and abs(np.corrcoef(s0, s1)[0, 1]) < 0.3
    q0, q1 = _np(eng.forward(torch.from_numpy(x[0]), noise=(0, 0, 13))), _np(eng.forward(torch.from_numpy(x[1]), noise=(1, 0, 13)))
    assert np.abs(q0 - q1).max() > 100 * Z.BOUND["default"]["q"]
    for n, s in ((0, s0), (1, s1)):
        q = Z.forward(params, x[n], s)[0]
        assert abs(q[0] - q[1]) < Z.CLOSE_Q["default"] or int(_np(eng.actions)[0, n]) == int(q[1] > q[0])


def test_51_prioritized_noisy_updates_chained_with_a_target_sync(dev, chain):
    """the device draws every batch from its own priorities and every pair of heads from its own counters; the float64 chain is fed the device's indices, weights
    and samples; every loss and all 11,274 parameters behind update 50 against it"""
    eng = _chain_engine(dev, chain)
    idx, w, losses, pairs = [], [], [], []
    for k in range(Z.CHAIN_UPDATES):
        pairs.append((device_sample(dev, Z.CHAIN_SEED, k, 0, Z.STREAM_LEARN)[0], device_sample(dev, Z.CHAIN_SEED, k, 1, Z.STREAM_LEARN)[0]))
        assert eng.update_index == k
        eng.train_step()
        idx.append(_np(eng.batch_inds).copy()); w.append(_np(eng.weights).copy()); losses.append(float(eng.loss.item()))
        if k == 25:
            eng.sync_target()
    idx, w = np.stack(idx), np.stack(w)
    assert idx.min() >= 0 and idx.max() < Z.CHAIN_STEPS and (w.max(axis=1) == 1).all() and (w > 0).all()
    l64, p64 = Z.chain(chain["ring"], idx, w, chain["params"], chain["target"], Z.CHAIN_N, Z.CHAIN_STEPS, pairs)
    worst = float((np.abs(np.array(losses) - l64) / np.abs(l64)).max())
    dp = float(np.abs(_np(eng.q.flat) - p64).max())
    record("chain_51", {"loss": worst, "loss_bound": Z.BOUND_CHAIN["loss"], "params": dp, "params_bound": Z.BOUND_CHAIN["params"]})
    assert eng.optimizer.step_count == Z.CHAIN_UPDATES == 51 and eng.update_index == 51
    assert np.abs(_np(eng.q.flat) - chain["params"])[Z.SIGMA:].max() > 20 * Z.LR                    # the sigmas learned
    assert worst <= Z.BOUND_CHAIN["loss"] and dp <= Z.BOUND_CHAIN["params"]


def test_prioritized_train_step_is_bitwise_the_unfused_sequence_and_repeatable(dev, chain):
    """sampler + mi_nz_update + scatter against sample() + grad() (mi_nz_grad + scatter) + deep_rl_amd.Adam.step over 4 updates with a target sync between them"""
    a, b = _chain_engine(dev, chain), _chain_engine(dev, chain)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        for x, y in ((a.batch_inds, b.batch_inds), (a.weights, b.weights), (a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg),
                     (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.target_values, b.target_values), (a.current, b.current), (a.next_actions, b.next_actions),
                     (a.td_abs, b.td_abs), (a.priorities, b.priorities), (a.max_priority, b.max_priority), (a.horizon, b.horizon)):
            assert np.array_equal(_np(x), _np(y)), u
        if u == 1:
            a.sync_target(); b.sync_target()
    c = _chain_engine(dev, chain)
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat)) and np.array_equal(_np(c.priorities), _np(a.priorities)) and np.array_equal(_np(c.loss), _np(a.loss))
    assert _np(a.grads)[Z.SIGMA:].any()


@pytest.mark.parametrize("prioritized", [True, False], ids=["prioritized", "uniform"])
def test_checkpoint_resume_is_bit_exact(dev, chain, tmp_path, prioritized):
    """nothing new is saved: the noise is keyed by counters the checkpoint already holds, so the resumed run draws the same heads when acting and when learning"""
    from deep_rl_amd import checkpoint
    kw = dict(learning_starts=0, total_timesteps=2000)
    a = _chain_engine(dev, chain, prioritized=prioritized, **kw)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "noisy"), a)
    b = make_engine(dev, 1, Z.CHAIN_STEPS + 1, seed=Z.CHAIN_SEED, batch_size=Z.CHAIN_BATCH, prioritized=prioritized, n_step=Z.CHAIN_N, **kw)
    b.reset()
    checkpoint.load(path, b)
    assert b.global_step == a.global_step == Z.CHAIN_STEPS + 30 and b.update_index == 3 and b.optimizer.step_count == 3
    pairs = lambda: [(a.q.flat, b.q.flat), (a.target_network.flat, b.target_network.flat), (a.observations, b.observations), (a.actions, b.actions),   # noqa: E731
                     (a.terminated, b.terminated), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.observation, b.observation)] + (
                         [(a.priorities, b.priorities), (a.max_priority, b.max_priority)] if prioritized else [])
    for x, y in pairs():
        assert np.array_equal(_np(x), _np(y))
    for u in range(3):
        for eng in (a, b):
            eng.act(10); eng.train_step()
            if u == 1:
                eng.sync_target()
    for x, y in pairs() + [(a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.td_abs, b.td_abs), (a.horizon, b.horizon), (a.grads, b.grads)] + ([(a.weights, b.weights)] if prioritized else []):
        assert np.array_equal(_np(x), _np(y))
    assert not np.array_equal(_np(a.q.flat), chain["params"]) and _np(a.q.flat).size == Z.NP


def test_errors_are_loud(dev):
    import deep_rl_amd as A
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_nz as K
    env = A.make("CartPole-v1", num_envs=1, device=dev, seed=1)
    q = A.NoisyDuelingQNetwork(env)
    for bad, slots in ((0, 64), (17, 64), (8, 8)):
        with pytest.raises(N.MiError, match="n_step"):
            A.NoisyDQNEngine(env, q, A.NoisyDuelingQNetwork(env), A.Adam(q, lr=Z.LR), slots=slots, n_step=bad)
    plain = A.DuelingQNetwork(env)
    with pytest.raises(N.MiError, match="NoisyDuelingQNetworks"):
        A.NoisyDQNEngine(env, plain, plain, A.Adam(plain, lr=Z.LR), slots=16)                  # the 11,019-float network of the older engines
    with pytest.raises(N.MiError):
        q.forward(torch.zeros(1, 4))                                                           # the module's forward is for CPU parameters
    for prioritized in (True, False):
        eng = make_engine(dev, 1, 128, prioritized=prioritized)
        assert eng.n_step == 3 and eng.noisy
        eng.reset()
        with pytest.raises(N.MiError):
            eng.train_step()                         # empty ring
        assert eng.global_step == 0
        eng.act(8)
        with pytest.raises(N.MiError):
            eng.train_step(np.arange(5))             # a wrong index count
        with pytest.raises(N.MiError, match="stream"):
            eng.forward(torch.zeros(1, 4), noise=(0, 0, 16))
        assert eng.update_index == 0 and eng.optimizer.step_count == 0
    # straight at the C ABI: negative codes, the text names the call, nothing is launched
    eng = make_engine(dev, 1, 128)
    eng.reset(); eng.act(8); eng.sample()
    L = K.lib()
    a = K.AdamArgs(K.ptr(eng.optimizer.exp_avg), K.ptr(eng.optimizer.exp_avg_sq), 1, Z.LR, 0.9, 0.999, 1e-8)
    before = _np(eng.q.flat).copy()
    eng.horizon.fill_(-7)

    def all_three(b, text):
        assert L.mi_nz_target(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and text in L.mi_nz_last_error() and b"mi_nz_target" in L.mi_nz_last_error()
        assert L.mi_nz_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and text in L.mi_nz_last_error()
        assert L.mi_nz_update(C.byref(eng._ring), C.byref(b), C.byref(a), eng._s()) == -1 and text in L.mi_nz_last_error()

    for n in (0, 17, 128, -3):
        b = eng._batch(0); b.n_step = n
        all_three(b, b"n_step")
    for h in (-1, 128):
        b = eng._batch(0); b.head_slot = h
        all_three(b, b"head_slot")
    b = eng._batch(0); b.horizon = None
    all_three(b, b"horizon is NULL")
    b = eng._batch(0); b.td_abs = None
    assert L.mi_nz_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and b"a batch buffer is NULL" in L.mi_nz_last_error()
    a.step = 0
    assert L.mi_nz_update(C.byref(eng._ring), C.byref(eng._batch(0)), C.byref(a), eng._s()) == -1   # optimizer step < 1
    act = K.NZAct(K.ptr(eng.q.flat), K.ptr(eng.observation), None, None, None, K.ptr(eng.episode_stats), 8, 100, 0, 0.0, 0.0, 0.5, 65, 0, 1, 0)
    assert L.mi_nz_act_steps(eng.env.handle, C.byref(eng._ring), C.byref(act), eng._s()) == -1 and b"n_steps" in L.mi_nz_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_np(eng.q.flat), before) and (_np(eng.horizon) == -7).all() and eng.global_step == 8       # nothing was launched
