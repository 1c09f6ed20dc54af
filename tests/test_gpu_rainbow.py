"""Rainbow on the MI355X (libmirl_rainbow.so, include/mi_rainbow.h through RainbowEngine): LIVE noisy acting, where every stored action is the float64 argmax
under the device's own sample for that (env, step) on a trajectory the CPU predicted; 51 chained prioritized updates against the float64 restatement
(tests/_rainbow_ref.py) fed the device's indices, weights and samples; the fused train_step against the unfused sequence; checkpoint / resume; loud errors.

The bounds are _rainbow_ref.BOUND / BOUND_CHAIN: max(8 x what the float32 evaluation measures against float64, the bar the suite holds DQN to).  Observed maxima
go to rainbow_gpu_maxima.json in the tests' results directory."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dqn_cases as D
import _rainbow_ref as Z
from test_gpu_rainbow_cases import _np, device_eps, make_engine, record

pytestmark = pytest.mark.gpu
f32 = np.float32
SUPPORT = Z.CHAIN_SUPPORT


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
    eng = make_engine(dev, 1, Z.CHAIN_STEPS + 1, params=chain["params"], target=chain["target"], seed=Z.CHAIN_SEED, batch_size=Z.CHAIN_BATCH, prioritized=prioritized,
                      support=SUPPORT, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(chain["ring"][name]))
    eng.global_step = Z.CHAIN_STEPS
    if prioritized:
        eng.priorities[:Z.CHAIN_STEPS] = 1e-2
        eng.refresh_sums()
    return eng


LIVE_N, LIVE_S, LIVE_STEPS, LIVE_BASE = 3, 16, 40, 5


def _live_params(seed):
    rng = np.random.default_rng([seed, 2018, 22])
    return Z.vector(D.init_params(rng)[1], rng, sigma_scale=2.0, jitter=True)


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
            q = np.stack([Z.forward(params, obs[n], SUPPORT, Z.eps(seed, LIVE_BASE + n, g, Z.STREAM_ACT))[1][0] for n in range(LIVE_N)])
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
    for seed in range(1, 60):
        seen, acts, gap = _predict(R, seed)
        if gap >= Z.CLOSE_Q["default"] and 0 < acts.sum() < acts.size:
            return dict(seed=seed, seen=seen, acts=acts, gap=gap)
    raise RuntimeError("no seed")


def test_live_noisy_acting_takes_the_float64_argmax_under_the_device_sample_at_every_step(dev, live):
    """3 envs x 16 slots, 40 steps in chunks of 8 (the ring wraps twice), epsilon 0: every one of the 120 stored actions"""
    seed = live["seed"]
    params = _live_params(seed)
    eng = make_engine(dev, LIVE_N, LIVE_S, params=params, target=params, seed=seed, base=LIVE_BASE, batch_size=8, learning_starts=0, max_episodes_logged=0, prioritized=False,
                      support=SUPPORT)
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
                q = Z.forward(params, x, SUPPORT, device_eps(dev, seed, LIVE_BASE + n, g, Z.STREAM_ACT))[1][0]
                worst = min(worst, abs(q[0] - q[1]))
                assert abs(q[0] - q[1]) >= Z.CLOSE_Q["default"] and a == int(q[1] > q[0]) == int(live["acts"][g, n]), (g, n, q, a)
                checked += 1
    assert checked == 120 and eng.global_step == 40
    record("live_acting", dict(steps=checked, smallest_gap=float(worst), close_q=Z.CLOSE_Q["default"], seed=seed))
    # the mean network would have acted otherwise somewhere: the noise is what chose
    mean = np.stack([[int(np.argmax(Z.forward(params, live["seen"][g, n], SUPPORT)[1][0])) for n in range(LIVE_N)] for g in range(LIVE_STEPS)])
    assert (mean != live["acts"]).any()
    # forward under an acting key is what the acting launch evaluated
    x = torch.from_numpy(live["seen"][7])
    p, q = eng.forward(x[1], noise=(LIVE_BASE + 1, 7, Z.STREAM_ACT), probs=True)
    rp, rq = Z.forward(params, live["seen"][7, 1], SUPPORT, device_eps(dev, seed, LIVE_BASE + 1, 7, Z.STREAM_ACT))
    assert np.abs(_np(q).astype(np.float64) - rq[0]).max() <= Z.BOUND["default"]["q"] and np.abs(_np(p).astype(np.float64) - rp[0]).max() <= Z.BOUND["default"]["probs"]
    # and with noisy = 0 the mean network acts: the same start, the mean network's first actions
    off = make_engine(dev, LIVE_N, LIVE_S, params=params, target=params, seed=seed, base=LIVE_BASE, batch_size=8, learning_starts=0, max_episodes_logged=0, prioritized=False,
                      support=SUPPORT, noisy=False)
    off.reset()
    off.act(1)
    q0 = Z.forward(params, live["seen"][0], SUPPORT)[1]
    sure = np.abs(q0[:, 0] - q0[:, 1]) >= Z.CLOSE_Q["default"]
    assert np.array_equal(_np(off.actions)[0][sure], (q0[:, 1] > q0[:, 0]).astype(np.int64)[sure])


def test_51_prioritized_updates_chained_with_a_target_sync(dev, chain):
    """the device draws every batch from its own priorities — its own row losses — and every pair of heads from its own counters; the float64 chain is fed the
    device's indices, weights and samples; every loss and all 36,774 parameters behind update 50 against it"""
    eng = _chain_engine(dev, chain)
    idx, w, losses, pairs = [], [], [], []
    for k in range(Z.CHAIN_UPDATES):
        pairs.append((device_eps(dev, Z.CHAIN_SEED, k, 0, Z.STREAM_LEARN), device_eps(dev, Z.CHAIN_SEED, k, 1, Z.STREAM_LEARN)))
        assert eng.update_index == k
        eng.train_step()
        idx.append(_np(eng.batch_inds).copy()); w.append(_np(eng.weights).copy()); losses.append(float(eng.loss.item()))
        uniq, cnt = np.unique(idx[-1], return_counts=True)
        once = np.isin(idx[-1], uniq[cnt == 1])
        assert once.any() and np.array_equal(_np(eng.priorities).reshape(-1)[idx[-1]][once], _np(eng.prio)[once])      # the row loss IS the new priority
        if k == 25:
            eng.sync_target()
    idx, w = np.stack(idx), np.stack(w)
    assert idx.min() >= 0 and idx.max() < Z.CHAIN_STEPS and (w.max(axis=1) == 1).all() and (w > 0).all()
    l64, p64 = Z.chain(chain["ring"], idx, w, chain["params"], chain["target"], Z.CHAIN_N, Z.CHAIN_STEPS, SUPPORT, pairs)
    worst = float((np.abs(np.array(losses) - l64) / np.abs(l64)).max())
    dp = float(np.abs(_np(eng.q.flat) - p64).max())
    print("chain: loss %.3g (bound %.3g), params %.3g (bound %.3g)" % (worst, Z.BOUND_CHAIN["loss"], dp, Z.BOUND_CHAIN["params"]))
    record("chain_51", {"loss": worst, "loss_bound": Z.BOUND_CHAIN["loss"], "params": dp, "params_bound": Z.BOUND_CHAIN["params"]})
    assert eng.optimizer.step_count == Z.CHAIN_UPDATES == 51 and eng.update_index == 51
    assert np.abs(_np(eng.q.flat) - chain["params"])[Z.SIGMA:].max() > 20 * Z.LR                    # the sigmas learned
    assert worst <= Z.BOUND_CHAIN["loss"] and dp <= Z.BOUND_CHAIN["params"]


def test_prioritized_train_step_is_bitwise_the_unfused_sequence_and_repeatable(dev, chain):
    """sampler + mi_rb_update + scatter against sample() + grad() (mi_rb_grad + scatter) + deep_rl_amd.Adam.step over 4 updates with a target sync between them"""
    a, b = _chain_engine(dev, chain), _chain_engine(dev, chain)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        for x, y in ((a.batch_inds, b.batch_inds), (a.weights, b.weights), (a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg),
                     (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.target_probs, b.target_probs), (a.probs, b.probs), (a.next_actions, b.next_actions),
                     (a.prio, b.prio), (a.priorities, b.priorities), (a.max_priority, b.max_priority), (a.horizon, b.horizon)):
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
    path = checkpoint.save(str(tmp_path / "rainbow"), a)
    b = make_engine(dev, 1, Z.CHAIN_STEPS + 1, seed=Z.CHAIN_SEED, batch_size=Z.CHAIN_BATCH, prioritized=prioritized, n_step=Z.CHAIN_N, support=SUPPORT, **kw)
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
    for x, y in pairs() + [(a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.prio, b.prio), (a.horizon, b.horizon), (a.grads, b.grads), (a.target_probs, b.target_probs)] + (
            [(a.weights, b.weights)] if prioritized else []):
        assert np.array_equal(_np(x), _np(y))
    assert not np.array_equal(_np(a.q.flat), chain["params"]) and _np(a.q.flat).size == Z.NP


def test_errors_are_loud(dev):
    import deep_rl_amd as A
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_rb as K
    env = A.make("CartPole-v1", num_envs=1, device=dev, seed=1)
    q = A.RainbowQNetwork(env)
    for bad, slots in ((0, 64), (17, 64), (8, 8)):
        with pytest.raises(N.MiError, match="n_step"):
            A.RainbowEngine(env, q, A.RainbowQNetwork(env), A.Adam(q, lr=Z.LR), slots=slots, n_step=bad)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(N.MiError, match="support"):
            A.RainbowEngine(env, q, A.RainbowQNetwork(env), A.Adam(q, lr=Z.LR), slots=16, v_min=lo, v_max=hi)
    with pytest.raises(N.MiError, match="n_atoms"):
        A.RainbowEngine(env, q, A.RainbowQNetwork(env), A.Adam(q, lr=Z.LR), slots=16, n_atoms=101)
    noisy = A.NoisyDuelingQNetwork(env)
    with pytest.raises(N.MiError, match="RainbowQNetworks"):
        A.RainbowEngine(env, noisy, noisy, A.Adam(noisy, lr=Z.LR), slots=16)                   # the 11,274-float network of the noisy engine
    with pytest.raises(N.MiError):
        q.forward(torch.zeros(1, 4))                                                           # the module's forward is for CPU parameters
    for prioritized in (True, False):
        eng = make_engine(dev, 1, 128, prioritized=prioritized)
        assert eng.n_step == 3 and eng.noisy and (eng.v_min, eng.v_max) == (0.0, 100.0)
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
        assert L.mi_rb_target(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and text in L.mi_rb_last_error() and b"mi_rb_target" in L.mi_rb_last_error()
        assert L.mi_rb_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and text in L.mi_rb_last_error()
        assert L.mi_rb_update(C.byref(eng._ring), C.byref(b), C.byref(a), eng._s()) == -1 and text in L.mi_rb_last_error()

    for n in (0, 17, 128, -3):
        b = eng._batch(0); b.n_step = n
        all_three(b, b"n_step")
    for h in (-1, 128):
        b = eng._batch(0); b.head_slot = h
        all_three(b, b"head_slot")
    b = eng._batch(0); b.horizon = None
    all_three(b, b"horizon is NULL")
    for lo, hi in ((3.0, 3.0), (4.0, 3.0), (0.0, float("inf")), (float("nan"), 3.0)):
        b = eng._batch(0); b.v_min, b.v_max = lo, hi
        all_three(b, b"support")
    b = eng._batch(0); b.prio = None
    assert L.mi_rb_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and b"a batch buffer is NULL" in L.mi_rb_last_error()
    a.step = 0
    assert L.mi_rb_update(C.byref(eng._ring), C.byref(eng._batch(0)), C.byref(a), eng._s()) == -1   # optimizer step < 1
    act = K.RBAct(K.ptr(eng.q.flat), K.ptr(eng.observation), None, None, None, K.ptr(eng.episode_stats), 8, 100, 0, 0.0, 0.0, 0.5, 65, 0, 1, 0.0, 100.0, 0)
    assert L.mi_rb_act_steps(eng.env.handle, C.byref(eng._ring), C.byref(act), eng._s()) == -1 and b"n_steps" in L.mi_rb_last_error()
    act.n_steps, act.v_max = 8, 0.0
    assert L.mi_rb_act_steps(eng.env.handle, C.byref(eng._ring), C.byref(act), eng._s()) == -1 and b"support" in L.mi_rb_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_np(eng.q.flat), before) and (_np(eng.horizon) == -7).all() and eng.global_step == 8       # nothing was launched
