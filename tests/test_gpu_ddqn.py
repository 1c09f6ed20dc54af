"""Double DQN on the MI355X (libmirl_ddqn.so, include/mi_ddqn.h through DoubleDQNEngine): the acting launch against the unchanged C oracle's DQN acting, the
forward API, 51 chained updates and the fused call against the float64 torch restatement (tests/_ddqn_ref.py), checkpoint / resume, loud errors.

The reference has no double_dqn.py.  Acting is DQN's, so the oracle's dqn_act_steps / dqn_forward / dqn_epsilon / dqn_explore_draw are its yardstick, bit for bit on
everything but the greedy choice, which is compared wherever the oracle's two action values differ by more than 1e-4 (the margin of tests/test_gpu_dqn.py).  The
update's bounds are _ddqn_ref.BOUND / BOUND_CHAIN: max(8 x what float32 torch measures against float64, the bar the suite holds DQN to).  Observed maxima go to
ddqn_gpu_maxima.json in the tests' results directory."""
import numpy as np
import pytest
import torch

import _ddqn_ref as X
import _dqn_cases as D
from test_gpu_ddqn_cases import _np, make_engine, record

pytestmark = pytest.mark.gpu


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


@pytest.fixture(autouse=True)
def _fdlibm(R):
    R.set_sincos_mode("fdlibm")
    yield
    R.set_sincos_mode("libm")


@pytest.fixture(scope="module")
def chain(R):
    """the ring and batches of the chained-update tests and the float64 chain, computed once on the CPU"""
    ring, indices, params, target = X.chain_data(R)
    losses, final = X.chain(ring, indices, params, target)
    return dict(ring=ring, indices=indices, params=params, target=target, losses=losses, final=final)


def _load_ring(eng, ring, global_step):
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(ring[name]))
    eng.global_step = global_step


def _chain_engine(dev, chain, **kw):
    eng = make_engine(dev, 1, X.CHAIN_STEPS + 1, params=chain["params"], target=chain["target"], seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, **kw)
    _load_ring(eng, chain["ring"], X.CHAIN_STEPS)
    return eng


@pytest.mark.parametrize("n", [3, 37, 4096])
def test_act_steps_keyed_rng_ring_wrap(dev, R, n):
    """3 / 37 / 4,096 envs (one env per workgroup up to 1,024, four beyond), a 16-slot ring (wraps many times), learning_starts = 45 inside a call, epsilon
    decaying to 0.05 within the test: the device's actions replayed on the oracle give all four ring tensors and `observation` bit for bit; at the first step of
    each call the decision follows the contract (the keyed random action before learning_starts and on exploring steps, the argmax on greedy ones)."""
    S, tt, ls, k = 16, 400, 45, 10
    g0, calls = (40, 2) if n == 4096 else (0, 40)          # the large shape runs steps 40 .. 59: its first call straddles learning_starts too
    eng = make_engine(dev, n, S, seed=5, base=300, learning_starts=ls, total_timesteps=tt, max_episodes_logged=0)
    rng = np.random.default_rng(1)
    params = (_np(eng.q.flat) + rng.normal(0, 0.05, X.NP)).astype(np.float32)
    eng.q.load_flat(params)
    env = R.VecCartPole(n, seed=5, env_id_base=300); st = R.ReplayStorage(S, n)
    obs_cur = env.reset(); st.observations[g0 % S] = obs_cur
    eng.global_step = g0
    assert np.array_equal(_np(eng.reset()), obs_cur)
    gs, n_greedy, n_random, n_checked = g0, 0, 0, 0
    for call in range(calls):
        obs_before = _np(eng.observation).copy()
        eng.act(k)
        fa = np.stack([_np(eng.actions[(gs + s) % S]) for s in range(k)])   # the device's actions of this call (k <= S), replayed on the oracle
        R.dqn_act_steps(env, params, st, obs_cur, k, gs, learning_starts=ls, total_timesteps=tt, forced_actions=fa)
        for name in ("observations", "actions", "rewards", "terminated"):
            assert np.array_equal(_np(getattr(eng, name)), getattr(st, name)), (call, name)
        assert np.array_equal(_np(eng.observation), obs_cur)
        eps = np.float32(R.dqn_epsilon(gs, total_timesteps=tt))
        qv = R.dqn_forward(params, obs_before)
        for e in range(0, n, 7 if n > 7 else 1):
            u, ra = R.dqn_explore_draw(5, 300 + e, gs - g0)                 # (the env step counters start at 0 whatever global_step is)
            if gs < ls or u < eps:
                assert fa[0, e] == ra; n_random += 1
            elif abs(qv[e, 0] - qv[e, 1]) > 1e-4:
                assert fa[0, e] == int(qv[e, 1] > qv[e, 0]); n_greedy += 1
            n_checked += 1
        gs += k
    assert eng.global_step == gs
    assert n_greedy > (10 if n == 3 else 50) and n_random > (10 if n == 3 else 50) and n_checked >= (120 if n == 3 else 240)


def test_an_env_acts_as_its_single_env_engine(dev):
    """shard invariance: env E of an N = 5 engine acts exactly as an N = 1 engine with env_id_base = E (64 steps across learning_starts)"""
    rng = np.random.default_rng(3)
    params = D.init_params(rng)[0]
    kw = dict(params=params, seed=9, learning_starts=45, total_timesteps=400, max_episodes_logged=0)
    big = make_engine(dev, 5, 70, **kw)
    big.global_step = 20
    big.reset()
    big.act(64)
    A5, O5, T5 = _np(big.actions), _np(big.observations), _np(big.terminated)
    assert set(np.unique(A5[20:70]).tolist()) == {0, 1}
    for E in range(5):
        one = make_engine(dev, 1, 70, base=E, **kw)
        one.global_step = 20
        one.reset()
        one.act(64)
        assert np.array_equal(_np(one.actions)[:, 0], A5[:, E]) and np.array_equal(_np(one.observations)[:, 0], O5[:, E]) and np.array_equal(_np(one.terminated)[:, 0], T5[:, E])
        assert np.array_equal(_np(one.observation)[0], _np(big.observation)[E])


@pytest.mark.parametrize("rows", [1, 5, 300])
def test_forward_against_float64(dev, rows):
    rng = np.random.default_rng(rows)
    params = D.init_params(rng)[0]
    obs = D._draw_obs(rng, rows)
    eng = make_engine(dev, 1, 2, params=params)
    q = _np(eng.forward(torch.from_numpy(obs)))
    q64 = X.forward(params, obs)
    err = float(np.abs(q - q64).max())
    record("forward_%d" % rows, {"q": err, "bound": X.BOUND["plain"]["q"], "max_abs_q": float(np.abs(q64).max())})
    assert q.shape == (rows, 2) and q.dtype == np.float32 and err <= X.BOUND["plain"]["q"]
    lead = _np(eng.forward(torch.from_numpy(obs).reshape(1, rows, 4)))
    assert lead.shape == (1, rows, 2) and np.array_equal(lead[0], q)


def test_51_updates_chained_with_a_target_sync(dev, chain):
    """the ring is built ON THE CPU (oracle acting, keyed RNG, fixed parameters), so a device and a CPU-only run see identical data; the indices are the oracle's
    dqn_sample; every loss and the parameters behind update 50 against the float64 torch chain"""
    eng = _chain_engine(dev, chain)
    worst = 0.0
    for k in range(X.CHAIN_UPDATES):
        eng.train_step(chain["indices"][k])
        worst = max(worst, abs(float(eng.loss.item()) - chain["losses"][k]) / abs(chain["losses"][k]))
        if k == 25:
            eng.sync_target()
    dp = float(np.abs(_np(eng.q.flat) - chain["final"]).max())
    record("chain_51", {"loss": worst, "loss_bound": X.BOUND_CHAIN["loss"], "params": dp, "params_bound": X.BOUND_CHAIN["params"]})
    assert eng.optimizer.step_count == X.CHAIN_UPDATES == 51 and eng.update_index == 51
    assert not np.array_equal(_np(eng.target_network.flat), _np(eng.q.flat)) and not np.array_equal(_np(eng.target_network.flat), chain["target"])
    assert worst <= X.BOUND_CHAIN["loss"] and dp <= X.BOUND_CHAIN["params"]


def test_fused_update_is_bitwise_the_unfused_sequence_and_repeatable(dev, chain, R):
    """mi_ddqn_update (in-launch index draw, Adam on the slab sum) against sample() (libmirl's mi_dqn_sample) + grad() + deep_rl_amd.Adam.step over 4 updates with a
    target sync between them; the same four updates once more give the same bits"""
    a, b = _chain_engine(dev, chain), _chain_engine(dev, chain)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        assert np.array_equal(_np(a.batch_inds), _np(b.batch_inds)) and _np(a.batch_inds).max() < X.CHAIN_STEPS   # the in-launch draw is mi_dqn_sample's
        assert np.array_equal(_np(a.batch_inds), R.dqn_sample(X.CHAIN_SEED, u, X.CHAIN_STEPS, X.CHAIN_BATCH))
        for x, y in ((a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
                     (a.target_values, b.target_values), (a.current, b.current), (a.next_actions, b.next_actions)):
            assert np.array_equal(_np(x), _np(y))
        if u == 1:
            a.sync_target(); b.sync_target()
    assert a.optimizer.step_count == b.optimizer.step_count == 4 and a.update_index == 4
    assert not np.array_equal(_np(a.q.flat), _np(a.target_network.flat)) and np.isfinite(_np(a.q.flat)).all()
    c = _chain_engine(dev, chain)
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat)) and np.array_equal(_np(c.grads), _np(a.grads)) and np.array_equal(_np(c.loss), _np(a.loss))


def test_checkpoint_resume_is_bit_exact(dev, chain, tmp_path):
    from deep_rl_amd import checkpoint
    kw = dict(learning_starts=100, total_timesteps=2000)
    a = _chain_engine(dev, chain, **kw)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "ddqn"), a)
    b = make_engine(dev, 1, X.CHAIN_STEPS + 1, seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, **kw)
    b.reset()
    checkpoint.load(path, b)
    assert b.global_step == a.global_step == X.CHAIN_STEPS + 30 and b.update_index == 3 and b.optimizer.step_count == 3
    for u in range(3):
        for eng in (a, b):
            eng.act(10); eng.train_step()
            if u == 1:
                eng.sync_target()
    for x, y in ((a.q.flat, b.q.flat), (a.target_network.flat, b.target_network.flat), (a.observations, b.observations), (a.actions, b.actions), (a.terminated, b.terminated),
                 (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.observation, b.observation)):
        assert np.array_equal(_np(x), _np(y))
    assert not np.array_equal(_np(a.q.flat), chain["params"])


def test_errors_are_loud(dev, monkeypatch):
    import deep_rl_amd as A
    from deep_rl_amd import _native as N
    from deep_rl_amd import dist
    env = A.make("CartPole-v1", num_envs=1, device=dev, seed=1)
    q, wrong = A.QNetwork(env), A.DuelingQNetwork(env)
    with pytest.raises(N.MiError):
        A.DoubleDQNEngine(env, wrong, wrong, A.Adam(wrong, lr=X.LR), slots=16)        # a network of another size
    with pytest.raises(N.MiError):
        A.DoubleDQNEngine(env, q, A.QNetwork(env), A.Adam(q, lr=X.LR), slots=1)       # slots < 2
    with monkeypatch.context() as mp:
        mp.setattr(dist, "world_size", lambda group=None: 2)
        with pytest.raises(N.MiError, match="single process"):
            A.DoubleDQNEngine(env, q, A.QNetwork(env), A.Adam(q, lr=X.LR), slots=16)  # world size > 1
    eng = make_engine(dev, 1, 16)
    eng.reset()
    with pytest.raises(N.MiError):
        eng.train_step()                         # empty ring
    with pytest.raises(N.MiError):
        eng.sample()                             # empty ring
    with pytest.raises(N.MiError):
        eng.sample(np.arange(5))                 # a wrong index count
    with pytest.raises(N.MiError):
        eng.train_step(np.arange(5))
    with pytest.raises(N.MiError):
        eng.act(65)
