"""Munchausen DQN on the MI355X (libmirl_mdqn.so, include/mi_mdqn.h through MunchausenDQNEngine): 51 chained updates and the fused call against the float64 torch
restatement (tests/_mdqn_ref.py), checkpoint / resume, acting that is DoubleDQNEngine's, loud errors.

The reference has no munchausen_dqn.py.  The ring and the indices of the chain are Double DQN's (_ddqn_ref.chain_data, built on the CPU by the C oracle's DQN
acting); the update's bounds are _mdqn_ref.BOUND_CHAIN: max(8 x what float32 torch measures against float64, the bar the suite holds DQN to).  Observed maxima go to
mdqn_gpu_maxima.json in the tests' results directory."""
import numpy as np
import pytest
import torch

import _mdqn_ref as X
from test_gpu_mdqn_cases import _np, make_engine, record

pytestmark = pytest.mark.gpu
CHAIN_SEED = 7


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
    """the ring and batches of the chained-update tests and the float64 chain, computed once on the CPU"""
    import _ddqn_ref as DD
    assert DD.CHAIN_SEED == CHAIN_SEED
    ring, indices, params, target = X.chain_data(R)
    losses, final = X.chain(ring, indices, params, target)
    return dict(ring=ring, indices=indices, params=params, target=target, losses=losses, final=final)


def _chain_engine(dev, chain, **kw):
    eng = make_engine(dev, 1, X.CHAIN_STEPS + 1, params=chain["params"], target=chain["target"], seed=CHAIN_SEED, batch_size=X.CHAIN_BATCH, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(chain["ring"][name]))
    eng.global_step = X.CHAIN_STEPS
    return eng


def test_51_updates_chained_with_a_target_sync(dev, chain):
    """the ring is built ON THE CPU (oracle acting, keyed RNG, fixed parameters); the indices are the oracle's dqn_sample; every loss and the parameters behind update
    50 against the float64 torch chain at the default alpha, tau and clip_lo"""
    eng = _chain_engine(dev, chain)
    assert (eng.alpha, eng.tau, eng.clip_lo) == (X.HP["alpha"], X.HP["tau"], X.HP["clip_lo"]) == (0.9, 0.03, -1.0)
    worst = 0.0
    for k in range(X.CHAIN_UPDATES):
        eng.train_step(chain["indices"][k])
        worst = max(worst, abs(float(eng.loss.item()) - chain["losses"][k]) / abs(chain["losses"][k]))
        if k == 25:
            eng.sync_target()
    dp = float(np.abs(_np(eng.q.flat) - chain["final"]).max())
    print("chain: loss %.3g (bound %.3g), params %.3g (bound %.3g)" % (worst, X.BOUND_CHAIN["loss"], dp, X.BOUND_CHAIN["params"]))
    record("chain_51", {"loss": worst, "loss_bound": X.BOUND_CHAIN["loss"], "params": dp, "params_bound": X.BOUND_CHAIN["params"]})
    assert eng.optimizer.step_count == X.CHAIN_UPDATES == 51 and eng.update_index == 51
    assert not np.array_equal(_np(eng.target_network.flat), _np(eng.q.flat)) and not np.array_equal(_np(eng.target_network.flat), chain["target"])
    assert (_np(eng.bonus) < 0).any() and (_np(eng.bonus) >= -1.0).all()
    assert worst <= X.BOUND_CHAIN["loss"] and dp <= X.BOUND_CHAIN["params"]


def test_fused_update_is_bitwise_the_unfused_sequence_and_repeatable(dev, chain, R):
    """mi_md_update (in-launch index draw, Adam on the slab sum) against sample() (libmirl's mi_dqn_sample) + grad() + deep_rl_amd.Adam.step over 4 updates with a
    target sync between them; the same four updates once more give the same bits"""
    a, b = _chain_engine(dev, chain), _chain_engine(dev, chain)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        assert np.array_equal(_np(a.batch_inds), _np(b.batch_inds)) and _np(a.batch_inds).max() < X.CHAIN_STEPS   # the in-launch draw is mi_dqn_sample's
        assert np.array_equal(_np(a.batch_inds), R.dqn_sample(CHAIN_SEED, u, X.CHAIN_STEPS, X.CHAIN_BATCH))
        for x, y in ((a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
                     (a.target_values, b.target_values), (a.current, b.current), (a.next_actions, b.next_actions), (a.bonus, b.bonus), (a.soft_value, b.soft_value)):
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
    """saved mid-run through the base class's branch of checkpoint.py and loaded into a fresh engine built with the same three knobs (constructor arguments, like
    gamma): acting and training continue bit for bit; a DoubleDQNEngine does not take the file"""
    import deep_rl_amd as A
    from deep_rl_amd import checkpoint
    kw = dict(learning_starts=100, total_timesteps=2000, alpha=0.7, tau=0.05, clip_lo=-0.5)
    a = _chain_engine(dev, chain, **kw)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "mdqn"), a)
    b = make_engine(dev, 1, X.CHAIN_STEPS + 1, seed=CHAIN_SEED, batch_size=X.CHAIN_BATCH, **kw)
    b.reset()
    checkpoint.load(path, b)
    assert b.global_step == a.global_step == X.CHAIN_STEPS + 30 and b.update_index == 3 and b.optimizer.step_count == 3
    for u in range(3):
        for eng in (a, b):
            eng.act(10); eng.train_step()
            if u == 1:
                eng.sync_target()
    for x, y in ((a.q.flat, b.q.flat), (a.target_network.flat, b.target_network.flat), (a.observations, b.observations), (a.actions, b.actions), (a.terminated, b.terminated),
                 (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.observation, b.observation), (a.bonus, b.bonus),
                 (a.soft_value, b.soft_value)):
        assert np.array_equal(_np(x), _np(y))
    assert not np.array_equal(_np(a.q.flat), chain["params"]) and (_np(a.bonus) >= -0.5).all()
    other = make_engine(dev, 1, X.CHAIN_STEPS + 1, seed=CHAIN_SEED, batch_size=X.CHAIN_BATCH, cls=A.DoubleDQNEngine, learning_starts=100, total_timesteps=2000)
    other.reset()
    with pytest.raises(A._native.MiError, match="MunchausenDQNEngine"):
        checkpoint.load(path, other)


def test_acting_and_forward_are_double_dqns(dev):
    """act() and forward() are inherited and go through libmirl_ddqn.so: on the same seed the two engines fill their rings with the same bits"""
    import deep_rl_amd as A
    import _dqn_cases as D
    params = D.init_params(np.random.default_rng(3))[0]
    kw = dict(params=params, seed=9, learning_starts=45, total_timesteps=400, max_episodes_logged=64)
    md, dd = make_engine(dev, 5, 70, **kw), make_engine(dev, 5, 70, cls=A.DoubleDQNEngine, **kw)
    for eng in (md, dd):
        eng.reset()
        eng.act(64); eng.act(36)
    assert md.global_step == dd.global_step == 100
    for name in ("observations", "actions", "rewards", "terminated", "observation", "episode_stats"):
        assert np.array_equal(_np(getattr(md, name)), _np(getattr(dd, name))), name
    assert set(np.unique(_np(md.actions)).tolist()) == {0, 1} and md.drain_episodes() == dd.drain_episodes()
    obs = torch.from_numpy(D._draw_obs(np.random.default_rng(4), 37))
    assert np.array_equal(_np(md.forward(obs)), _np(dd.forward(obs)))


def test_evaluate_is_the_same_loud_error_and_so_are_bad_arguments(dev):
    import deep_rl_amd as A
    from deep_rl_amd import _native as N
    eng = make_engine(dev, 1, 16)
    eng.reset()
    with pytest.raises(N.MiError) as mine:
        A.evaluate(eng)
    with pytest.raises(N.MiError) as theirs:
        A.evaluate(make_engine(dev, 1, 16, cls=A.DoubleDQNEngine))
    assert str(mine.value).replace("MunchausenDQNEngine", "DoubleDQNEngine") == str(theirs.value)
    with pytest.raises(N.MiError):
        eng.train_step()                         # empty ring
    with pytest.raises(N.MiError):
        eng.sample(np.arange(5))                 # a wrong index count
    for kw in (dict(tau=0.0), dict(tau=-0.03), dict(clip_lo=0.25), dict(alpha=float("nan"))):
        with pytest.raises(N.MiError):
            make_engine(dev, 1, 16, **kw)
    eng.act(8)
    eng.tau = 0.0                                # past the constructor: the library's own check, with its text
    with pytest.raises(N.MiError, match="tau must be > 0"):
        eng.train_step()
    eng.tau, eng.clip_lo = 0.03, 0.5
    with pytest.raises(N.MiError, match="clip_lo must be <= 0"):
        eng.target()
    assert eng.update_index == 0 and eng.optimizer.step_count == 0
