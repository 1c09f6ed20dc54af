"""Prioritized dueling Double DQN on the MI355X (libmirl_pdd.so, include/mi_pdd.h through PDDDQNEngine): the acting launch against the unchanged C oracle's DQN
acting, the 500-step TimeLimit cases, the forward API, the prioritized bookkeeping around libmirl's sampler, 51 chained prioritized updates against the float64 torch
restatement (tests/_pdd_ref.py), checkpoint / resume in both modes, loud errors.

Acting is DQN's with another network, so the oracle's dqn_act_steps / dqn_epsilon / dqn_explore_draw are its yardstick, bit for bit on everything but the greedy
choice, which is compared with the float64 dueling forward wherever its two action values differ by at least 1e-4 (the margin of tests/test_gpu_dqn.py).  The
update's bounds are _pdd_ref.BOUND / BOUND_CHAIN: max(8 x what float32 torch measures against float64, the bar the suite holds DQN to).  Observed maxima go to
pdd_gpu_maxima.json in the tests' results directory."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dqn_cases as D
import _pdd_ref as X
import _timelimit_cases as T
from test_gpu_pdd_cases import _np, make_engine, record
from test_gpu_timelimit import _check_call, _check_ring, _checkpoint_inside_a_long_episode, _reset_case, _reset_inside_an_episode, _run_forced, _snapshot, _start

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


@pytest.fixture(autouse=True)
def _fdlibm(R):
    R.set_sincos_mode("fdlibm")
    yield
    R.set_sincos_mode("libm")


@pytest.fixture(scope="module")
def chain(R):
    """the ring of the chained-update tests, computed once on the CPU"""
    ring, indices, weights, params, target = X.chain_data(R)
    return dict(ring=ring, indices=indices, weights=weights, params=params, target=target)


def _chain_engine(dev, chain, prioritized=True, **kw):
    """every transition of the CPU-built ring stored; prioritized: each at the initial max_priority, as acting would have left them"""
    eng = make_engine(dev, 1, X.CHAIN_STEPS + 1, params=chain["params"], target=chain["target"], seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=prioritized, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(chain["ring"][name]))
    eng.global_step = X.CHAIN_STEPS
    if prioritized:
        eng.priorities[:X.CHAIN_STEPS] = 1e-2
        eng.refresh_sums()
    return eng


# ---- acting ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 37, 4096])
def test_act_steps_keyed_rng_ring_wrap(dev, R, n):
    """3 / 37 / 4,096 envs (one env per workgroup up to 1,024, four beyond), a 16-slot ring (wraps many times), learning_starts = 45 inside a call, epsilon
    decaying to 0.05 within the test: the device's actions replayed on the oracle give all four ring tensors and `observation` bit for bit; at the first step of
    each call the decision follows the contract (the keyed random action before learning_starts and on exploring steps, the float64 dueling argmax on greedy ones
    whose margin is at least 1e-4).  Prioritized: after every call the rows written hold max_priority and the write head holds 0."""
    S, tt, ls, k = 16, 400, 45, 10
    g0, calls = (40, 2) if n == 4096 else (0, 40)          # the large shape runs steps 40 .. 59: its first call straddles learning_starts too
    eng = make_engine(dev, n, S, seed=5, base=300, learning_starts=ls, total_timesteps=tt, max_episodes_logged=0)
    assert eng.prioritized
    rng = np.random.default_rng(1)
    params = (_np(eng.q.flat) + rng.normal(0, 0.05, X.NP)).astype(f32)
    eng.q.flat.copy_(torch.from_numpy(params))             # (.flat alone: this engine never reads .eff)
    env = R.VecCartPole(n, seed=5, env_id_base=300); st = R.ReplayStorage(S, n)
    obs_cur = env.reset(); st.observations[g0 % S] = obs_cur
    eng.global_step = g0
    assert np.array_equal(_np(eng.reset()), obs_cur)
    unused = np.zeros(D.NP, f32)                           # the oracle's network: never evaluated, every action is forced
    gs, n_greedy, n_random, n_checked = g0, 0, 0, 0
    for call in range(calls):
        obs_before = _np(eng.observation).copy()
        eng.act(k)
        fa = np.stack([_np(eng.actions[(gs + s) % S]) for s in range(k)])   # the device's actions of this call (k <= S), replayed on the oracle
        R.dqn_act_steps(env, unused, st, obs_cur, k, gs, learning_starts=ls, total_timesteps=tt, forced_actions=fa)
        for name in ("observations", "actions", "rewards", "terminated"):
            assert np.array_equal(_np(getattr(eng, name)), getattr(st, name)), (call, name)
        assert np.array_equal(_np(eng.observation), obs_cur)
        eps = f32(R.dqn_epsilon(gs, total_timesteps=tt))
        qv = X.forward(params, obs_before)
        for e in range(0, n, 7 if n > 7 else 1):
            u, ra = R.dqn_explore_draw(5, 300 + e, gs - g0)                 # (the env step counters start at 0 whatever global_step is)
            if gs < ls or u < eps:
                assert fa[0, e] == ra; n_random += 1
            elif abs(qv[e, 0] - qv[e, 1]) >= 1e-4:
                assert fa[0, e] == int(qv[e, 1] > qv[e, 0]); n_greedy += 1
            n_checked += 1
        gs += k
        prio = _np(eng.priorities)
        written = [(g % S) for g in range(max(g0, gs - (S - 1)), gs)]
        assert (prio[written] == f32(1e-2)).all() and (prio[gs % S] == 0).all(), (call, "priorities after act")
    assert eng.global_step == gs and float(eng.max_priority.item()) == float(f32(1e-2))
    assert n_greedy > (10 if n == 3 else 50) and n_random > (10 if n == 3 else 50) and n_checked >= (120 if n == 3 else 240)


def test_an_env_acts_as_its_single_env_engine(dev):
    """shard invariance: env E of an N = 5 engine acts exactly as an N = 1 engine with env_id_base = E (64 steps across learning_starts)"""
    rng = np.random.default_rng(3)
    params = D.init_params(rng)[1]
    kw = dict(params=params, seed=9, learning_starts=45, total_timesteps=400, max_episodes_logged=0, prioritized=False)
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


@pytest.mark.parametrize("rows", [1, 5, 300, 1500])
def test_forward_against_float64(dev, rows):
    """1,500 rows: more than the 1,024 workgroups of the forward launch"""
    rng = np.random.default_rng(rows)
    params = D.init_params(rng)[1]
    obs = D._draw_obs(rng, rows)
    eng = make_engine(dev, 1, 2, params=params, prioritized=False)
    q = _np(eng.forward(torch.from_numpy(obs)))
    q64 = X.forward(params, obs)
    err = float(np.abs(q - q64).max())
    record("forward_%d" % rows, {"q": err, "bound": X.BOUND["plain"]["q"], "max_abs_q": float(np.abs(q64).max())})
    assert q.shape == (rows, 2) and q.dtype == f32 and err <= X.BOUND["plain"]["q"]
    lead = _np(eng.forward(torch.from_numpy(obs).reshape(1, rows, 4)))
    assert lead.shape == (1, rows, 2) and np.array_equal(lead[0], q)


# ---- the 500-step TimeLimit (tests/_timelimit_cases.py) ------------------------------------------------------------------
def _tl_make(dev, n, slots, params=None, greedy=False, prioritized=False):
    """params: the flat parameter vector (default: zeros — the teacher-forced paths run no forward); greedy: epsilon 0 and no learning_starts from step 0"""
    import deep_rl_amd as A
    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=5, env_id_base=300)
    q, tgt = A.DuelingQNetwork(env), A.DuelingQNetwork(env)
    q.load_flat(np.zeros(X.NP, f32) if params is None else params)
    tgt.load_state_dict(q.state_dict())
    kw = dict(learning_starts=0, start_e=0.0, end_e=0.0) if greedy else {}
    return A.PDDDQNEngine(env, q, tgt, A.Adam(q, lr=2.5e-4), slots=slots, max_episodes_logged=8192, prioritized=prioritized, **kw)


@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
def test_teacher_forced_acting_at_the_limit(dev, forced, schedule):
    """1,100 steps of the scripted 5-env case: one run (prioritized) on a ring that holds the whole run, compared at the end; one (uniform: a prioritized acting call
    must be shorter than the ring) on 16 slots, compared after every call"""
    case = T.get("n5", forced)
    call_list = T.calls(schedule, case.steps)
    for slots, every in ((case.steps + 1, False), (16, True)):
        eng = _tl_make(dev, case.n, slots, prioritized=slots > case.steps)
        _start(eng, case)
        _run_forced(eng, case, call_list, slots, every, ("pdd", forced, schedule, slots))
        if slots > case.steps:      # the stored flag is `terminated`, not `done`: the two differ exactly on the truncated steps
            differ = _np(eng.terminated)[1:] != case.done.astype(np.uint8)
            assert np.array_equal(differ, case.trunc) and differ.sum() == case.counts()["truncations"] >= 2
            trunc_step, trunc_env = np.nonzero(case.trunc)      # a truncated step leaves terminated = 0 and the RESET observation in the next slot
            assert not _np(eng.terminated)[1:][trunc_step, trunc_env].any()
            assert np.array_equal(_np(eng.observations)[1:][trunc_step, trunc_env], case.obs[1:][trunc_step, trunc_env])
            assert (_np(eng.priorities)[:case.steps] == f32(1e-2)).all() and (_np(eng.priorities)[case.steps] == 0).all()


@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
def test_two_envs_per_workgroup_at_the_limit(dev, forced):
    """1,030 envs on a grid capped at 1,024 workgroups: workgroups 0 - 5 walk two long-episode envs each; all 1,030 envs are compared"""
    case = T.get("n1030", forced)
    eng = _tl_make(dev, case.n, case.steps + 1)
    _start(eng, case)
    _run_forced(eng, case, T.calls("49+50", case.steps), case.steps + 1, False, ("pdd", forced, "49+50", case.steps + 1))


def test_greedy_controller_runs_into_the_limit(dev):
    """FORCED = false: the hand-built dueling controller network (q_1 - q_0 = K w . obs) acts greedily for 1,100 steps.  The device's own actions are replayed on the
    oracle: ring, flags, statistics, log and `elapsed` exact; the action is (q_1 > q_0) of a float64 forward wherever the two values are at least DQN's close-value
    distance apart (at most 1 % left out); at least one env is truncated twice."""
    from oracle import cpu_ref as Rr
    n, steps = 5, 1100
    slots = steps + 1
    params = T.CONTROLLERS["dueling"](T.CONTROLLER_K)
    eng = _tl_make(dev, n, slots, params=params, greedy=True, prioritized=True)
    eng.reset()
    snaps, call_list = [], T.calls("49+50", steps)
    for k in call_list:
        eng.act(k)
        snaps.append(_snapshot(eng))
    actions = _np(eng.actions)[:steps]
    assert set(np.unique(actions).tolist()) == {0, 1}
    case = T.replay(Rr, n, 5, 300, actions)
    g = 0
    for k, snap in zip(call_list, snaps):
        _check_call(snap, case, g, k, "pdd")
        g += k
    _check_ring(eng, case, steps, slots, "pdd")
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    q = T.q64("dueling", params, case.obs[:-1].reshape(-1, 4))
    far = np.abs(q[:, 1] - q[:, 0]) >= T.close_q("dueling")
    assert (~far).mean() <= 0.01, int((~far).sum())
    assert np.array_equal(actions.reshape(-1)[far], (q[:, 1] > q[:, 0]).astype(np.int64)[far])


def test_checkpoint_inside_a_long_episode(dev, tmp_path):
    """saved at global step 300 of the 5-env case, loaded into a fresh engine whose env was driven somewhere else, continued to step 620: ring, `elapsed`, log and
    statistics equal the uninterrupted run bit for bit, and the truncation comes at step 500 (the body of tests/test_gpu_timelimit.py's test); prioritized engines"""
    _checkpoint_inside_a_long_episode(lambda n, slots, params=None: _tl_make(dev, n, slots, params=params, prioritized=True), T.get("n5", False), X.NP,
                                      str(tmp_path / "pdd"), "pdd")


def test_reset_inside_an_episode_restarts_the_limit(dev):
    """300 balanced steps, reset(), 520 more: no truncation at step 500, every env truncated 500 steps after the reset"""
    from oracle import cpu_ref as Rr
    _reset_inside_an_episode(lambda n, slots: _tl_make(dev, n, slots), _reset_case(Rr, 5), "pdd")


# ---- the prioritized bookkeeping (libmirl's sampler, driven by this engine) ----------------------------------------------
def test_train_step_scatters_td_abs_last_duplicate_wins_and_keeps_the_running_max(dev, chain):
    eng = _chain_engine(dev, chain)
    rng = np.random.default_rng(11)
    mp = float(f32(1e-2))
    for u in range(3):
        idx = rng.integers(0, X.CHAIN_STEPS, X.CHAIN_BATCH)
        idx[5], idx[77], idx[127] = idx[3], idx[3], idx[100]                # repeated rows: the same row evaluated twice gives the same |td|, so placed below
        before = _np(eng.priorities).reshape(-1).copy()
        eng.train_step(idx)
        td = _np(eng.td_abs)
        want = before.copy()
        for b in range(X.CHAIN_BATCH):
            want[idx[b]] = td[b]                                            # in batch order: the last duplicate wins
        assert np.array_equal(_np(eng.batch_inds), idx) and np.array_equal(_np(eng.priorities).reshape(-1).view(np.uint32), want.view(np.uint32)), u
        assert td[5] == td[3] == td[77] and (td > 0).all() and np.array_equal(td.view(np.uint32), np.abs(_np(eng.target_values) - _np(eng.current)).view(np.uint32))
        mp = max(mp, float(td.max()))
        assert float(eng.max_priority.item()) == mp, u                      # the running maximum: it never comes down
        w = _np(eng.weights)
        assert w.max() == 1.0 and (w > 0).all() and (u == 0) == bool((w == 1.0).all())      # equal priorities: every weight exactly 1; afterwards they differ
    assert eng.update_index == 3 and eng.optimizer.step_count == 3
    # the incremental chunk sums are what a full pass gives
    inc = eng._per_ws.clone()
    eng.refresh_sums()
    n0 = (X.CHAIN_STEPS + 1 + 63) // 64; n1 = (n0 + 63) // 64
    assert torch.equal(inc.view(torch.float64)[:2 * n0 + 2 * n1], eng._per_ws.view(torch.float64)[:2 * n0 + 2 * n1])
    # a later acting call gives its new rows the running max, not the initial one
    eng.reset()
    eng.act(4)
    assert (_np(eng.priorities)[X.CHAIN_STEPS % eng.slots] == f32(mp)).all() and mp > 1e-2


def test_sample_draws_what_PERDQNEngine_draws(dev):
    """the same seed, ring shape, counters and priorities (equal ones, then random ones with zeros): libmirl's sampler gives both engines the same indices and weights"""
    import deep_rl_amd as A
    n, S, B = 7, 100, 256
    kw = dict(batch_size=B, total_timesteps=1000, max_episodes_logged=0)
    mine = make_engine(dev, n, S, seed=9, **kw)
    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=9)
    q, tq = A.QNetwork(env), A.QNetwork(env)
    per = A.PERDQNEngine(env, q, tq, A.ClipAdam(q, lr=X.LR, eps=1e-8), slots=S, **kw)
    rng = np.random.default_rng(4)
    prio = rng.gamma(0.5, 1.0, (S, n)).astype(f32)
    prio[rng.random((S, n)) < 0.15] = 0.0
    for p in (np.full((S, n), 0.37, f32), prio):
        p = p.copy(); p[63:] = 0.0
        for eng in (mine, per):
            eng.priorities.copy_(torch.from_numpy(p)); eng.refresh_sums()
            eng.global_step, eng.update_index = 63, 17
            eng.sample()
        assert np.array_equal(_np(mine.batch_inds), _np(per.batch_inds)) and _np(mine.batch_inds).max() < 63 * n
        assert np.array_equal(_np(mine.weights).view(np.uint32), _np(per.weights).view(np.uint32)) and float(mine.weights.max()) == 1.0
        assert mine.beta() == per.beta() == (1 - 0.4) * 63 / 1000 + 0.4
        keep = rng.choice(np.flatnonzero(p.reshape(-1) > 0), B)
        mine.sample(keep); per.sample(keep)
        assert np.array_equal(_np(mine.batch_inds), keep) and np.array_equal(_np(mine.weights).view(np.uint32), _np(per.weights).view(np.uint32))
    assert len(np.unique(_np(mine.weights))) > 10


def test_51_prioritized_updates_chained_with_a_target_sync(dev, chain):
    """the ring is built ON THE CPU (oracle acting, keyed RNG, fixed parameters); the device draws every batch from its own priorities and the float64 torch chain is
    fed the device's indices and weights; every loss and the parameters behind update 50 against it"""
    eng = _chain_engine(dev, chain)
    idx, w, losses = [], [], []
    for k in range(X.CHAIN_UPDATES):
        eng.train_step()
        idx.append(_np(eng.batch_inds).copy()); w.append(_np(eng.weights).copy()); losses.append(float(eng.loss.item()))
        if k == 25:
            eng.sync_target()
    idx, w = np.stack(idx), np.stack(w)
    assert idx.min() >= 0 and idx.max() < X.CHAIN_STEPS and (w.max(axis=1) == 1).all() and (w > 0).all() and w[1:].min() < 0.9
    assert len({tuple(r) for r in idx}) == X.CHAIN_UPDATES                  # every update drew another batch
    l64, p64 = X.chain(chain["ring"], idx, w, chain["params"], chain["target"])
    worst = float((np.abs(np.array(losses) - l64) / np.abs(l64)).max())
    dp = float(np.abs(_np(eng.q.flat) - p64).max())
    record("chain_51", {"loss": worst, "loss_bound": X.BOUND_CHAIN["loss"], "params": dp, "params_bound": X.BOUND_CHAIN["params"]})
    assert eng.optimizer.step_count == X.CHAIN_UPDATES == 51 and eng.update_index == 51
    assert not np.array_equal(_np(eng.target_network.flat), _np(eng.q.flat)) and not np.array_equal(_np(eng.target_network.flat), chain["target"])
    assert worst <= X.BOUND_CHAIN["loss"] and dp <= X.BOUND_CHAIN["params"]


def test_prioritized_train_step_is_bitwise_the_unfused_sequence_and_repeatable(dev, chain):
    """sampler + mi_pdd_update + scatter against sample() + grad() (mi_pdd_grad + scatter) + deep_rl_amd.Adam.step over 4 updates with a target sync between them"""
    a, b = _chain_engine(dev, chain), _chain_engine(dev, chain)
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        for x, y in ((a.batch_inds, b.batch_inds), (a.weights, b.weights), (a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg),
                     (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.target_values, b.target_values), (a.current, b.current), (a.next_actions, b.next_actions),
                     (a.td_abs, b.td_abs), (a.priorities, b.priorities), (a.max_priority, b.max_priority)):
            assert np.array_equal(_np(x), _np(y)), u
        if u == 1:
            a.sync_target(); b.sync_target()
    c = _chain_engine(dev, chain)
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat)) and np.array_equal(_np(c.priorities), _np(a.priorities)) and np.array_equal(_np(c.loss), _np(a.loss))


@pytest.mark.parametrize("prioritized", [True, False], ids=["prioritized", "uniform"])
def test_checkpoint_resume_is_bit_exact(dev, chain, tmp_path, prioritized):
    from deep_rl_amd import checkpoint
    kw = dict(learning_starts=100, total_timesteps=2000)
    a = _chain_engine(dev, chain, prioritized=prioritized, **kw)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "pdd"), a)
    b = make_engine(dev, 1, X.CHAIN_STEPS + 1, seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=prioritized, **kw)
    b.reset()
    checkpoint.load(path, b)
    assert b.global_step == a.global_step == X.CHAIN_STEPS + 30 and b.update_index == 3 and b.optimizer.step_count == 3
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
    for x, y in pairs() + [(a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.td_abs, b.td_abs)] + ([(a.weights, b.weights)] if prioritized else []):
        assert np.array_equal(_np(x), _np(y))
    assert not np.array_equal(_np(a.q.flat), chain["params"])
    if prioritized:
        assert float(a.max_priority.item()) > 1e-2 and len(np.unique(_np(a.priorities))) > 100


def test_errors_are_loud(dev, monkeypatch):
    import deep_rl_amd as A
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_pdd as K
    from deep_rl_amd import dist
    env = A.make("CartPole-v1", num_envs=1, device=dev, seed=1)
    q, wrong = A.DuelingQNetwork(env), A.QNetwork(env)
    with pytest.raises(N.MiError):
        A.PDDDQNEngine(env, wrong, wrong, A.Adam(wrong, lr=X.LR), slots=16)                  # a network of another size
    with pytest.raises(N.MiError):
        A.PDDDQNEngine(env, q, A.DuelingQNetwork(env), A.Adam(q, lr=X.LR), slots=1)          # slots < 2
    with pytest.raises(N.MiError):
        A.PDDDQNEngine(env, q, A.DuelingQNetwork(env), A.Adam(q, lr=X.LR), slots=16, batch_size=0)   # batch 0
    with monkeypatch.context() as mp:
        mp.setattr(dist, "world_size", lambda group=None: 2)
        with pytest.raises(N.MiError, match="single process"):
            A.PDDDQNEngine(env, q, A.DuelingQNetwork(env), A.Adam(q, lr=X.LR), slots=16)     # world size > 1
    for prioritized in (True, False):
        eng = make_engine(dev, 1, 128, prioritized=prioritized)
        eng.reset()
        with pytest.raises(N.MiError):
            eng.train_step()                         # empty ring
        with pytest.raises(N.MiError):
            eng.sample()                             # empty ring
        with pytest.raises(N.MiError):
            eng.act(65)                              # n_steps 65
        assert eng.global_step == 0
        eng.act(8)
        with pytest.raises(N.MiError):
            eng.sample(np.arange(5))                 # a wrong index count
        with pytest.raises(N.MiError):
            eng.train_step(np.arange(5))
        assert eng.update_index == 0 and eng.optimizer.step_count == 0
    small = make_engine(dev, 1, 16)
    small.reset()
    with pytest.raises(N.MiError, match="shorter than the ring"):
        small.act(16)                                # a prioritized acting call as long as the ring
    assert small.global_step == 0
    # straight at the C ABI: NULL td_abs, a batch of 0, misaligned params — negative codes, the text names the call, nothing is launched
    eng = make_engine(dev, 1, 128)
    eng.reset(); eng.act(8); eng.sample()
    L = K.lib()
    b = eng._batch(0); b.td_abs = None
    assert L.mi_pdd_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and b"a batch buffer is NULL" in L.mi_pdd_last_error()
    a = K.AdamArgs(K.ptr(eng.optimizer.exp_avg), K.ptr(eng.optimizer.exp_avg_sq), 1, X.LR, 0.9, 0.999, 1e-8)
    assert L.mi_pdd_update(C.byref(eng._ring), C.byref(b), C.byref(a), eng._s()) == -1
    b = eng._batch(0); b.batch = 0
    assert L.mi_pdd_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and L.mi_pdd_target(C.byref(eng._ring), C.byref(b), eng._s()) == -1
    b = eng._batch(0); b.params = K.ptr(eng.q.flat) + 4
    assert L.mi_pdd_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and L.mi_pdd_target(C.byref(eng._ring), C.byref(b), eng._s()) == -1
    obs = torch.zeros((1, 4), device=dev); out = torch.zeros((1, 2), device=dev)
    assert L.mi_pdd_forward(K.ptr(eng.q.flat) + 4, K.ptr(obs), 1, K.ptr(out), eng._s()) == -1
    act = K.PDDAct(K.ptr(eng.q.flat) + 4, K.ptr(eng.observation), None, None, None, K.ptr(eng.episode_stats), 0, 100, 0, 1.0, 0.05, 0.5, 1, 0)
    assert L.mi_pdd_act_steps(eng.env.handle, C.byref(eng._ring), C.byref(act), eng._s()) == -1
    a.step = 0
    assert L.mi_pdd_update(C.byref(eng._ring), C.byref(eng._batch(0)), C.byref(a), eng._s()) == -1   # optimizer step < 1
    before = _np(eng.q.flat).copy()
    torch.cuda.synchronize()
    assert np.array_equal(_np(eng.q.flat), before) and eng.optimizer.step_count == 0
