"""n-step prioritized dueling Double DQN on the MI355X (libmirl_nstep.so, include/mi_nstep.h through NStepDQNEngine): with n_step 1 the engine IS PDDDQNEngine
bit for bit through acting and training; the walk against a LIVE head — a ring the acting launch itself filled, before and after it wraps; 51 chained prioritized
updates against the float64 restatement (tests/_nstep_ref.py); the fused train_step against the unfused sequence; checkpoint / resume in both modes; loud errors.

The bounds are _nstep_ref.BOUND / BOUND_CHAIN: max(8 x what the float32 evaluation measures against float64, the bar the suite holds DQN to).  Observed maxima go to
nstep_gpu_maxima.json in the tests' results directory."""
import ctypes as C

import numpy as np
import pytest
import torch

import _nstep_ref as X
from test_gpu_nstep_cases import _np, make_engine, record

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
        ring, indices, weights, params, target = X.chain_data(R)
    finally:
        R.set_sincos_mode("libm")
    return dict(ring=ring, indices=indices, weights=weights, params=params, target=target)


def _chain_engine(dev, chain, prioritized=True, **kw):
    """every transition of the CPU-built ring stored; prioritized: each at the initial max_priority, as acting would have left them"""
    kw.setdefault("n_step", X.CHAIN_N)
    eng = make_engine(dev, 1, X.CHAIN_STEPS + 1, params=chain["params"], target=chain["target"], seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=prioritized, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(chain["ring"][name]))
    eng.global_step = X.CHAIN_STEPS
    if prioritized:
        eng.priorities[:X.CHAIN_STEPS] = 1e-2
        eng.refresh_sums()
    return eng


@pytest.mark.parametrize("prioritized", [True, False], ids=["prioritized", "uniform"])
def test_engine_with_one_step_is_the_pdd_engine_bit_for_bit(dev, prioritized):
    """the same seed through 200 acting steps of 3 envs on a 64-slot ring (it wraps three times, learning_starts inside) and 20 train_steps with a target sync"""
    import deep_rl_amd as A

    kw = dict(seed=11, batch_size=64, learning_starts=45, total_timesteps=400, max_episodes_logged=0, prioritized=prioritized)
    a, b = make_engine(dev, 3, 64, n_step=1, **kw), make_engine(dev, 3, 64, cls=A.PDDDQNEngine, **kw)
    assert type(a) is A.NStepDQNEngine and type(b) is A.PDDDQNEngine and a.K is not b.K
    a.reset(); b.reset()
    for u in range(20):
        for eng in (a, b):
            eng.act(10); eng.train_step()
            if u == 9:
                eng.sync_target()
        assert (_np(a.horizon) == 1).all()
    assert a.global_step == b.global_step == 200 and a.optimizer.step_count == b.optimizer.step_count == 20
    pairs = [(a.q.flat, b.q.flat), (a.target_network.flat, b.target_network.flat), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
             (a.observations, b.observations), (a.actions, b.actions), (a.terminated, b.terminated), (a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.grads, b.grads),
             (a.target_values, b.target_values), (a.current, b.current), (a.td_abs, b.td_abs), (a.next_actions, b.next_actions)]
    if prioritized:
        pairs += [(a.priorities, b.priorities), (a.max_priority, b.max_priority), (a.weights, b.weights)]
    for k, (x, y) in enumerate(pairs):
        assert np.array_equal(_np(x), _np(y)), k
    assert not np.array_equal(_np(a.q.flat), _np(a.target_network.flat)) and np.isfinite(_np(a.q.flat)).all()


def _live_check(eng, idx, label):
    """target() and grad() on `idx` against the float64 reference evaluated on the ring copied off the device, with head = global_step % slots"""
    from deep_rl_amd._ring_engine import RingEngine

    S, N = eng.slots, eng.N
    head = eng.global_step % S
    c = dict(params=_np(eng.q.flat), target=_np(eng.target_network.flat), idx=idx, n_step=eng.n_step, head=head, gamma=eng.gamma, weights=None,
             **{k: _np(getattr(eng, k)) for k in ("observations", "actions", "rewards", "terminated")})
    e = X.evaluate(c)
    eng.sample(idx)
    eng.horizon.fill_(-7)
    eng.target()
    hz, tg, na = _np(eng.horizon).astype(np.int64), _np(eng.target_values).astype(np.float64), _np(eng.next_actions).astype(np.int64)
    assert np.array_equal(hz, e["horizon"]), (label, np.flatnonzero(hz != e["horizon"]))
    err = float(np.abs(tg - e["target"]).max())
    clear = np.abs(e["q_next"][:, 0] - e["q_next"][:, 1]) >= X.CLOSE_Q["plain"]
    assert np.array_equal(na[clear], e["next_actions"][clear]) and clear.mean() > 0.9
    eng.horizon.fill_(-7)
    RingEngine.grad(eng)
    assert np.array_equal(_np(eng.horizon), hz) and np.array_equal(_np(eng.target_values).astype(np.float64), tg)
    gerr = float(np.abs(_np(eng.grads) - e["grads"]).max() / np.abs(e["grads"]).max())
    record("live_head_" + label, dict(target=err, target_bound=X.BOUND["plain"]["target"], grad=gerr, head=int(head), horizons=sorted(set(hz.tolist()))))
    assert err <= X.BOUND["plain"]["target"] and (not clear.all() or gerr <= X.BOUND["plain"]["grad"])
    return e, head


def test_walk_against_a_live_head_before_and_after_the_ring_wraps(dev):
    """3 envs x 16 slots, batch 48, n_step 3, forced actions (always push right) that end an episode about every 10 steps"""
    N, S, B = 3, 16, 48
    eng = make_engine(dev, N, S, seed=3, batch_size=B, learning_starts=0, total_timesteps=400, max_episodes_logged=0, prioritized=False, n_step=3)
    rng = np.random.default_rng(5)
    eng.q.flat.copy_(torch.from_numpy((_np(eng.q.flat) + rng.normal(0, 0.05, X.NP)).astype(f32)))
    eng.target_network.flat.copy_(torch.from_numpy((_np(eng.target_network.flat) + rng.normal(0, 0.05, X.NP)).astype(f32)))
    eng.reset()
    push = torch.ones((10, N), dtype=torch.int64)
    eng.act(10, forced_actions=push)
    assert eng.global_step == 10 and eng._upper() == 30
    stored = np.arange(30, dtype=np.int64)
    idx = np.concatenate([stored, stored[:B - 30]])                      # the 30 stored rows, repeated to fill the batch
    e, head = _live_check(eng, idx, "unwrapped")
    assert head == 10
    m = e["horizon"][:30].reshape(10, N)                                 # [slot][env]
    term = _np(eng.terminated)
    assert (m[9] == 1).all() and (m[8] <= 2).all()                       # the newest rows stop at the head
    assert ((m[8] == 2) | (term[9] != 0)).all() and {1, 2, 3} <= set(m.reshape(-1).tolist())
    for _ in range(3):
        eng.act(10, forced_actions=push)
    assert eng.global_step == 40 and eng._upper() == S * N == B
    e, head = _live_check(eng, np.arange(B, dtype=np.int64), "wrapped")
    assert head == 8
    m, term = e["horizon"].reshape(S, N), _np(eng.terminated)
    assert (m[7] == 1).all() and (m[6] <= 2).all()                       # cut by the head
    assert (m[8] >= 1).all() and ((m[8] > 1) | (term[9] != 0)).all()     # the stale rows ON the head: step 1 taken, then on unless terminated
    assert term.sum() >= 3 and ((m < 3) & (term.reshape(-1)[e["at"]].reshape(S, N) != 0)).any() and (m == 3).any()
    assert (m[15] > 1).any()                                             # a walk across the ring's end


def test_51_prioritized_updates_chained_with_a_target_sync(dev, chain):
    """§18's CPU-built ring, n_step 3; the device draws every batch from its own priorities and the float64 chain is fed the device's indices and weights; every
    loss and the parameters behind update 50 against it"""
    eng = _chain_engine(dev, chain)
    idx, w, losses, hz = [], [], [], set()
    for k in range(X.CHAIN_UPDATES):
        eng.train_step()
        idx.append(_np(eng.batch_inds).copy()); w.append(_np(eng.weights).copy()); losses.append(float(eng.loss.item()))
        hz |= set(_np(eng.horizon).tolist())
        if k == 25:
            eng.sync_target()
    idx, w = np.stack(idx), np.stack(w)
    assert idx.min() >= 0 and idx.max() < X.CHAIN_STEPS and (w.max(axis=1) == 1).all() and (w > 0).all() and w[1:].min() < 0.9 and hz == {1, 2, 3}
    assert len({tuple(r) for r in idx}) == X.CHAIN_UPDATES                  # every update drew another batch
    l64, p64 = X.chain(chain["ring"], idx, w, chain["params"], chain["target"], X.CHAIN_N, X.CHAIN_STEPS)
    worst = float((np.abs(np.array(losses) - l64) / np.abs(l64)).max())
    dp = float(np.abs(_np(eng.q.flat) - p64).max())
    record("chain_51", {"loss": worst, "loss_bound": X.BOUND_CHAIN["loss"], "params": dp, "params_bound": X.BOUND_CHAIN["params"]})
    assert eng.optimizer.step_count == X.CHAIN_UPDATES == 51 and eng.update_index == 51
    assert not np.array_equal(_np(eng.target_network.flat), _np(eng.q.flat)) and not np.array_equal(_np(eng.target_network.flat), chain["target"])
    assert worst <= X.BOUND_CHAIN["loss"] and dp <= X.BOUND_CHAIN["params"]


def test_prioritized_train_step_is_bitwise_the_unfused_sequence_and_repeatable(dev, chain):
    """sampler + mi_ns_update + scatter against sample() + grad() (mi_ns_grad + scatter) + deep_rl_amd.Adam.step over 4 updates with a target sync between them"""
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


@pytest.mark.parametrize("prioritized", [True, False], ids=["prioritized", "uniform"])
def test_checkpoint_resume_is_bit_exact_and_n_step_is_part_of_it(dev, chain, tmp_path, prioritized):
    from deep_rl_amd import _native as N
    from deep_rl_amd import checkpoint
    kw = dict(learning_starts=100, total_timesteps=2000)
    a = _chain_engine(dev, chain, prioritized=prioritized, **kw)
    a.reset()
    for u in range(3):
        a.act(10); a.train_step()
    path = checkpoint.save(str(tmp_path / "nstep"), a)
    other = make_engine(dev, 1, X.CHAIN_STEPS + 1, seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=prioritized, n_step=2, **kw)
    other.reset()
    with pytest.raises(N.MiError, match="n_step"):
        checkpoint.load(path, other)                                        # another n_step computes another algorithm
    b = make_engine(dev, 1, X.CHAIN_STEPS + 1, seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=prioritized, n_step=X.CHAIN_N, **kw)
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
    for x, y in pairs() + [(a.batch_inds, b.batch_inds), (a.loss, b.loss), (a.td_abs, b.td_abs), (a.horizon, b.horizon)] + ([(a.weights, b.weights)] if prioritized else []):
        assert np.array_equal(_np(x), _np(y))
    assert not np.array_equal(_np(a.q.flat), chain["params"]) and _np(a.horizon).max() == X.CHAIN_N


def test_errors_are_loud(dev):
    import deep_rl_amd as A
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_ns as K
    env = A.make("CartPole-v1", num_envs=1, device=dev, seed=1)
    q = A.DuelingQNetwork(env)
    for bad, slots in ((0, 64), (17, 64), (-1, 64), (8, 8), (3, 3)):
        with pytest.raises(N.MiError, match="n_step"):
            A.NStepDQNEngine(env, q, A.DuelingQNetwork(env), A.Adam(q, lr=X.LR), slots=slots, n_step=bad)
    wrong = A.QNetwork(env)
    with pytest.raises(N.MiError):
        A.NStepDQNEngine(env, wrong, wrong, A.Adam(wrong, lr=X.LR), slots=16)                # a network of another size
    for prioritized in (True, False):
        eng = make_engine(dev, 1, 128, prioritized=prioritized)
        assert eng.n_step == 3
        eng.reset()
        with pytest.raises(N.MiError):
            eng.train_step()                         # empty ring
        assert eng.global_step == 0
        eng.act(8)
        with pytest.raises(N.MiError):
            eng.train_step(np.arange(5))             # a wrong index count
        assert eng.update_index == 0 and eng.optimizer.step_count == 0
    # straight at the C ABI: the walk's own arguments — negative codes, the text names the call, nothing is launched
    eng = make_engine(dev, 1, 128)
    eng.reset(); eng.act(8); eng.sample()
    L = K.lib()
    a = K.AdamArgs(K.ptr(eng.optimizer.exp_avg), K.ptr(eng.optimizer.exp_avg_sq), 1, X.LR, 0.9, 0.999, 1e-8)
    before = _np(eng.q.flat).copy()
    eng.horizon.fill_(-7)

    def all_three(b, text):
        assert L.mi_ns_target(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and text in L.mi_ns_last_error() and b"mi_ns_target" in L.mi_ns_last_error()
        assert L.mi_ns_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and text in L.mi_ns_last_error()
        assert L.mi_ns_update(C.byref(eng._ring), C.byref(b), C.byref(a), eng._s()) == -1 and text in L.mi_ns_last_error()

    for n in (0, 17, 128, -3):
        b = eng._batch(0); b.n_step = n
        all_three(b, b"n_step")
    for h in (-1, 128):
        b = eng._batch(0); b.head_slot = h
        all_three(b, b"head_slot")
    b = eng._batch(0); b.horizon = None
    all_three(b, b"horizon is NULL")
    b = eng._batch(0); b.td_abs = None
    assert L.mi_ns_grad(C.byref(eng._ring), C.byref(b), eng._s()) == -1 and b"a batch buffer is NULL" in L.mi_ns_last_error()
    a.step = 0
    assert L.mi_ns_update(C.byref(eng._ring), C.byref(eng._batch(0)), C.byref(a), eng._s()) == -1   # optimizer step < 1
    torch.cuda.synchronize()
    assert np.array_equal(_np(eng.q.flat), before) and (_np(eng.horizon) == -7).all()               # nothing was launched
