"""pdd_grad_kernel, pdd_target_kernel and pdd_reduce_kernel (deep_rl_amd/csrc/mi_pdd.hip) on the synthetic rings of tests/_pdd_cases.py (validated on the CPU by
tests/test_pdd_cases_cpu.py) against FLOAT64 AUTOGRAD (tests/_pdd_ref.py), through PDDDQNEngine with forced indices and placed weights: one row in the last slot
of a two-slot ring, 5 rows, one row more than the gradient launch has workgroups, a batch whose workgroups walk three rows, weights NULL, all 1 and spanning 1e-3 .. 1
with an exact 0, target == online bit for bit, an online head that ties bit for bit, whole batches with live == 0 and live == 1, gamma 0 and 1, action values of 30,
advantage rows that cancel, pre-activations of exactly 0.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_pdd_ref.BOUND = max(8 x the float32 torch evaluation's measured distance from float64, the bar the suite holds DQN to).  No case and no row is excluded, action
comparisons included.  On the uniform cases the same batch also goes through libmirl's plain-DQN image of the dueling networks (mi_dueling_pack), libmirl_ddqn.so's
gradient launch and mi_dueling_unpack_grads: another device evaluation by other kernels, which must agree within the same bound.  Observed maxima go to
pdd_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _dqn_cases as D
import _pdd_cases as K
import _pdd_ref as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def make_engine(dev, n, slots, params=None, target=None, seed=1, base=0, batch_size=128, **kw):
    """PDDDQNEngine as the script builds it: two DuelingQNetworks and deep_rl_amd.Adam at optim.Adam's defaults"""
    import deep_rl_amd as A

    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    torch.manual_seed(seed)
    q, tq = A.DuelingQNetwork(env), A.DuelingQNetwork(env)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    return A.PDDDQNEngine(env, q, tq, A.Adam(q, lr=X.LR), slots=slots, batch_size=batch_size, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).copy().view(np.uint32)


def record(key, value):
    path = os.path.join(X.results_dir(), "pdd_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    if "family" in value:
        fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
        for k in X.FIGURES:
            if k in value:
                fam[k] = max(fam.get(k, 0.0), value[k])
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _engine(dev, c, weights="case"):
    """weights "case": the case's own (None: a uniform engine, whose launches get NULL); an array: a prioritized engine holding it"""
    (N, S) = c["ring"]
    w = c["weights"] if isinstance(weights, str) else weights
    eng = make_engine(dev, N, S, params=c["params"], target=c["target"], batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0, prioritized=w is not None)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S                                    # min(global_step, slots) * N: every transition of the ring is stored
    if w is not None:
        eng.weights.copy_(torch.from_numpy(w))
    return eng


def _grad(eng):
    """the library's gradient call alone (RingEngine.grad: PDDDQNEngine.grad adds the priority scatter, which is libmirl's and tested in tests/test_gpu_pdd.py)"""
    from deep_rl_amd._ring_engine import RingEngine
    RingEngine.grad(eng)


def _result(eng):
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target=_np(eng.target_values).astype(np.float64),
               current=_np(eng.current).astype(np.float64), td_abs=_np(eng.td_abs).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64))
    return got, [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_values), _bits(eng.current), _bits(eng.td_abs), _np(eng.next_actions).copy()]


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(dev, i):
    c = K.make_case(i)
    fam, e = c["family"], c["exp"]
    eng = _engine(dev, c)
    assert (eng.N, eng.slots, eng.batch_size, eng.gamma, eng.prioritized) == (c["ring"][0], c["ring"][1], c["mb"], c["gamma"], c["weights"] is not None)
    eng.batch_inds.copy_(torch.from_numpy(c["idx"]))
    eng.target()
    alone = (_np(eng.next_actions).copy(), _bits(eng.target_values))
    _grad(eng)
    got, bits = _result(eng)
    assert np.array_equal(alone[0], got["next_actions"]) and np.array_equal(alone[1], bits[2]), "mi_pdd_target is not the gradient launch's first pass"
    _grad(eng)
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    if fam in K.TIES:
        assert not got["next_actions"].any()               # torch.argmax: a bit-for-bit tie goes to action 0
    obs = np.concatenate([c["observations"].reshape(-1, 4)[c["idx"]], c["observations"].reshape(-1, 4)[D.successor(c["idx"], *c["ring"])]])
    got["q"], got["q_ref"] = _np(eng.forward(torch.from_numpy(obs))).astype(np.float64), X.forward(c["params"], obs)
    fig = X.figures(e, got, fam)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=c["mb"]))
    assert set(fig) == set(X.FIGURES)
    assert not X.within(fig, fam), (c["name"], X.within(fig, fam))
    assert np.array_equal(_bits(eng.td_abs), np.abs(_np(eng.target_values) - _np(eng.current)).view(np.uint32))      # |td| of the f32 values written out, unweighted
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    if fam in K.TIES:                                      # the online q of a tie case is one number twice, on the device too
        q = _np(eng.forward(torch.from_numpy(obs)))
        assert np.array_equal(q[:, 0].view(np.uint32), q[:, 1].view(np.uint32))
    if c["name"] == "terminal_all_9":                      # live == 0 in every row: another target vector, the same bits
        eng.target_network.load_flat(np.random.default_rng(99).normal(0, 1, X.NP).astype(np.float32))
        _grad(eng)
        _, bits3 = _result(eng)
        assert all(np.array_equal(a, b) for a, b in zip(bits, bits3)), "the target net reaches a batch whose successors are all terminated"
    if c["weights"] is None or c["wkind"] == "one":        # weights NULL == weights all 1.0f, bit for bit
        other = _engine(dev, c, weights=np.ones(c["mb"], np.float32) if c["weights"] is None else None)
        assert other.prioritized == (c["weights"] is None)
        other.batch_inds.copy_(torch.from_numpy(c["idx"]))
        _grad(other)
        _, obits = _result(other)
        assert all(np.array_equal(a, b) for a, b in zip(bits, obits)), "weights NULL and weights of 1.0f give different bits"
    # mi_pdd_update from fresh optimizer state: the same gradient bit for bit, parameters that are one Adam step on it
    step = _engine(dev, c)
    step.batch_inds.copy_(torch.from_numpy(c["idx"]))
    o = step.optimizer
    a = step.K.AdamArgs(step.K.ptr(o.exp_avg), step.K.ptr(o.exp_avg_sq), 1, X.LR, X.BETAS[0], X.BETAS[1], X.ADAM_EPS)
    step.K.update(step._ring, step._batch(0), a, step._s())
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "mi_pdd_update's gradient / loss / target / current / td_abs are not mi_pdd_grad's bits"
    p = c["params"].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    X.adam_step(p, got["grads"], m, v, 1)
    after = _np(step.q.flat)
    assert np.abs(after - p).max() <= 1e-6                 # (the bound of tests/test_gpu_ddqn_cases.py: a step of at most lr in f32, p - step rounded once)
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits


@pytest.mark.parametrize("i", K.UNIFORM, ids=[K.NAMES[i] for i in K.UNIFORM])
def test_uniform_case_agrees_with_the_dueling_image_through_the_double_dqn_library(dev, i):
    """mi_dueling_pack images of both networks through mi_ddqn_grad, then mi_dueling_unpack_grads: the same loss and gradient by other kernels of two other
    libraries.  next_actions equal; loss, target, current and the gradient within the device bound of the family."""
    import deep_rl_amd as A
    from deep_rl_amd import _native as N

    c = K.make_case(i)
    fam, e = c["family"], c["exp"]
    eng = _engine(dev, c)
    eng.batch_inds.copy_(torch.from_numpy(c["idx"]))
    _grad(eng)
    mine, _ = _result(eng)
    (Nn, S) = c["ring"]
    env = A.make("CartPole-v1", num_envs=Nn, device=dev, seed=1)
    q, tq = A.QNetwork(env), A.QNetwork(env)
    q.flat.copy_(eng.q.eff); tq.flat.copy_(eng.target_network.eff)        # DuelingQNetwork.load_flat repacked them
    dd = A.DoubleDQNEngine(env, q, tq, A.Adam(q, lr=X.LR), slots=S, batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(dd, name).copy_(torch.from_numpy(c[name]))
    dd.global_step = S
    dd.sample(c["idx"])
    dd.grad()
    buf = torch.zeros(N.DUELING_NPARAMS + 2, dtype=torch.float32, device=dev)
    N.check(N.lib().mi_dueling_unpack_grads(N.ptr(dd.grads), N.ptr(buf), N.stream_ptr(dev)), "mi_dueling_unpack_grads")
    theirs = dict(grads=_np(buf[:N.DUELING_NPARAMS]).astype(np.float64), loss=float(dd.loss.item()), target=_np(dd.target_values).astype(np.float64),
                  current=_np(dd.current).astype(np.float64), next_actions=_np(dd.next_actions).astype(np.int64))
    assert np.array_equal(theirs["next_actions"], mine["next_actions"]) and np.array_equal(mine["next_actions"], e["next_actions"])
    scale = float(np.abs(e["target"]).max()) if fam == "scale" else 1.0
    fig = dict(grad=float(np.abs(theirs["grads"] - mine["grads"]).max() / np.abs(e["grads"]).max()), loss=abs(theirs["loss"] - mine["loss"]) / abs(e["loss"]),
               target=float(np.abs(theirs["target"] - mine["target"]).max()) / scale, current=float(np.abs(theirs["current"] - mine["current"]).max()) / scale)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
    record("image_" + c["name"], dict(fig, mb=c["mb"]))
    assert np.isfinite(theirs["grads"]).all() and not X.within(fig, fam), (c["name"], X.within(fig, fam))


def test_update_is_bitwise_grad_plus_adam_and_the_in_launch_draw_is_mi_dqn_sample(dev):
    """uniform mode on the CPU-built ring of the chained tests: mi_pdd_update (in-launch index draw, Adam on the slab sum) against sample() (libmirl's mi_dqn_sample)
    + grad() + deep_rl_amd.Adam.step (libmirl's mi_adam) over 4 updates with a target sync between them; the same four updates once more give the same bits"""
    from oracle import cpu_ref as R
    R.lib().ref_set_num_threads(8)
    ring, _, _, params, target = X.chain_data(R)

    def engine():
        eng = make_engine(dev, 1, X.CHAIN_STEPS + 1, params=params, target=target, seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=False)
        for name in ("observations", "actions", "rewards", "terminated"):
            getattr(eng, name).copy_(torch.from_numpy(ring[name]))
        eng.global_step = X.CHAIN_STEPS
        return eng

    a, b = engine(), engine()
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        assert np.array_equal(_np(a.batch_inds), _np(b.batch_inds)) and _np(a.batch_inds).max() < X.CHAIN_STEPS   # the in-launch draw is mi_dqn_sample's
        assert np.array_equal(_np(a.batch_inds), R.dqn_sample(X.CHAIN_SEED, u, X.CHAIN_STEPS, X.CHAIN_BATCH))
        for x, y in ((a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
                     (a.target_values, b.target_values), (a.current, b.current), (a.td_abs, b.td_abs), (a.next_actions, b.next_actions)):
            assert np.array_equal(_np(x), _np(y)), u
        if u == 1:
            a.sync_target(); b.sync_target()
    assert a.optimizer.step_count == b.optimizer.step_count == 4 and a.update_index == 4
    assert not np.array_equal(_np(a.q.flat), _np(a.target_network.flat)) and np.isfinite(_np(a.q.flat)).all()
    c = engine()
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat)) and np.array_equal(_np(c.grads), _np(a.grads)) and np.array_equal(_np(c.loss), _np(a.loss))
