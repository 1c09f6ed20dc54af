"""ns_grad_kernel, ns_target_kernel and ns_reduce_kernel (deep_rl_amd/csrc/mi_nstep.hip, the walk of mi_nwalk.h) on the synthetic rings of tests/_nstep_cases.py
(validated on the CPU by tests/test_nstep_cases_cpu.py) against FLOAT64 AUTOGRAD (tests/_nstep_ref.py), through NStepDQNEngine with forced indices, a placed head and
placed weights: every kind of row — full horizon, terminated at step 1, in between and at n, cut by the head, ending on it, sitting on it, terminated on it,
crossing the ring's end, repeated — with n_step 1, 2, 3, 5 and 16, on one row, on one row more than the gradient launch has workgroups and on a batch whose
workgroups walk three rows.

Everything no walk reads holds NaN (observations — the intermediate ones included — and rewards, those beyond each stop included), 2 (actions) or 1 (terminated),
so a stray read shows in the result.  horizon and next_actions are compared exactly; the bounds are _nstep_ref.BOUND = max(8 x the float32 evaluation's measured
distance from float64, the bar the suite holds DQN to).  No case and no row is excluded.

The anchor: all sixteen rings of tests/_pdd_cases.py through mi_ns_grad with n_step 1 at three head positions give mi_pdd_grad's bits.
Observed maxima go to nstep_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _nstep_cases as K
import _nstep_ref as X
import _pdd_cases as PK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def make_engine(dev, n, slots, params=None, target=None, seed=1, base=0, batch_size=128, cls=None, **kw):
    """NStepDQNEngine (or `cls`) as the script builds it: two DuelingQNetworks and deep_rl_amd.Adam at optim.Adam's defaults"""
    import deep_rl_amd as A

    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    torch.manual_seed(seed)
    q, tq = A.DuelingQNetwork(env), A.DuelingQNetwork(env)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    return (cls or A.NStepDQNEngine)(env, q, tq, A.Adam(q, lr=X.LR), slots=slots, batch_size=batch_size, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).copy().view(np.uint32)


def record(key, value):
    path = os.path.join(X.results_dir(), "nstep_gpu_maxima.json")
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
    try:
        from deep_rl_amd import _native_ns
        d["nstep_source_id"] = _native_ns.source_id()
    except Exception:   # noqa: BLE001  (the id is a label on the record, not what is tested here)
        pass
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _engine(dev, c, weights="case", head=None, cls=None, **kw):
    """weights "case": the case's own (None: a uniform engine, whose launches get NULL); an array: a prioritized engine holding it.  The engine's global_step puts
    the head where the case (or `head`) has it, in a ring that has wrapped."""
    (N, S) = c["ring"]
    w = c["weights"] if isinstance(weights, str) else weights
    eng = make_engine(dev, N, S, params=c["params"], target=c["target"], batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0, prioritized=w is not None, cls=cls, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S + (c["head"] if head is None else head)     # min(global_step, slots) * N: every transition of the ring is stored
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
    bits = [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_values), _bits(eng.current), _bits(eng.td_abs), _np(eng.next_actions).copy()]
    if hasattr(eng, "horizon"):
        got["horizon"] = _np(eng.horizon).astype(np.int64)
        bits.append(_np(eng.horizon).copy())
    return got, bits


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(dev, i):
    c = K.make_case(i)
    fam, e = c["family"], c["exp"]
    eng = _engine(dev, c, n_step=c["n_step"])
    assert (eng.N, eng.slots, eng.batch_size, eng.gamma, eng.prioritized, eng.n_step) == (c["ring"][0], c["ring"][1], c["mb"], c["gamma"], c["weights"] is not None, c["n_step"])
    assert eng.global_step % eng.slots == c["head"]
    eng.batch_inds.copy_(torch.from_numpy(c["idx"]))
    eng.horizon.fill_(-7)
    eng.target()
    alone = (_np(eng.next_actions).copy(), _bits(eng.target_values), _np(eng.horizon).copy())
    eng.horizon.fill_(-7)
    _grad(eng)
    got, bits = _result(eng)
    assert np.array_equal(alone[0], got["next_actions"]) and np.array_equal(alone[1], bits[2]) and np.array_equal(alone[2], bits[6]), "mi_ns_target is not the gradient launch's first pass"
    _grad(eng)
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    assert np.array_equal(got["horizon"], e["horizon"]), "horizon differs on rows %s" % np.flatnonzero(got["horizon"] != e["horizon"])
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something no walk reads was read or multiplied, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    flat = c["observations"].reshape(-1, 4)
    obs = np.concatenate([flat[c["idx"]], flat[e["at"]]])
    got["q"], got["q_ref"] = _np(eng.forward(torch.from_numpy(obs))).astype(np.float64), X.P.forward(c["params"], obs)
    fig = X.figures(e, got, fam)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=c["mb"], n_step=c["n_step"]))
    assert set(fig) == set(X.FIGURES)
    assert not X.within(fig, fam), (c["name"], X.within(fig, fam))
    assert np.array_equal(_bits(eng.td_abs), np.abs(_np(eng.target_values) - _np(eng.current)).view(np.uint32))      # |td| of the f32 values written out, unweighted
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    if c["gamma"] == 0.0:                                   # the target is r_1, bit for bit
        (N, S), idx = c["ring"], c["idx"]
        assert np.array_equal(bits[2], c["rewards"].reshape(-1)[((idx // N + 1) % S) * N + idx % N].view(np.uint32))
    if c["weights"] is None or c["wkind"] == "one":        # weights NULL == weights all 1.0f, bit for bit
        other = _engine(dev, c, weights=np.ones(c["mb"], np.float32) if c["weights"] is None else None, n_step=c["n_step"])
        assert other.prioritized == (c["weights"] is None)
        other.batch_inds.copy_(torch.from_numpy(c["idx"]))
        _grad(other)
        _, obits = _result(other)
        assert all(np.array_equal(a, b) for a, b in zip(bits, obits)), "weights NULL and weights of 1.0f give different bits"
    # mi_ns_update from fresh optimizer state: the same gradient bit for bit, parameters that are one Adam step on it
    step = _engine(dev, c, n_step=c["n_step"])
    step.batch_inds.copy_(torch.from_numpy(c["idx"]))
    o = step.optimizer
    a = step.K.AdamArgs(step.K.ptr(o.exp_avg), step.K.ptr(o.exp_avg_sq), 1, X.LR, X.BETAS[0], X.BETAS[1], X.ADAM_EPS)
    step.K.update(step._ring, step._batch(0), a, step._s())
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "mi_ns_update's gradient / loss / target / current / td_abs / horizon are not mi_ns_grad's bits"
    p = c["params"].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    X.adam_step(p, got["grads"], m, v, 1)
    after = _np(step.q.flat)
    assert np.abs(after - p).max() <= 1e-6                 # (the bound of tests/test_gpu_pdd_cases.py: a step of at most lr in f32, p - step rounded once)
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits


@pytest.mark.parametrize("i", range(len(PK.SPECS)), ids=PK.NAMES)
def test_one_step_is_mi_pdd_grad_bit_for_bit_wherever_the_head_is(dev, i):
    """the anchor: n_step 1 on every ring of tests/_pdd_cases.py, with the head in slot 0, in the last slot and in the slot of a sampled row"""
    import deep_rl_amd as A

    c = PK.make_case(i)
    (N, S) = c["ring"]
    pdd = _engine(dev, dict(c, head=0), cls=A.PDDDQNEngine)
    pdd.batch_inds.copy_(torch.from_numpy(c["idx"]))
    _grad(pdd)
    want, wbits = _result(pdd)
    assert np.array_equal(want["next_actions"], c["exp"]["next_actions"]) and len(wbits) == 6
    for head in (0, S - 1, int(c["idx"][0]) // N):
        eng = _engine(dev, c, head=head, n_step=1)
        assert eng.global_step % S == head
        eng.batch_inds.copy_(torch.from_numpy(c["idx"]))
        eng.horizon.fill_(-7)
        _grad(eng)
        _, bits = _result(eng)
        for name, a, b in zip(("grads", "loss", "target", "current", "td_abs", "next_actions"), bits, wbits):
            assert np.array_equal(a, b), "%s differs from mi_pdd_grad's with the head in slot %d" % (name, head)
        assert (bits[6] == 1).all()


def test_update_is_bitwise_grad_plus_adam_and_the_in_launch_draw_is_mi_dqn_sample(dev):
    """uniform mode, n_step 3, on the CPU-built ring of the chained tests: mi_ns_update (in-launch index draw, Adam on the slab sum) against sample() (libmirl's
    mi_dqn_sample) + grad() + deep_rl_amd.Adam.step (libmirl's mi_adam) over 4 updates with a target sync between them; the same four updates once more give the
    same bits"""
    from oracle import cpu_ref as R
    R.lib().ref_set_num_threads(8)
    ring, _, _, params, target = X.chain_data(R)

    def engine():
        eng = make_engine(dev, 1, X.CHAIN_STEPS + 1, params=params, target=target, seed=X.CHAIN_SEED, batch_size=X.CHAIN_BATCH, prioritized=False, n_step=X.CHAIN_N)
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
                     (a.target_values, b.target_values), (a.current, b.current), (a.td_abs, b.td_abs), (a.next_actions, b.next_actions), (a.horizon, b.horizon)):
            assert np.array_equal(_np(x), _np(y)), u
        assert np.array_equal(_np(a.horizon), X.walk(ring, _np(a.batch_inds), X.CHAIN_N, X.CHAIN_STEPS, 0.99)[3]) and set(_np(a.horizon).tolist()) <= {1, 2, 3} and _np(a.horizon).max() == 3
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
