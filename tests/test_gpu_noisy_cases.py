"""nz_grad_kernel, nz_target_kernel, nz_forward_kernel, nz_reduce_kernel and nz_noise_kernel (deep_rl_amd/csrc/mi_noisy.hip) on the cases of tests/_noisy_cases.py
(validated on the CPU by tests/test_noisy_cases_cpu.py) against FLOAT64 AUTOGRAD through mu + sigma * eps (tests/_noisy_ref.py) FED THE DEVICE'S OWN SAMPLE from
mi_nz_noise, through NoisyDQNEngine with forced indices, a placed head, placed weights and a placed update index: the fourteen poisoned n-step rings under sigma 0,
the default sigma, sigma x 8, noisy = 0, synced parameters and a weight of exactly 0.

horizon and next_actions are compared exactly; the bounds are _noisy_ref.BOUND = max(8 x the float32 evaluation's measured distance from float64, the bar the
suite holds DQN to).  No case and no row is excluded.  The device's sample itself is held to the restatement: xi |xi| against the float64 z, the element products
bit for bit, mean and variance of 4,096 samples, and that the streams and the two networks of an update draw different samples.

The anchor: all fourteen rings through mi_nz_grad with noisy = 0 give mi_ns_grad's bits on the first 11,019 floats and exact zeros in the sigma gradient.
Observed maxima go to noisy_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _noisy_cases as C
import _noisy_ref as Z
import _nstep_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def make_engine(dev, n, slots, params=None, target=None, seed=1, base=0, batch_size=128, **kw):
    """NoisyDQNEngine as the script builds it: two NoisyDuelingQNetworks and deep_rl_amd.Adam at optim.Adam's defaults"""
    import deep_rl_amd as A

    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    torch.manual_seed(seed)
    q, tq = A.NoisyDuelingQNetwork(env), A.NoisyDuelingQNetwork(env)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    return A.NoisyDQNEngine(env, q, tq, A.Adam(q, lr=Z.LR), slots=slots, batch_size=batch_size, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).copy().view(np.uint32)


def record(key, value):
    path = os.path.join(Z.results_dir(), "noisy_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    if "family" in value:
        fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
        for k in Z.FIGURES:
            if k in value:
                fam[k] = max(fam.get(k, 0.0), value[k])
    try:
        from deep_rl_amd import _native_nz
        d["noisy_source_id"] = _native_nz.source_id()
    except Exception:   # noqa: BLE001  (the id is a label on the record, not what is tested here)
        pass
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def device_sample(dev, seed, a, b, stream):
    """-> (xi [171], eps [255]) float32 numpy from mi_nz_noise"""
    from deep_rl_amd import _native_nz as N

    xi, eps = torch.full((171,), np.nan, dtype=torch.float32, device=dev), torch.full((255,), np.nan, dtype=torch.float32, device=dev)
    N.noise(seed, a, b, stream, xi, eps, N.stream_ptr(dev))
    return _np(xi), _np(eps)


def _engine(dev, c, weights="case", noisy=None, **kw):
    """weights "case": the case's own (None: a uniform engine, whose launches get NULL); an array: a prioritized engine holding it.  global_step puts the head where
    the case has it in a ring that has wrapped; the env's seed and update_index are the case's noise key."""
    (N, S) = c["ring"]
    w = c["weights"] if isinstance(weights, str) else weights
    eng = make_engine(dev, N, S, params=c["params"], target=c["target"], seed=c["noise_seed"], batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0,
                      prioritized=w is not None, n_step=c["n_step"], noisy=bool(c["noisy"]) if noisy is None else noisy, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S + c["head"]
    eng.update_index = c["u"]
    if w is not None:
        eng.weights.copy_(torch.from_numpy(w))
    eng.batch_inds.copy_(torch.from_numpy(c["idx"]))
    return eng


def _grad(eng):
    """the library's gradient call alone (RingEngine.grad: PDDDQNEngine.grad adds the priority scatter, which is libmirl's)"""
    from deep_rl_amd._ring_engine import RingEngine
    RingEngine.grad(eng)


def _result(eng):
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target=_np(eng.target_values).astype(np.float64),
               current=_np(eng.current).astype(np.float64), td_abs=_np(eng.td_abs).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64),
               horizon=_np(eng.horizon).astype(np.int64))
    bits = [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_values), _bits(eng.current), _bits(eng.td_abs), _np(eng.next_actions).copy(), _np(eng.horizon).copy()]
    return got, bits


@pytest.mark.parametrize("i", range(len(C.SPECS)), ids=C.NAMES)
def test_case_against_float64_fed_the_device_sample(dev, i):
    c = C.make_case(i)
    fam = c["family"]
    eng = _engine(dev, c)
    assert eng.q.flat.numel() == 11274 and eng.grads.numel() == 11274 and eng.global_step % eng.slots == c["head"] and eng.noisy == bool(c["noisy"])
    xi_on, eps_on = device_sample(dev, c["noise_seed"], c["u"], 0, Z.STREAM_LEARN)
    xi_tg, _ = device_sample(dev, c["noise_seed"], c["u"], 1, Z.STREAM_LEARN)
    assert np.abs(xi_on * np.abs(xi_on) - Z.normal(c["noise_seed"], c["u"], 0, 14, np.float64)).max() <= Z.BOUND_DRAW["z"]
    e = Z.evaluate(c, xi_on=xi_on, xi_tg=xi_tg)                       # float64, the device's own factors
    assert np.array_equal(e["next_actions"], c["exp"]["next_actions"]), "the device's sample and the restatement's choose different actions: the case's q gap does not cover the draw's error"
    eng.horizon.fill_(-7)
    eng.target()
    alone = (_np(eng.next_actions).copy(), _bits(eng.target_values), _np(eng.horizon).copy())
    eng.horizon.fill_(-7)
    _grad(eng)
    got, bits = _result(eng)
    assert np.array_equal(alone[0], got["next_actions"]) and np.array_equal(alone[1], bits[2]) and np.array_equal(alone[2], bits[6]), "mi_nz_target is not the gradient launch's first pass"
    _grad(eng)
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    assert np.array_equal(got["horizon"], e["horizon"]), "horizon differs on rows %s" % np.flatnonzero(got["horizon"] != e["horizon"])
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    flat = c["observations"].reshape(-1, 4)
    obs = np.concatenate([flat[c["idx"]], flat[e["at"]]])
    key = (c["u"], 0, Z.STREAM_LEARN) if c["noisy"] else None
    got["q"], got["q_ref"] = _np(eng.forward(torch.from_numpy(obs), noise=key)).astype(np.float64), Z.forward(c["params"], obs, xi_on if c["noisy"] else None)
    fig = Z.figures(e, got, c["ring_family"])
    print(c["name"], fam, {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=c["mb"], n_step=c["n_step"]))
    assert set(fig) == set(Z.FIGURES)
    assert not Z.within(fig, fam), (c["name"], Z.within(fig, fam))
    assert np.array_equal(_bits(eng.td_abs), np.abs(_np(eng.target_values) - _np(eng.current)).view(np.uint32))
    g32 = _np(eng.grads)
    if c["noisy"]:                                                     # slab[SIGMA + t] = gh * eps_t: one product per slab; with one slab it is the product of the outputs
        if c["mb"] == 1:
            assert np.array_equal(g32[Z.SIGMA:], g32[Z.HEAD:Z.SIGMA] * eps_on)      # (as values: the slab sum starts from +0, so a product of -0 arrives as +0)
    else:
        assert not g32[Z.SIGMA:].any() and np.array_equal(g32[Z.SIGMA:].view(np.uint32), np.zeros(255, np.uint32))      # exact zeros, +0
    # mi_nz_update from fresh optimizer state: the same gradient bit for bit, parameters that are one Adam step on it
    step = _engine(dev, c)
    o = step.optimizer
    a = step.K.AdamArgs(step.K.ptr(o.exp_avg), step.K.ptr(o.exp_avg_sq), 1, Z.LR, Z.BETAS[0], Z.BETAS[1], Z.ADAM_EPS)
    step.K.update(step._ring, step._batch(0), a, step._s())
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "mi_nz_update's outputs are not mi_nz_grad's bits"
    p = c["params"].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    Z.adam_step(p, got["grads"], m, v, 1)
    after = _np(step.q.flat)
    assert np.abs(after - p).max() <= 1e-6                 # (the bound of tests/test_gpu_nstep_cases.py: a step of at most lr in f32, p - step rounded once)
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_noisy_off_is_mi_ns_grad_bit_for_bit(dev, i):
    """the anchor: every ring with its non-zero sigma in place and noisy = 0 against NStepDQNEngine on the first 11,019 floats; mi_nz_target and mi_nz_forward too"""
    import test_gpu_nstep_cases as TN

    base = K.make_case(i)
    c = C.make_case(i)
    if not c["params"][Z.SIGMA:].any():                                # the sigma_0 rings: give the anchor a sigma it must ignore
        c = dict(c, params=np.concatenate([c["params"][:Z.SIGMA], Z.default_sigma()]), target=np.concatenate([c["target"][:Z.SIGMA], Z.default_sigma(2.0)]))
    ns = TN._engine(dev, base, n_step=base["n_step"])
    ns.batch_inds.copy_(torch.from_numpy(base["idx"]))
    ns.target()
    want_t = (_np(ns.next_actions).copy(), _bits(ns.target_values), _np(ns.horizon).copy())
    TN._grad(ns)
    _, wbits = TN._result(ns)
    eng = _engine(dev, c, noisy=False)
    eng.horizon.fill_(-7)
    eng.target()
    assert np.array_equal(_np(eng.next_actions), want_t[0]) and np.array_equal(_bits(eng.target_values), want_t[1]) and np.array_equal(_np(eng.horizon), want_t[2])
    _grad(eng)
    _, bits = _result(eng)
    assert np.array_equal(bits[0][:Z.NP_MEAN], wbits[0]), "the gradient's first 11,019 floats differ from mi_ns_grad's"
    assert np.array_equal(bits[0][Z.SIGMA:], np.zeros(255, np.uint32)), "the sigma gradient is not exact zeros"
    for name, a, b in zip(("loss", "target", "current", "td_abs", "next_actions", "horizon"), bits[1:], wbits[1:]):
        assert np.array_equal(a, b), "%s differs from mi_ns_grad's" % name
    obs = torch.from_numpy(base["observations"].reshape(-1, 4)[base["idx"]])
    assert np.array_equal(_bits(eng.forward(obs)), _bits(ns.forward(obs))), "mi_nz_forward without a key is not mi_pdd_forward"


def test_the_device_draw(dev):
    """the sample as the kernels form it against the restatement; 4,096 samples' moments; different keys, different samples"""
    seed = 20181
    xs, es = zip(*[device_sample(dev, seed, u, 0, Z.STREAM_LEARN) for u in range(24)])
    xs, es = np.array(xs), np.array(es)
    z64 = Z.normal(seed, np.arange(24), 0, Z.STREAM_LEARN, np.float64)
    d = float(np.abs(xs * np.abs(xs) - z64).max())
    print("device draw: xi |xi| against float64 z: %.3g (bound %.3g)" % (d, Z.BOUND_DRAW["z"]))
    record("draw", dict(z=d, samples=24 * 171))
    assert d <= Z.BOUND_DRAW["z"]
    assert np.array_equal(np.sign(xs), np.sign(z64))
    for x, e in zip(xs, es):                                           # the element products, bit for bit from the device's own factors
        assert np.array_equal(e.view(np.uint32), Z.eps_of(x).view(np.uint32))
    # 4,096 numbers: 24 samples of 171 are 4,104; the first 4,096 of them
    z = (xs * np.abs(xs)).astype(np.float64).reshape(-1)[:4096]
    assert abs(z.mean()) <= 5 / np.sqrt(4096) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / 4096)
    act, _ = device_sample(dev, seed, 0, 0, Z.STREAM_ACT)
    tgt, _ = device_sample(dev, seed, 0, 1, Z.STREAM_LEARN)
    other_seed, _ = device_sample(dev, seed + 1, 0, 0, Z.STREAM_LEARN)
    far, _ = device_sample(dev, seed, (1 << 40) + 3, (1 << 33) + 9, Z.STREAM_ACT)
    for o in (act, tgt, other_seed, xs[1]):
        assert not np.array_equal(o, xs[0]) and abs(np.corrcoef(o, xs[0])[0, 1]) < 0.3
    assert np.abs(far * np.abs(far) - Z.normal(seed, (1 << 40) + 3, (1 << 33) + 9, Z.STREAM_ACT, np.float64)).max() <= Z.BOUND_DRAW["z"]      # 64-bit keys reach the counter
    assert np.abs(act * np.abs(act) - Z.normal(seed, 0, 0, Z.STREAM_ACT, np.float64)).max() <= Z.BOUND_DRAW["z"]


def test_update_is_bitwise_grad_plus_adam_over_four_updates(dev):
    """uniform mode, n_step 3, on the CPU-built ring of the chained tests: mi_nz_update (in-launch index draw, Adam on the slab sum of all 11,274 elements) against
    sample() + grad() + deep_rl_amd.Adam.step over 4 updates with a target sync between them; every update draws new samples; the same four once more give the
    same bits"""
    from oracle import cpu_ref as R
    R.lib().ref_set_num_threads(8)
    ring, _, _, params, target, _ = Z.chain_data(R)

    def engine():
        eng = make_engine(dev, 1, Z.CHAIN_STEPS + 1, params=params, target=target, seed=Z.CHAIN_SEED, batch_size=Z.CHAIN_BATCH, prioritized=False, n_step=Z.CHAIN_N)
        for name in ("observations", "actions", "rewards", "terminated"):
            getattr(eng, name).copy_(torch.from_numpy(ring[name]))
        eng.global_step = Z.CHAIN_STEPS
        return eng

    a, b = engine(), engine()
    sig = []
    for u in range(4):
        a.train_step()
        b.sample(); b.grad(); b.optimizer.step(b.grads); b.update_index += 1
        assert np.array_equal(_np(a.batch_inds), _np(b.batch_inds)) and np.array_equal(_np(a.batch_inds), R.dqn_sample(Z.CHAIN_SEED, u, Z.CHAIN_STEPS, Z.CHAIN_BATCH))
        for x, y in ((a.q.flat, b.q.flat), (a.grads, b.grads), (a.loss, b.loss), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq),
                     (a.target_values, b.target_values), (a.current, b.current), (a.td_abs, b.td_abs), (a.next_actions, b.next_actions), (a.horizon, b.horizon)):
            assert np.array_equal(_np(x), _np(y)), u
        sig.append(_np(a.grads)[Z.SIGMA:].copy())
        if u == 1:
            a.sync_target(); b.sync_target()
    assert a.optimizer.step_count == b.optimizer.step_count == 4 and a.update_index == 4
    assert all(s.any() for s in sig) and not np.array_equal(_np(a.q.flat)[Z.SIGMA:], params[Z.SIGMA:])            # the sigmas learn
    c = engine()
    for u in range(4):
        c.train_step()
        if u == 1:
            c.sync_target()
    assert np.array_equal(_np(c.q.flat), _np(a.q.flat)) and np.array_equal(_np(c.grads), _np(a.grads)) and np.array_equal(_np(c.loss), _np(a.loss))
