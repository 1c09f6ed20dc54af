"""rb_grad_kernel, rb_target_kernel, rb_forward_kernel, rb_reduce_kernel and rb_noise_kernel (deep_rl_amd/csrc/mi_rainbow.hip) on the cases of
tests/_rainbow_cases.py (validated on the CPU by tests/test_rainbow_cases_cpu.py) against FLOAT64 AUTOGRAD (tests/_rainbow_ref.py) FED THE DEVICE'S OWN SAMPLE from
mi_rb_noise, through RainbowEngine with forced indices, a placed head, placed weights and a placed update index: the fourteen poisoned n-step rings under sigma 0,
the default sigma, sigma x 8, noisy = 0, synced parameters and a weight of exactly 0, on wide and narrow supports with the placed distributional edges.

horizon and next_actions are compared exactly; the bounds are _rainbow_ref.BOUND = max(8 x the float32 evaluation's measured distance from float64, the bar the
suite holds DQN to).  No case and no row is excluded.  The device's sample itself is held to the restatement: xi |xi| against the float64 z, the factors laid over
the rows as the header says, mean and variance of 4,096 numbers, and that the streams and the two networks of an update draw different samples.
Observed maxima go to rainbow_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _noisy_cases as NC
import _rainbow_cases as C
import _rainbow_ref as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def make_engine(dev, n, slots, params=None, target=None, seed=1, base=0, batch_size=128, support=(0.0, 100.0), **kw):
    """RainbowEngine as the script builds it: two RainbowQNetworks and deep_rl_amd.Adam at optim.Adam's defaults"""
    import deep_rl_amd as A

    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    torch.manual_seed(seed)
    q, tq = A.RainbowQNetwork(env, v_min=support[0], v_max=support[1]), A.RainbowQNetwork(env, v_min=support[0], v_max=support[1])
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    return A.RainbowEngine(env, q, tq, A.Adam(q, lr=Z.LR), slots=slots, batch_size=batch_size, v_min=support[0], v_max=support[1], **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).copy().view(np.uint32)


def record(key, value):
    path = os.path.join(Z.results_dir(), "rainbow_gpu_maxima.json")
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
        from deep_rl_amd import _native_rb
        d["rainbow_source_id"] = _native_rb.source_id()
    except Exception:   # noqa: BLE001  (the id is a label on the record, not what is tested here)
        pass
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def device_sample(dev, seed, a, b, stream):
    """-> (xi [321], fin [153, 84], fout [153]) float32 numpy from mi_rb_noise"""
    from deep_rl_amd import _native_rb as N

    nan = lambda *s: torch.full(s, np.nan, dtype=torch.float32, device=dev)   # noqa: E731
    xi, fin, fout = nan(321), nan(153, 84), nan(153)
    N.noise(seed, a, b, stream, xi, fin, fout, N.stream_ptr(dev))
    return _np(xi), _np(fin), _np(fout)


def device_eps(dev, seed, a, b, stream):
    """the element noise [13,005] as float32 products of the device's own factors"""
    _, fin, fout = device_sample(dev, seed, a, b, stream)
    return Z.eps_of(fin, fout)


def _engine(dev, c, weights="case", noisy=None, **kw):
    """weights "case": the case's own (None: a uniform engine, whose launches get NULL); an array: a prioritized engine holding it.  global_step puts the head where
    the case has it in a ring that has wrapped; the env's seed and update_index are the case's noise key."""
    (N, S) = c["ring"]
    w = c["weights"] if isinstance(weights, str) else weights
    eng = make_engine(dev, N, S, params=c["params"], target=c["target"], seed=c["noise_seed"], batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0,
                      prioritized=w is not None, n_step=c["n_step"], noisy=bool(c["noisy"]) if noisy is None else noisy, support=c["support"], **kw)
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
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target_probs=_np(eng.target_probs).astype(np.float64),
               probs=_np(eng.probs).astype(np.float64), prio=_np(eng.prio).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64),
               horizon=_np(eng.horizon).astype(np.int64))
    bits = [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_probs), _bits(eng.probs), _bits(eng.prio), _np(eng.next_actions).copy(), _np(eng.horizon).copy()]
    return got, bits


@pytest.mark.parametrize("i", range(len(C.SPECS)), ids=C.NAMES)
def test_case_against_float64_fed_the_device_sample(dev, i):
    c = C.make_case(i)
    fam = c["family"]
    eng = _engine(dev, c)
    assert eng.q.flat.numel() == 36774 and eng.grads.numel() == 36774 and eng.global_step % eng.slots == c["head"] and eng.noisy == bool(c["noisy"])
    xi_on, fin, fout = device_sample(dev, c["noise_seed"], c["u"], 0, Z.STREAM_LEARN)
    assert np.abs(xi_on * np.abs(xi_on) - Z.normal(c["noise_seed"], c["u"], 0, 14, np.float64)).max() <= Z.BOUND_DRAW["z"]
    e_on, e_tg = Z.eps_of(fin, fout), device_eps(dev, c["noise_seed"], c["u"], 1, Z.STREAM_LEARN)
    e = Z.evaluate(c, e_on=e_on, e_tg=e_tg)                           # float64, the device's own element noise
    assert np.array_equal(e["next_actions"], c["exp"]["next_actions"]), "the device's sample and the restatement's choose different actions: the case's q gap does not cover the draw's error"
    eng.horizon.fill_(-7)
    eng.target()
    alone = (_np(eng.next_actions).copy(), _bits(eng.target_probs), _np(eng.horizon).copy())
    eng.horizon.fill_(-7)
    eng.target_probs.fill_(float("nan"))
    _grad(eng)
    got, bits = _result(eng)
    assert np.array_equal(alone[0], got["next_actions"]) and np.array_equal(alone[1], bits[2]) and np.array_equal(alone[2], bits[6]), "mi_rb_target is not the gradient launch's target pass"
    _grad(eng)
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    assert np.array_equal(got["horizon"], e["horizon"]), "horizon differs on rows %s" % np.flatnonzero(got["horizon"] != e["horizon"])
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    flat = c["observations"].reshape(-1, 4)
    nb = len(c["idx"])
    obs = torch.from_numpy(np.concatenate([flat[c["idx"]], flat[e["at"]]]))
    key = (c["u"], 0, Z.STREAM_LEARN) if c["noisy"] else None
    p_all, q_all = eng.forward(obs, noise=key, probs=True)
    got["q_row"], got["q_next"] = _np(q_all).astype(np.float64)[:nb], _np(q_all).astype(np.float64)[nb:]
    act = (flat_actions(c)[c["idx"]] != 0).astype(np.int64)
    assert np.array_equal(_bits(p_all[:nb])[np.arange(nb), act], bits[3]), "mi_rb_forward's distribution of the stored action is not the gradient launch's probs"
    if c["noisy"]:                                                     # the target network's q at obs[s_m] under ITS sample, through the same forward kernel
        teng = _engine(dev, dict(c, params=c["target"]))
        got["q_target"] = _np(teng.forward(obs[nb:], noise=(c["u"], 1, Z.STREAM_LEARN))).astype(np.float64)
    else:
        got["q_target"] = _np(_engine(dev, dict(c, params=c["target"])).forward(obs[nb:])).astype(np.float64)
    fig = Z.figures(e, got)
    print(c["name"], fam, {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=c["mb"], n_step=c["n_step"]))
    assert set(fig) == set(Z.FIGURES)
    assert not Z.within(fig, fam), (c["name"], Z.within(fig, fam))
    assert (got["prio"] >= 0).all() and np.abs(_np(eng.target_probs).sum(axis=1) - 1).max() < 1e-5
    g32 = _np(eng.grads)
    if c["noisy"]:                                                     # slab[SIGMA + t] = g_t * eps_t: one product per slab; with one slab it is the product of the outputs
        if c["mb"] == 1:
            assert np.array_equal(g32[Z.SIGMA:], g32[Z.HEAD:Z.SIGMA] * e_on)        # (as values: the slab sum starts from +0, so a product of -0 arrives as +0)
    else:
        assert not g32[Z.SIGMA:].any() and np.array_equal(g32[Z.SIGMA:].view(np.uint32), np.zeros(Z.NHEAD, np.uint32))      # exact zeros, +0
    # mi_rb_update from fresh optimizer state: the same gradient bit for bit, parameters that are one Adam step on it
    step = _engine(dev, c)
    o = step.optimizer
    a = step.K.AdamArgs(step.K.ptr(o.exp_avg), step.K.ptr(o.exp_avg_sq), 1, Z.LR, Z.BETAS[0], Z.BETAS[1], Z.ADAM_EPS)
    step.K.update(step._ring, step._batch(0), a, step._s())
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "mi_rb_update's outputs are not mi_rb_grad's bits"
    p = c["params"].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    Z.adam_step(p, got["grads"], m, v, 1)
    after = _np(step.q.flat)
    assert np.abs(after - p).max() <= 1e-6                 # (the bound of tests/test_gpu_nstep_cases.py: a step of at most lr in f32, p - step rounded once)


def flat_actions(c):
    return c["actions"].reshape(-1)


@pytest.mark.parametrize("i", range(len(C.SPECS)), ids=C.NAMES)
def test_noisy_off_gives_exact_zeros_and_the_noisy_library_s_horizon(dev, i):
    """noisy = 0 on every ring, with a non-zero sigma in place: a sigma gradient of exact +0, the mean network's outputs (two runs with different update indices
    agree bit for bit), and the horizon mi_nz_grad writes on the same ring and indices"""
    import test_gpu_noisy_cases as TZ

    c = C.make_case(i)
    if not c["params"][Z.SIGMA:].any():                                # the sigma_0 rings: give the anchor a sigma it must ignore
        c = dict(c, params=np.concatenate([c["params"][:Z.SIGMA], Z.default_sigma()]), target=np.concatenate([c["target"][:Z.SIGMA], Z.default_sigma(2.0)]))
    eng = _engine(dev, c, noisy=False)
    eng.horizon.fill_(-7)
    _grad(eng)
    got, bits = _result(eng)
    assert np.array_equal(bits[0][Z.SIGMA:], np.zeros(Z.NHEAD, np.uint32)), "the sigma gradient is not exact zeros"
    other = _engine(dev, c, noisy=False)
    other.update_index = c["u"] + 5
    _grad(other)
    _, obits = _result(other)
    assert all(np.array_equal(a, b) for a, b in zip(bits, obits)), "noisy = 0 depends on the noise key"
    e = Z.evaluate(dict(c, noisy=0))
    assert np.array_equal(got["next_actions"], e["next_actions"]) or C.FAMILY_OF[c["name"]] != "off"     # (the off cases' conditions hold for the mean network)
    nz = TZ._engine(dev, NC.make_case(i), noisy=False)
    nz.horizon.fill_(-7)
    TZ._grad(nz)
    assert np.array_equal(_np(eng.horizon), _np(nz.horizon)), "horizon differs from mi_nz_grad's"


def test_the_device_draw(dev):
    """the sample as the kernels form it against the restatement; 4,096 numbers' moments; different keys, different samples"""
    seed = 20182
    xs, fins, fouts = zip(*[device_sample(dev, seed, u, 0, Z.STREAM_LEARN) for u in range(13)])
    xs = np.array(xs)
    z64 = Z.normal(seed, np.arange(13), 0, Z.STREAM_LEARN, np.float64)
    d = float(np.abs(xs * np.abs(xs) - z64).max())
    print("device draw: xi |xi| against float64 z: %.3g (bound %.3g)" % (d, Z.BOUND_DRAW["z"]))
    record("draw", dict(z=d, samples=13 * 321))
    assert d <= Z.BOUND_DRAW["z"]
    assert np.array_equal(np.sign(xs), np.sign(z64))
    for x, fin, fout in zip(xs, fins, fouts):                          # the factors over the rows, bit for bit: value rows, then a * 51 + j
        rfin, rfout = Z.factors(x)
        assert np.array_equal(fin.view(np.uint32), rfin.view(np.uint32)) and np.array_equal(fout.view(np.uint32), rfout.view(np.uint32))
    # 4,096 numbers: 13 samples of 321 are 4,173; the first 4,096 of them
    z = (xs * np.abs(xs)).astype(np.float64).reshape(-1)[:4096]
    assert abs(z.mean()) <= 5 / np.sqrt(4096) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / 4096)
    act = device_sample(dev, seed, 0, 0, Z.STREAM_ACT)[0]
    tgt = device_sample(dev, seed, 0, 1, Z.STREAM_LEARN)[0]
    other_seed = device_sample(dev, seed + 1, 0, 0, Z.STREAM_LEARN)[0]
    far = device_sample(dev, seed, (1 << 40) + 3, (1 << 33) + 9, Z.STREAM_ACT)[0]
    for o in (act, tgt, other_seed, xs[1]):
        assert not np.array_equal(o, xs[0]) and abs(np.corrcoef(o, xs[0])[0, 1]) < 0.3
    assert np.abs(far * np.abs(far) - Z.normal(seed, (1 << 40) + 3, (1 << 33) + 9, Z.STREAM_ACT, np.float64)).max() <= Z.BOUND_DRAW["z"]      # 64-bit keys reach the counter
    assert np.abs(act * np.abs(act) - Z.normal(seed, 0, 0, Z.STREAM_ACT, np.float64)).max() <= Z.BOUND_DRAW["z"]


def test_update_is_bitwise_grad_plus_adam_over_four_updates(dev):
    """uniform mode, n_step 3, on the CPU-built ring of the chained tests: mi_rb_update (in-launch index draw, Adam on the slab sum of all 36,774 elements) against
    sample() + grad() + deep_rl_amd.Adam.step over 4 updates with a target sync between them; every update draws new samples; the same four once more give the
    same bits"""
    from oracle import cpu_ref as R
    R.lib().ref_set_num_threads(8)
    ring, _, _, params, target, _ = Z.chain_data(R)

    def engine():
        eng = make_engine(dev, 1, Z.CHAIN_STEPS + 1, params=params, target=target, seed=Z.CHAIN_SEED, batch_size=Z.CHAIN_BATCH, prioritized=False, n_step=Z.CHAIN_N,
                          support=Z.CHAIN_SUPPORT)
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
                     (a.target_probs, b.target_probs), (a.probs, b.probs), (a.prio, b.prio), (a.next_actions, b.next_actions), (a.horizon, b.horizon)):
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
