"""REINFORCE on the MI355X (libmirl_pg.so, include/mi_reinforce.h) against the unmodified reference (tests/golden/reinforce_ref_trace.npz) and the numpy
restatement (tests/_reinforce_ref.py).

Tolerances.  The fixture is the reference's own f32 evaluation; the restatement and the device are two more f32 evaluations in other summation orders (the device
adds hardware exp / log at ~1 ulp).  tests/test_reinforce_ref_pinned_cpu.py measures the restatement against the fixture over all 100 updates: gradient
4.4e-7 of max |g|, log-probs 7.2e-7, normalised returns 7.2e-7 absolute, Adam chained on reference gradients 2.4e-7 (1.8e-7 here).  The device bounds are 8 x those
figures.  Gradient and optimizer are tested SEPARATELY, each from reference inputs: chaining them is ill-conditioned for this script.
Observed maxima are written to reinforce_gpu_maxima.json in the tests' results directory (_reinforce_ref.results_dir) and recorded in docs/LEDGER.md."""
import json
import os

import numpy as np
import pytest

import _reinforce_ref as P
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

GRAD_BOUND = 8 * 4.4e-7      # of max |g|
LP_BOUND = 8 * 7.2e-7        # absolute; also the probability bound of the draw check
RN_BOUND = 8 * 7.2e-7        # absolute
ADAM_BOUND = 8 * 2.4e-7      # absolute, 100 chained steps


def _record(key, value):
    path = os.path.join(P.results_dir(), "reinforce_gpu_maxima.json")
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec[key] = value
    json.dump(rec, open(path, "w"), indent=1)
    print(key, json.dumps(value))


def _make(n, seed=1, env_id_base=0, params=None):
    import torch

    import deep_rl_amd as D

    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=env_id_base)
    torch.manual_seed(seed)
    agent = D.DropoutPolicy(env)
    if params is not None:
        agent.load_flat(params)
    opt = D.Adam(agent, lr=1e-2)
    return D.ReinforceEngine(env, agent, opt)


def _np(t):
    return t.detach().cpu().numpy()


def _device_rows(eng):
    """-> per env (X, A, M, log_probs, b_returns) of the valid rows of the last rollout"""
    lens = _np(eng.lengths)
    obs, act, mb, lp, rn = _np(eng.observations), _np(eng.actions), _np(eng.mask_bits), _np(eng.log_probs), _np(eng.b_returns)
    return lens, [(obs[n, :lens[n]], act[n, :lens[n]].astype(np.int64), P.words_to_masks(mb[n, :lens[n]]), lp[n, :lens[n]], rn[n, :lens[n]]) for n in range(len(lens))]


def _restated_grad(rows, params, dtype=np.float64):
    g = np.zeros(898, np.float64)
    for X, A, M, _lp, _rn in rows:
        _, Rn = P.returns_normalised(len(A))
        g += P.grad(params, X, A, M, Rn, dtype).astype(np.float64)
    return g


def test_initial_weights_are_the_references():
    t = P.load_trace()
    eng = _make(1)
    assert np.array_equal(_np(eng.agent.flat), t["init_params"])
    shapes = [tuple(p.shape) for p in eng.agent.parameters()]
    assert shapes == [(128, 4), (128,), (2, 128), (2,)]


def test_teacher_forced_reference_run():
    """all 100 reference episodes: forced reset state, actions and masks, the reference's parameters before each update"""
    import torch

    t = P.load_trace()
    eng = _make(1)
    worst = dict(lp=0.0, rn=0.0, grad=0.0, grad_vs_cpu32=0.0)
    steps = 0
    R.set_sincos_mode("fdlibm")
    try:
        for e in range(100):
            ep = P.episode(t, e)
            n = ep["length"]
            eng.agent.load_flat(ep["params"])
            fa = np.zeros((1, 500), np.int32); fa[0, :n] = ep["A"]
            fm = np.zeros((1, 500, 4), np.uint32); fm[0, :n] = ep["W"]
            eng.rollout(torch.from_numpy(ep["reset"][None]), torch.from_numpy(fa), torch.from_numpy(fm.view(np.int32)))
            eng.compute_returns()
            eng.grad()
            assert int(eng.lengths[0]) == n == int(eng.episodic_returns[0])
            obs = _np(eng.observations[0])
            assert np.array_equal(obs[0], ep["X"][0]) and np.array_equal(obs[1:n + 1], ep["obs_after"])           # the fixture, no step left out
            o_obs, o_term, o_done, _tr = P.replay_episode(ep["reset"], ep["A"])
            assert len(o_obs) == n and o_done[-1] and np.array_equal(obs[1:n + 1], o_obs)                           # the oracle stepper, device-matched mode
            assert np.array_equal(o_term, ep["terminated"].astype(bool))
            assert np.array_equal(_np(eng.actions[0, :n]), ep["A"]) and np.array_equal(_np(eng.mask_bits[0, :n]).view(np.uint32), ep["W"])
            worst["lp"] = max(worst["lp"], float(np.abs(_np(eng.log_probs[0, :n]) - ep["b_log_probs"]).max()))
            worst["rn"] = max(worst["rn"], float(np.abs(_np(eng.b_returns[0, :n]) - ep["b_returns"]).max()))
            assert float(eng.log_probs[0, n:].abs().max()) == 0.0 and float(eng.returns[0, n:].abs().max()) == 0.0 and float(eng.b_returns[0, n:].abs().max()) == 0.0
            scale = float(np.abs(ep["grads"]).max())
            g = _np(eng.grads)
            err = float(np.abs(g - ep["grads"]).max()) / scale
            cpu = float(np.abs(P.grad(ep["params"], ep["X"], ep["A"], ep["M"], ep["b_returns"]) - ep["grads"]).max()) / scale
            worst["grad"] = max(worst["grad"], err)
            worst["grad_vs_cpu32"] = max(worst["grad_vs_cpu32"], err / cpu)
            steps += n
    finally:
        R.set_sincos_mode("libm")
    assert steps == 7706
    _record("teacher_forced", worst)
    assert worst["lp"] <= LP_BOUND, worst
    assert worst["rn"] <= RN_BOUND, worst
    assert worst["grad"] <= GRAD_BOUND, worst
    assert worst["grad_vs_cpu32"] <= 8.0, worst      # and update by update: at most 8 x the f32 restatement's error on the same update


def test_adam_on_the_references_gradient_sequence():
    import torch

    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_pg as PG

    t = P.load_trace()
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(t["init_params"].copy()).to(dev); m = torch.zeros_like(p); v = torch.zeros_like(p)
    rp = t["init_params"].copy(); rm = np.zeros_like(rp); rv = np.zeros_like(rp)
    worst = worst_fixture = 0.0
    for e in range(100):
        g = torch.from_numpy(t["grads"][e]).to(dev)
        PG.check(PG.lib().mi_pg_adam(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), 898, e + 1, 1e-2, 0.9, 0.999, 1e-8, N.stream_ptr(dev)), "mi_pg_adam")
        P.adam_step(rp, t["grads"][e], rm, rv, e + 1)
        worst = max(worst, float(np.abs(_np(p) - rp).max()))
        worst_fixture = max(worst_fixture, float(np.abs(_np(p) - t["params_after"][e]).max()))
    _record("adam_chained", {"vs_restatement": worst, "vs_fixture": worst_fixture})
    assert worst <= ADAM_BOUND and worst_fixture <= ADAM_BOUND


@pytest.mark.parametrize("n", [1, 64, 4096])
def test_production_rng(n):
    seed = 3
    eng = _make(n, seed=seed)
    params = _np(eng.agent.flat).copy()
    eng.rollout(); eng.compute_returns(); eng.grad()
    lens, rows = _device_rows(eng)
    assert lens.min() >= 1 and lens.max() <= 500
    # masks: the keyed stream, bit for bit (first episode of every env: step counters start at 0)
    bits = kept = 0
    for e, (X, A, M, lp, rn) in enumerate(rows):
        assert np.array_equal(M, P.keyed_masks(seed, e, np.arange(lens[e]))), e
        bits += M.size; kept += int(M.sum())
    if n == 4096:
        assert bits >= 1_000_000
        assert abs(kept / bits - 0.4) < 5 * np.sqrt(0.24 / bits), (kept / bits, bits)
    # actions: the inverse-CDF draw on the device's own probabilities
    allX = np.concatenate([r[0] for r in rows]); allW = np.concatenate([_np(eng.mask_bits[e, :lens[e]]) for e in range(n)])
    import torch

    p0 = _np(eng.agent.forward(torch.from_numpy(allX), torch.from_numpy(allW)))[:, 0]
    u = np.concatenate([P.action_uniforms(seed, e, np.arange(lens[e])) for e in range(n)])
    a_dev = np.concatenate([r[1] for r in rows])
    differ = (u >= p0).astype(np.int64) != a_dev
    assert np.all(np.abs(u[differ] - p0[differ]) <= LP_BOUND), "an action differs from the draw away from the boundary"
    share = float(differ.mean())
    assert share < 1e-3
    # the device's log-probs are the restatement's at its own actions and masks
    pr, lpr, _h = P.forward(params, allX, np.concatenate([r[2] for r in rows]))
    lp_err = float(np.abs(lpr[np.arange(len(a_dev)), a_dev] - np.concatenate([r[3] for r in rows])).max())
    assert float(np.abs(pr[:, 0] - p0).max()) <= LP_BOUND and lp_err <= LP_BOUND
    # replay through the oracle stepper: keyed reset noise, the device's actions -> the device's lengths and observations
    R.set_sincos_mode("fdlibm")
    try:
        for e in (range(n) if n <= 64 else range(0, n, 16)):
            X, A = rows[e][0], rows[e][1]
            s0 = R.reset_noise(seed, e, 0)
            assert np.array_equal(X[0], s0.astype(np.float32))
            o_obs, _t, o_done, _tr = P.replay_episode(s0, A)
            assert len(o_obs) == lens[e] and o_done[-1], e
            assert np.array_equal(_np(eng.observations[e, 1:lens[e] + 1]), o_obs)
    finally:
        R.set_sincos_mode("libm")
    rn_err = max(float(np.abs(P.returns_normalised(len(r[1]))[1] - r[4]).max()) for r in rows)
    g_ref = _restated_grad(rows, params)
    g_err = float(np.abs(_np(eng.grads) - g_ref).max() / np.abs(g_ref).max())
    _record("production_rng_n%d" % n, {"rows": int(lens.sum()), "boundary_share": share, "probs_err": float(np.abs(pr[:, 0] - p0).max()), "log_prob_err": lp_err,
                                       "b_returns_err": rn_err, "grad_err_of_max": g_err, "keep_rate": kept / bits})
    assert rn_err <= RN_BOUND
    assert g_err <= GRAD_BOUND


def test_env_alone_is_env_inside_4096():
    big = _make(4096, seed=5)
    big.rollout()
    for e in (0, 1, 63, 64, 2049, 4095):
        one = _make(1, seed=5, env_id_base=e)
        one.rollout()
        n = int(one.lengths[0])
        assert n == int(big.lengths[e])
        for name in ("observations", "actions", "mask_bits", "log_probs"):
            a, b = _np(getattr(one, name)[0]), _np(getattr(big, name)[e])
            assert np.array_equal(a[:n + (1 if name == "observations" else 0)].view(np.uint32), b[:n + (1 if name == "observations" else 0)].view(np.uint32)), (e, name)


def _balancing_actions(reset, rule):
    """forced actions from a rule on the oracle's f64 state, until done"""
    env = R.VecCartPole(1, seed=1)
    env.reset(np.asarray(reset, np.float64).reshape(1, 4))
    acts = []
    while True:
        s = env.state[0].copy()
        a = rule(s)
        acts.append(a)
        _o, _r, d, tr, _fr, _fl = env.step(np.array([a]), forced_reset=np.zeros((1, 4)))
        if d[0]:
            return np.array(acts, np.int32), bool(tr[0])


def test_ragged_lengths_truncation_and_poisoned_storage():
    import torch

    n = 8
    resets = np.array([[0.01 * (i - 3), 0.0, 0.02 * ((i % 3) - 1), 0.0] for i in range(n)], np.float64)
    rules = [lambda s: int(s[2] + 0.5 * s[3] + 0.05 * s[0] + 0.1 * s[1] > 0)] * 2 + [lambda s: 0, lambda s: 1, lambda s: int(s[2] < 0)] + [lambda s: int(s[2] + 0.5 * s[3] > 0)] * 3
    R.set_sincos_mode("fdlibm")
    try:
        acts = [_balancing_actions(resets[i], rules[i]) for i in range(n)]
    finally:
        R.set_sincos_mode("libm")
    want = np.array([len(a) for a, _ in acts])
    assert want.max() == 500 and want.min() < 20 and any(tr for _, tr in acts)      # a truncated 500-step episode beside short ones in the same launch
    fa = np.zeros((n, 500), np.int32)
    for i, (a, _) in enumerate(acts):
        fa[i, :len(a)] = a
        fa[i, len(a):] = 1 - a[-1]            # whatever lies behind the end must never be read as a step
    eng = _make(n, seed=2)
    params = _np(eng.agent.flat).copy()
    POISON_I = 0x7FC0DEAD
    eng.actions.fill_(12345); eng.mask_bits.fill_(POISON_I); eng.observations.fill_(float("nan"))
    eng.rollout(torch.from_numpy(resets), torch.from_numpy(fa), None)
    eng.compute_returns(); eng.grad()
    lens, rows = _device_rows(eng)
    assert np.array_equal(lens, want)
    for i in range(n):
        L = int(lens[i])
        assert np.array_equal(rows[i][1], fa[i, :L])
        assert np.array_equal(rows[i][2], P.keyed_masks(2, i, np.arange(L)))
        # rows behind the end: log-probs / returns zero, everything else untouched (row L of the observations is the terminal observation)
        assert float(eng.log_probs[i, L:].abs().max()) == 0.0 and float(eng.returns[i, L:].abs().max()) == 0.0 and float(eng.b_returns[i, L:].abs().max()) == 0.0
        assert bool((eng.actions[i, L:] == 12345).all()) and bool((eng.mask_bits[i, L:] == POISON_I).all())
        assert bool(torch.isfinite(eng.observations[i, :L + 1]).all()) and (L == 500 or bool(torch.isnan(eng.observations[i, L + 1:]).all()))
    g = _np(eng.grads).copy()
    g_ref = _restated_grad(rows, params)
    err = float(np.abs(g - g_ref).max() / np.abs(g_ref).max())
    _record("ragged_truncation", {"lengths": lens.tolist(), "grad_err_of_max": err})
    assert np.isfinite(g).all() and err <= GRAD_BOUND
    # poison every row behind every episode's end (b_returns and log-probs too): the gradient must not move by a bit
    for i in range(n):
        L = int(lens[i])
        eng.observations[i, L:] = float("nan"); eng.b_returns[i, L:] = float("nan"); eng.log_probs[i, L:] = float("inf")
        eng.actions[i, L:] = -7; eng.mask_bits[i, L:] = -1
    eng.grad()
    assert np.array_equal(_np(eng.grads).view(np.uint32), g.view(np.uint32))


@pytest.mark.parametrize("n", [3, 4096])
def test_update_is_the_pieces_and_is_deterministic(n):
    import torch

    names = ("observations", "actions", "mask_bits", "log_probs", "returns", "b_returns", "lengths", "grads")

    def snapshot(eng):
        torch.cuda.synchronize()
        d = {k: _np(getattr(eng, k)).copy() for k in names}
        d.update(params=_np(eng.agent.flat).copy(), m=_np(eng.optimizer.exp_avg).copy(), v=_np(eng.optimizer.exp_avg_sq).copy())
        return d

    def same(a, b):
        for k in a:
            x, y = a[k], b[k]
            if k in ("observations", "actions", "mask_bits"):       # compare what the episodes wrote
                L = a["lengths"]
                x = np.concatenate([x[i, :L[i]].reshape(L[i], -1) for i in range(len(L))]); y = np.concatenate([y[i, :L[i]].reshape(L[i], -1) for i in range(len(L))])
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), k

    fused = _make(n, seed=7)
    for _ in range(3):
        fused.update()
    a = snapshot(fused)
    pieces = _make(n, seed=7)
    for _ in range(3):
        pieces.rollout(); pieces.compute_returns(); pieces.grad(); pieces.optimizer_step()      # Adam through libmirl.so's mi_adam
    same(a, snapshot(pieces))
    again = _make(n, seed=7)
    for _ in range(3):
        again.update()
    same(a, snapshot(again))
    assert fused.optimizer.step_count == pieces.optimizer.step_count == 3 and np.isfinite(a["params"]).all()
    assert not np.array_equal(a["params"], _np(_make(n, seed=7).agent.flat))


def test_checkpoint_resume_is_bit_exact(tmp_path):
    from deep_rl_amd import checkpoint

    full = _make(16, seed=4)
    for _ in range(5):
        full.update()
    first = _make(16, seed=4)
    for _ in range(2):
        first.update()
    path = checkpoint.save(str(tmp_path / "pg"), first)
    resumed = _make(16, seed=4)
    checkpoint.load(path, resumed)
    assert resumed.optimizer.step_count == 2 and resumed.update_index == 2
    for _ in range(3):
        resumed.update()
    for name in ("lengths", "log_probs", "b_returns", "grads"):
        assert np.array_equal(_np(getattr(full, name)).view(np.uint32), _np(getattr(resumed, name)).view(np.uint32)), name
    assert np.array_equal(_np(full.agent.flat).view(np.uint32), _np(resumed.agent.flat).view(np.uint32))
    assert np.array_equal(_np(full.optimizer.exp_avg_sq).view(np.uint32), _np(resumed.optimizer.exp_avg_sq).view(np.uint32))


def test_eval_mode_forward_matches_the_restatement():
    import torch

    eng = _make(1, seed=9)
    X = np.random.RandomState(0).uniform(-0.2, 0.2, (257, 4)).astype(np.float32)
    p = _np(eng.agent.forward(torch.from_numpy(X)))
    pr, _lp, _h = P.forward(_np(eng.agent.flat), X, None)
    assert p.shape == (257, 2) and float(np.abs(p - pr).max()) <= LP_BOUND and float(np.abs(p.sum(1) - 1).max()) < 1e-6
