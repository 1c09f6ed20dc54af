"""The IQN kernels on the synthetic cases of tests/_iqn_ref.py (validated on the CPU by tests/test_iqn_cases_cpu.py) against float64: terminated rows, successors
across the ring's end, several envs, batches of 1, 5, 33, 32 and 70 rows (the last walks two rows in some workgroups: MI_IQN_MAX_SLABS is 64); the loss stage alone
at its edges against exact values; acting at 4,096 envs against single-env engines; checkpoint save / load.  Bounds: those of tests/_iqn_ref.py (8 x the f32
restatement's measured distance from the reference and from float64); nothing is excluded from a loss or gradient comparison."""
import numpy as np
import pytest

import _iqn_ref as R

pytestmark = pytest.mark.gpu
_REF = {}


def _case(i):
    if i not in _REF:
        shp = R.CASES[i]
        c = R.make_case(*shp, R.CASE_SEEDS[shp])
        _REF[i] = (c, R.update(c["params"], c["target_params"], c["ring"], c["inds"], c["taus"], c["next_taus"], c["tau_dashes"], dtype=np.float64))
    return _REF[i]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_update_on_a_synthetic_case_against_float64(i):
    import _iqn_gpu as G
    (batch, envs, slots), (c, r) = R.CASES[i], _case(i)
    eng = G.make_engine(c["params"], c["target_params"], num_envs=envs, slots=slots, batch_size=batch, ringv=c["ring"])
    eng.global_step = slots
    out = G.run_grad(eng, c["inds"], c["taus"], c["next_taus"], c["tau_dashes"])
    close = np.abs(r["q_next"][:, 1] - r["q_next"][:, 0]) < R.CLOSE_Q
    assert close.sum() <= 1 and np.array_equal(out["next_actions"][~close], r["next_actions"][~close])
    assert np.array_equal(out["next_actions"], r["next_actions"])   # the seeds leave no close row
    scale = max(np.abs(r["current"]).max(), np.abs(r["target"]).max())
    fig = dict(current=np.abs(out["current"] - r["current"]).max(), target=np.abs(out["target"] - r["target"]).max(),
               loss=abs(out["loss"] - r["loss"]) / abs(r["loss"]), grad=np.abs(out["grads"] - r["grads"]).max() / np.abs(r["grads"]).max())
    print("case", R.CASES[i], {k: float(v) for k, v in fig.items()}, "scale", float(scale))
    G.record("case_quantiles_rel", max(fig["current"], fig["target"]) / scale); G.record("case_loss_rel", fig["loss"]); G.record("case_grad_rel", fig["grad"])
    assert np.array_equal(out["taus"], c["taus"])
    assert max(fig["current"], fig["target"]) <= R.BOUND_QUANT_REL * max(1.0, scale)
    assert fig["loss"] <= R.BOUND_LOSS_REL and fig["grad"] <= R.BOUND_GRAD_REL
    per_tensor = R.tensor_grad_errors(out["grads"], r["grads"])   # each tensor against its own largest element
    print("   per tensor", {k: float("%.2g" % v) for k, v in per_tensor.items()})
    G.record("case_grad_tensor_rel", max(per_tensor.values()))
    assert max(per_tensor.values()) <= R.BOUND_GRAD_TENSOR_REL, per_tensor
    # the fused call on the same batch steps the parameters by Adam on exactly this gradient
    p0 = c["params"].copy(); m = np.zeros_like(p0); v = np.zeros_like(p0)
    R.adam_step(p0, out["grads"], m, v, 1, eps=0.01 / batch)   # the engine's Adam: eps = 1e-2 / batch_size
    eng.train_step(c["inds"])
    assert np.array_equal(eng.grads.cpu().numpy(), out["grads"]) and np.abs(eng.q.flat.cpu().numpy() - p0).max() <= R.BOUND_PARAM_ABS


def _huber(cur, tgt, tau):
    import torch
    from deep_rl_amd import _native_iqn as K
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    c, g, u = t(cur), t(tgt), t(tau)
    loss = torch.zeros(1, dtype=torch.float32, device=dev); d = torch.zeros_like(c)
    K.check(K.lib().mi_iqn_quantile_huber(K.ptr(c), K.ptr(g), K.ptr(u), c.shape[0], K.ptr(loss), K.ptr(d), K.stream_ptr(dev)), "mi_iqn_quantile_huber")
    torch.cuda.synchronize()
    return float(loss.item()), d.cpu().numpy()


def test_quantile_huber_edges_against_exact_values():
    """delta exactly +-kappa (the quadratic branch: value 1, slope +-2), +-0 (value 0, slope 0, indicator 0 for both zeros), just beyond kappa (the linear branch:
    value |d| - 1/2, slope +-1), tau at 0 and at 1 - 2^-24.  All inputs are dyadic, so the float64 values are exact and the f32 loss stage reproduces the
    per-element terms exactly; only the summation rounds."""
    f32 = np.float32
    B = 2
    cur = np.zeros((B, 64), f32)
    tgt = np.zeros((B, 64), f32)
    edge = np.array([1.0, -1.0, 0.0, -0.0, np.nextafter(f32(1), f32(2)), -np.nextafter(f32(1), f32(2)), 0.5, -0.5, 3.0, -3.0, 0.25, 1.5, -1.5, 2.0, -2.0, 0.75], f32)
    tgt[0] = np.tile(edge, 4)
    tgt[1] = np.tile(edge[::-1], 4)
    cur[1] = f32(0.5)
    tau = np.zeros((B, 64), f32)
    tau[:, 0::4] = 0.0; tau[:, 1::4] = f32(1.0 - 2.0 ** -24); tau[:, 2::4] = 0.5; tau[:, 3::4] = 0.25
    loss, d = _huber(cur, tgt, tau)
    l64, d64, _ = R.quantile_huber(cur, tgt, tau, np.float64)
    l32, d32, _ = R.quantile_huber(cur, tgt, tau, np.float32)
    assert loss == float(l32) and np.array_equal(d, d32)          # no fma, no transcendental: the restated order gives the same bits
    assert abs(loss - l64) <= 64 * 2.0 ** -24 * abs(l64) and np.abs(d - d64).max() <= 64 * 2.0 ** -24 * np.abs(d64).max()   # 64-term f32 sums of exact terms
    # spot values: row 0 (current 0), tau_0 = 0: delta = +1 -> w = 0; tau_1 = 1 - 2^-24 with delta_j over the 16 edges
    delta = tgt[0].astype(np.float64)
    w = np.abs(float(tau[0, 1]) - (delta < 0))
    hub = np.where(np.abs(delta) <= 1, delta * delta, np.abs(delta) - 0.5)
    grd = np.where(np.abs(delta) <= 1, 2 * delta, np.sign(delta))
    assert abs(d[0, 1] - (-(w * grd).sum() / (B * 64))) <= 1e-6 and (w * hub).sum() > 0


def test_quantile_huber_fully_terminated_batch():
    """every row terminated: target_j = reward for all j, so delta_ij = 1 - current_i independent of j"""
    rng = np.random.default_rng(5)
    cur = rng.uniform(-2, 3, size=(5, 64)).astype(np.float32)
    tgt = np.ones((5, 64), np.float32)
    tau = (rng.integers(0, 1 << 24, size=(5, 64)) / float(1 << 24)).astype(np.float32)
    loss, d = _huber(cur, tgt, tau)
    l64, d64, _ = R.quantile_huber(cur, tgt, tau, np.float64)
    assert abs(loss - l64) <= R.BOUND_LOSS_REL * abs(l64) and np.abs(d - d64).max() <= R.BOUND_GRAD_REL * np.abs(d64).max()


def test_fully_terminated_batch_through_the_engine():
    import _iqn_gpu as G
    c = R.make_case(5, 3, 7, R.CASE_SEEDS[(5, 3, 7)])
    obs, actions, rewards, term = c["ring"]
    eng = G.make_engine(c["params"], c["target_params"], num_envs=3, slots=7, batch_size=5, ringv=(obs, actions, rewards, np.ones_like(term)))
    out = G.run_grad(eng, c["inds"], c["taus"], c["next_taus"], c["tau_dashes"])
    assert np.array_equal(out["target"], np.ones((5, 64), np.float32))


def _episode_figures(term):
    ends = np.flatnonzero(term)
    lens = np.diff(np.concatenate([[-1], ends]))
    return len(ends), int(lens.sum()), int(lens.max()) if len(ends) else 0


def test_acting_at_4096_envs_matches_single_env_engines():
    """4,096 envs share 1,024 workgroups (each walks four envs); spot-checked envs act exactly as N = 1 engines keyed with their ids, and the launch's episode
    statistics are the sums over the envs of what the ring itself shows.  32 steps from fresh episodes behind learning_starts at epsilon ~ 0.5: both branches run."""
    import _iqn_gpu as G
    p = R.load_ckpt(int(R.load_trace()["checkpoints"][-1]))["params_before"]
    S, T, g0 = 34, 32, 5_000
    kw = dict(slots=S, learning_starts=1_000)
    big = G.make_engine(p, p, num_envs=4096, **kw)
    big.global_step = g0
    big.reset()
    big.act(T)
    _np = lambda t: t.cpu().numpy()   # noqa: E731
    A, O, Tm = _np(big.actions), _np(big.observations), _np(big.terminated)
    term = Tm[(g0 + 1 + np.arange(T)) % S]
    per_env = np.array([_episode_figures(term[:, E]) for E in range(4096)])
    for E in (0, 1023, 1024, 4095):
        one = G.make_engine(p, p, num_envs=1, env_id_base=E, **kw)
        one.global_step = g0
        one.reset()
        one.act(T)
        assert np.array_equal(_np(one.actions)[:, 0], A[:, E]) and np.array_equal(_np(one.observations)[:, 0], O[:, E])
        assert _np(one.episode_stats)[:3].tolist() == per_env[E].tolist()
    st = _np(big.episode_stats).tolist()
    assert per_env[:, 0].sum() >= 400
    assert st[:3] == [int(per_env[:, 0].sum()), int(per_env[:, 1].sum()), int(per_env[:, 2].max())] and st[3] == 0
    assert big.global_step == g0 + T


def test_checkpoint_save_load_continue_equals_the_uninterrupted_run(tmp_path):
    import _iqn_gpu as G
    import deep_rl_amd.checkpoint as ckpt
    p = R.load_trace()["init_params"]
    kw = dict(num_envs=2, slots=40, batch_size=8, learning_starts=8)

    def steps(eng, k):
        for _ in range(k):
            eng.act(4)
            eng.train_step()
            if eng.global_step % 16 == 0:
                eng.sync_target()

    a = G.make_engine(p, p, **kw); a.reset(); steps(a, 12)
    b = G.make_engine(p, p, **kw); b.reset(); steps(b, 5)
    path = ckpt.save(str(tmp_path / "iqn"), b)
    c = G.make_engine(p * 0, p * 0, **kw)
    ckpt.load(path, c)
    steps(c, 7)
    _np = lambda t: t.cpu().numpy()   # noqa: E731
    assert np.array_equal(_np(a.q.flat), _np(c.q.flat)) and np.array_equal(_np(a.target_network.flat), _np(c.target_network.flat))
    assert np.array_equal(_np(a.observations), _np(c.observations)) and np.array_equal(_np(a.actions), _np(c.actions))
    assert np.array_equal(_np(a.optimizer.exp_avg_sq), _np(c.optimizer.exp_avg_sq)) and a.global_step == c.global_step
