"""libmirl_iqn.so against the fixtures captured from the reference's own statements (tests/golden/iqn_ref_*.npz, tools/capture_iqn_ref.py): forward, targets and
gradient at the checkpoints, the 21 chained updates teacher-forced with the reference's indices and taus, the fused update against grad + Adam bit for bit,
repeatability, the production Philox draws against their restatement, and argument errors.  Bounds: tests/_iqn_ref.py (8 x the f32 restatement's measured
distance); the device's observed maxima go to iqn_gpu_maxima.json in the results directory."""
import ctypes as C

import numpy as np
import pytest

import _iqn_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trace():
    return R.load_trace()


def _np(t):
    return t.detach().cpu().numpy()


def _engine(trace, params, target_params, **kw):
    import _iqn_gpu as G
    ringv = R.ring(trace)
    return G.make_engine(params, target_params, num_envs=1, slots=len(ringv[1]), batch_size=int(trace["hparams"][5]), ringv=ringv, **kw)


def test_acting_forwards_of_the_reference(trace):
    import torch
    import _iqn_gpu as G
    import deep_rl_amd as M
    p = torch.from_numpy(trace["act_params"]).cuda()
    quant, q = M.iqn_forward(p, torch.from_numpy(trace["act_obs"]), torch.from_numpy(trace["act_taus"]))
    scale = float(np.abs(trace["act_quantiles"]).max())
    eq, ea = np.abs(_np(quant) - trace["act_quantiles"]).max(), np.abs(_np(q) - trace["act_q"]).max()
    print("acting forwards: quantiles %.3g (max |quantile| %.1f), q %.3g" % (eq, scale, ea))
    G.record("fixture_act_quantiles_rel", eq / scale); G.record("fixture_act_q_abs", ea)
    assert eq <= R.BOUND_QUANT_REL * scale and ea <= R.BOUND_Q_ABS
    assert np.array_equal((_np(q)[:, 1] > _np(q)[:, 0]).astype(np.int32), trace["act_action"])


@pytest.mark.parametrize("j", range(4))
def test_forward_target_grad_at_a_fixture_checkpoint(trace, j):
    import _iqn_gpu as G
    c = R.load_ckpt(int(trace["checkpoints"][j]))
    eng = _engine(trace, c["params_before"], c["target_params"])
    # the target stage alone, then the whole gradient
    eng.sample(c["batch_inds"]); eng.force_taus(c["taus"], c["next_taus"], c["tau_dashes"])
    eng.target()
    tgt_alone, na_alone = _np(eng.target_action_quantiles).copy(), _np(eng.next_actions).copy()
    out = G.run_grad(eng, c["batch_inds"], c["taus"], c["next_taus"], c["tau_dashes"])
    assert np.array_equal(out["target"], tgt_alone) and np.array_equal(out["next_actions"], na_alone)
    assert np.array_equal(out["next_actions"], c["next_actions"])
    scale = max(np.abs(c["current_action_quantiles"]).max(), np.abs(c["target_action_quantiles"]).max())
    fig = dict(quant=max(np.abs(out["current"] - c["current_action_quantiles"]).max(), np.abs(out["target"] - c["target_action_quantiles"]).max()) / scale,
               loss=abs(out["loss"] - float(c["loss"][0])) / float(c["loss"][0]), grad=np.abs(out["grads"] - c["grads"]).max() / np.abs(c["grads"]).max())
    print("checkpoint", int(c["update"][0]), {k: float(v) for k, v in fig.items()})
    G.record("fixture_quantiles_rel", fig["quant"]); G.record("fixture_loss_rel", fig["loss"]); G.record("fixture_grad_rel", fig["grad"])
    assert fig["quant"] <= R.BOUND_QUANT_REL and fig["loss"] <= R.BOUND_LOSS_REL and fig["grad"] <= R.BOUND_GRAD_REL   # every element, nothing left out
    per_tensor = R.tensor_grad_errors(out["grads"], c["grads"])   # each tensor against its own largest element: the extractor's gradients are not hidden behind the head's
    print("   per tensor", {k: float("%.2g" % v) for k, v in per_tensor.items()})
    G.record("fixture_grad_tensor_rel", max(per_tensor.values()))
    assert max(per_tensor.values()) <= R.BOUND_GRAD_TENSOR_REL, per_tensor


def test_chained_updates_teacher_forced_land_on_the_references_parameters(trace):
    """21 updates with the reference's indices and taus from the window's start (parameters, target, Adam moments and step count), the target sync behind the
    11th: the parameters stay within the parameter bound (8 x the restatement's own 21-step distance) of the reference's at every checkpoint, all 21 losses within
    the loss bound plus the fixture's explicit allowance for td errors inside the kappa margin"""
    import torch
    import _iqn_gpu as G
    st = R.load_start()
    eng = _engine(trace, st["params"], st["target_params"])
    o = eng.optimizer
    o.exp_avg.copy_(torch.from_numpy(st["exp_avg"])); o.exp_avg_sq.copy_(torch.from_numpy(st["exp_avg_sq"])); o.step_count = int(trace["start_adam_step"][0])
    after = {int(k): R.load_ckpt(int(k))["params_after"] for k in trace["checkpoints"]}
    worst_p, worst_l = 0.0, 0.0
    for k in range(21):
        eng.force_taus(trace["taus"][k], trace["next_taus"][k], trace["tau_dashes"][k])
        eng.train_step(trace["batch_inds"][k])
        # every update's loss: the bound plus what the td errors the fixture names inside the kappa margin could move it by (0 at the checkpoints)
        excess = abs(float(eng.loss.item()) - trace["loss"][k]) - trace["flip_allowance"][k]
        worst_l = max(worst_l, excess / trace["loss"][k])
        if k in after:
            worst_p = max(worst_p, float(np.abs(_np(eng.q.flat) - after[k]).max()))
        if k in trace["sync_after_update"]:
            eng.sync_target()
    print("chained updates: max |p - reference| %.3g, max loss error %.3g" % (worst_p, worst_l))
    G.record("chained_param_abs", worst_p); G.record("chained_loss_rel", worst_l)
    assert worst_p <= R.BOUND_PARAM_ABS and worst_l <= R.BOUND_LOSS_REL
    assert o.step_count == int(trace["start_adam_step"][0]) + 21


def _four_updates(trace, fused):
    """four updates with production draws (indices and taus from the kernels' own streams), a target sync between the second and the third"""
    st = R.load_start()
    eng = _engine(trace, st["params"], st["target_params"], seed=11)
    eng.global_step = 500
    if not fused:
        eng.optimizer = _UnfusedAdam(eng.q.flat)   # any optimizer but deep_rl_amd.Adam itself takes the unfused path; this one steps with libmirl's mi_adam
    rec = []
    for k in range(4):
        eng.train_step()
        rec.append((_np(eng.q.flat).copy(), _np(eng.grads).copy(), float(eng.loss.item()), _np(eng.batch_inds).copy(), _np(eng.taus).copy(),
                    _np(eng.target_action_quantiles).copy()))
        if k == 1:
            eng.sync_target()
    return eng, rec


class _UnfusedAdam:
    """deep_rl_amd.Adam behind a different type: IQNEngine.train_step then takes sample() + grad() + optimizer.step()"""

    def __init__(self, flat):
        import deep_rl_amd as M
        self._a = M.Adam(flat, lr=5e-5, eps=1e-2 / 8)

    def step(self, grads):
        self._a.step(grads)


def test_update_equals_grad_plus_adam_bitwise_and_repeats(trace):
    _e1, fused = _four_updates(trace, True)
    _e2, again = _four_updates(trace, True)
    _e3, unfused = _four_updates(trace, False)
    for a, b, c in zip(fused, again, unfused):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y), "a repeated run gives other bits"
            assert np.array_equal(x, z), "mi_iqn_update differs from mi_iqn_grad + mi_adam"
    assert not np.array_equal(fused[0][0], fused[3][0])


def test_production_draws_equal_the_restated_philox_draws(trace):
    """indices (stream 4) and the three tau draws (streams 10 / 11 / 12) of an update, bit for bit; next_taus and tau_dashes through the targets they produce"""
    eng, rec = _four_updates(trace, True)
    ringv = R.ring(trace)
    upper = min(500, eng.slots) * 1
    B = eng.batch_size
    for k, (_p, _g, _l, inds, taus, tgt) in enumerate(rec):
        assert np.array_equal(inds, R.index_draws(11, k, B, upper))
        assert np.array_equal(taus, R.tau_draws(11, k, np.arange(B), 64, 10))
    # the targets of update 3 from the restated next_taus / tau_dashes (float64 on the device's inputs): within the quantile bound, i.e. the same taus
    k = 3
    tp = rec[1][0]                                   # the sync behind update 1 copied these parameters
    X, A, Xn, Rw, T = R.batch_of(ringv, rec[k][3])
    na, tg, _q = R.target(tp, Xn, Rw, T, R.tau_draws(11, k, np.arange(B), 32, 11), R.tau_draws(11, k, np.arange(B), 64, 12), dtype=np.float64)
    scale = np.abs(tg).max()
    assert np.abs(rec[k][5] - tg).max() <= R.BOUND_QUANT_REL * scale and np.array_equal(na, eng.next_actions.cpu().numpy())


def test_acting_taus_equal_the_restated_philox_draws(trace):
    """the taus of greedy steps (stream 9, env n, idx = step counter * 8 + m, word w = tau 4 m + w) as the acting launch reports them through taus_out, bit for bit,
    over three steps of three envs; and the action each step stores is the argmax of the forward at exactly those taus"""
    import torch
    import _iqn_gpu as G
    import deep_rl_amd as M
    p = R.load_ckpt(int(trace["checkpoints"][-1]))["params_after"]
    eng = G.make_engine(p, p, num_envs=3, slots=16, seed=5, learning_starts=0, final_epsilon=0.0, epsilon_decay_steps=1)
    eng.global_step = 10                      # epsilon = max(1 - 10, 0) = 0: every step is greedy
    obs = [_np(eng.reset()).copy()]
    out = torch.full((3, 3, 32), -1.0, dtype=torch.float32, device="cuda")
    for s in range(3):                        # one step per launch, so that the observation before every step is known
        eng.act(1, taus_out=out[s:s + 1])
        obs.append(_np(eng.observation).copy())
    taus = _np(out)
    for s in range(3):
        want = np.stack([R.tau_draws(5, n, [s], 32, 9, base=8)[0] for n in range(3)])   # the env step counter is s: fresh envs, one draw per step
        assert np.array_equal(taus[s].view(np.uint32), want.view(np.uint32)), s
        _quant, q = M.iqn_forward(eng.q.flat, torch.from_numpy(obs[s]), torch.from_numpy(want))
        q = _np(q)
        far = np.abs(q[:, 1] - q[:, 0]) > R.CLOSE_Q
        assert np.array_equal(_np(eng.actions)[(10 + s) % 16][far], (q[:, 1] > q[:, 0]).astype(np.int64)[far])
    # exploring steps leave their rows untouched
    eng2 = G.make_engine(p, p, num_envs=3, slots=16, seed=5, learning_starts=100)
    eng2.reset()
    out2 = torch.full((2, 3, 32), -1.0, dtype=torch.float32, device="cuda")
    eng2.act(2, taus_out=out2)
    assert float(out2.max()) == -1.0


def test_bad_arguments_return_einval(trace):
    import torch
    from deep_rl_amd import _native_iqn as K
    st = R.load_start()
    eng = _engine(trace, st["params"], st["target_params"])
    L, s = K.lib(), K.stream_ptr(eng.device)
    obs = torch.zeros((2, 4), device="cuda"); taus = torch.zeros((2, 8), device="cuda"); out = torch.zeros((2, 8, 2), device="cuda")
    assert L.mi_iqn_forward(K.ptr(eng.q.flat), K.ptr(obs), K.ptr(taus), 2, 65, K.ptr(out), None, s) == K.MI_IQN_EINVAL
    assert L.mi_iqn_forward(K.ptr(eng.q.flat), K.ptr(obs), K.ptr(taus), 2, 8, None, None, s) == K.MI_IQN_EINVAL
    assert L.mi_iqn_forward(K.ptr(eng.q.flat) + 4, K.ptr(obs), K.ptr(taus), 2, 8, K.ptr(out), None, s) == K.MI_IQN_EINVAL   # misaligned parameters
    b = eng._batch(0)
    b.batch = 0
    assert L.mi_iqn_grad(C.byref(eng._ring), C.byref(b), s) == K.MI_IQN_EINVAL
    b = eng._batch(eng.slots + 1)
    assert L.mi_iqn_grad(C.byref(eng._ring), C.byref(b), s) == K.MI_IQN_EINVAL and "sample_upper" in L.mi_iqn_last_error().decode()
    b = eng._batch(0)
    b.workspace = None
    assert L.mi_iqn_update(C.byref(eng._ring), C.byref(b), None, s) == K.MI_IQN_EINVAL
    a = K.IQNAct(K.ptr(eng.q.flat), None, None, None, None, None, None, None, 0, 0, -1e-4, 0.01, 65, 0)
    assert L.mi_iqn_act_steps(eng.env.handle, C.byref(eng._ring), C.byref(a), s) == K.MI_IQN_EINVAL
    with pytest.raises(K.MiError):
        eng.sample(np.arange(5))
    torch.cuda.synchronize()
