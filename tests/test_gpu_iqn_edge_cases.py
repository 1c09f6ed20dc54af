"""iqn_grad_kernel, iqn_target_kernel, iqn_forward_kernel and iqn_reduce_kernel (deep_rl_amd/csrc/mi_iqn.hip; slab sum and row index of mi_ring.h) on the placed edge
cases of tests/_iqn_edge_cases.py (validated on the CPU by tests/test_iqn_edge_cases_cpu.py) against FLOAT64 AUTOGRAD, through IQNEngine with forced indices and
forced taus: every tail of the slab sum at <= 64 slabs and workgroups that walk two and three rows, a* that varies inside the batch and between the next_taus and the
tau_dashes, a target head that ties bit for bit, whole batches with lg == 0 and lg == gamma, gamma 0 and 1, d at exactly 0, +-kappa, one step to either side of
+-kappa and far out through the gradient launch, pre-activations of exactly 0 at all five ReLU sites, three dead layers, one stored action (either one), indices
outside the ring, taus at 0 and at 1 - 2^-24 and repeated taus; and mi_iqn_forward at K = 1 .. 64 and at one row more than its grid.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_iqn_edge_cases.BOUND = max(8 x the f32 restatement's measured distance from float64, the shipped bound of tests/_iqn_ref.py), per family and figure.  No case and
no row is excluded, action comparisons included.  Observed maxima go to iqn_edge_gpu_maxima.json in the tests' results directory (a copy: profiles/)."""
import json
import os

import numpy as np
import pytest

import _iqn_edge_cases as K
import _iqn_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    a = _np(t).copy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def record(key, value):
    path = os.path.join(R.results_dir(), "iqn_edge_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    if "family" in value:
        fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
        for k in K.FIGURES:
            fam[k] = max(fam.get(k, 0.0), value[k])
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _engine(c):
    import _iqn_gpu as G
    N, S = c["ring"]
    eng = G.make_engine(c["params"], c["target"], num_envs=N, slots=S, batch_size=c["mb"], ringv=K.ringv(c), gamma=c["gamma"], max_episodes_logged=0)
    eng.global_step = S                                    # min(global_step, slots) * N: every transition of the ring is stored
    eng.force_taus(c["taus"], c["next_taus"], c["tau_dashes"])
    return eng


def _result(eng):
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target=_np(eng.target_action_quantiles).astype(np.float64),
               current=_np(eng.current_action_quantiles).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64))
    return got, [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_action_quantiles), _bits(eng.current_action_quantiles), _bits(eng.next_actions)]


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(i):
    import torch
    from deep_rl_amd.agent import iqn_forward
    c = K.make_case(i)
    fam, e, mb = c["family"], c["exp"], c["mb"]
    rows = np.arange(mb)
    eng = _engine(c)
    assert (eng.N, eng.slots, eng.batch_size) == (c["ring"][0], c["ring"][1], mb) and f32(eng.gamma) == f32(c["gamma"])
    # 1. mi_iqn_target is the gradient launch's first pass; a second launch gives the same bits
    eng.sample(c["idx"])
    eng.target()
    alone = (_bits(eng.next_actions), _bits(eng.target_action_quantiles))
    eng.grad()
    got, bits = _result(eng)
    assert np.array_equal(alone[0], bits[4]) and np.array_equal(alone[1], bits[2]), "mi_iqn_target is not the gradient launch's first pass"
    eng.grad()
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    # 2. finite everywhere; a* is float64's on every row; the taus that were used are the taus that were given
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    assert _same(_np(eng.taus), c["taus"]), "taus out is not taus in"
    # 3. the targets, bit for bit, from the device's own quantiles at the successors: a product, then a sum (include/mi_iqn.h)
    _Xb, A, Xn, Rw, Tm = K.batch_of(c)
    tflat = eng.target_network.flat
    q = _np(iqn_forward(tflat, torch.from_numpy(Xn), torch.from_numpy(c["next_taus"]))[1])
    theta = _np(iqn_forward(tflat, torch.from_numpy(Xn), torch.from_numpy(c["tau_dashes"]))[0])
    assert theta.shape == (mb, K.NT, 2) and q.shape == (mb, 2)
    assert np.array_equal((q[:, 1] > q[:, 0]).astype(np.int64), got["next_actions"])
    lg = np.where(Tm != 0, f32(0), f32(c["gamma"])).astype(f32)[:, None]
    tg, cur = _np(eng.target_action_quantiles), _np(eng.current_action_quantiles)
    want = (Rw.astype(f32)[:, None] + (lg * theta[rows, :, got["next_actions"]]).astype(f32)).astype(f32)
    assert _same(want, tg), "target is not f32(r + f32(lg * quantile[a*])) of the device's own quantiles"
    reward = np.repeat(Rw.astype(f32)[:, None], K.NT, axis=1)
    if fam == "target_tie":
        assert _same(q[:, 0], q[:, 1]) and _same(theta[:, :, 0], theta[:, :, 1]) and not got["next_actions"].any()   # the two chains tie bit for bit; a tie goes to action 0
    if c["name"] in ("terminal_all_9", "gamma_0_17", "huber_placed_13"):
        assert _same(tg, reward), "target is not the reward bit for bit"
    if fam in ("huber_placed", "dead_head"):
        assert _same(cur, np.repeat(c["params"][K.QB2:][A][:, None], K.NT, axis=1)), "current is not Q.b2 of the stored action bit for bit"
    if fam == "huber_placed":
        d = tg[:, None, :] - cur[:, :, None]
        for v in K.HUBER_U:
            assert (d == f32(v)).any(), v
    # the loss stage has no fma and the header fixes its order: from the device's own current, target and taus the restatement's row losses, summed in the slab
    # order, are the device's loss
    rl = R.quantile_huber(cur, tg, c["taus"], f32)[2]
    loss_bits = bool(f32(K.sum_rows_slabs(rl) * (f32(1.0) / f32(mb * K.NT))) == f32(got["loss"]))
    assert loss_bits, "the loss through iqn_grad_kernel has not the bits of _iqn_ref.quantile_huber's row losses in the slab order"   # every case, huber_placed's edges among them
    # 4. the figures against float64
    got["q"] = q.astype(np.float64)
    fig = K.figures(e, got)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"], "loss bits:", loss_bits)
    record(c["name"], dict(fig, family=fam, mb=mb, loss_bit_exact=loss_bits))
    assert set(fig) == set(K.FIGURES)
    assert not K.within(fig, fam), (c["name"], K.within(fig, fam))
    # 5. exact zeros stay exact
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    tz = lambda names: sum(K.SIZE[k] for k in names)   # noqa: E731
    least = dict(huber_placed=K.QW2, kink_placed=K.KINK_ZEROS, dead_emb=tz(K.DEAD_ZERO["dead_emb"]), dead_te=tz(K.DEAD_ZERO["dead_te"]), dead_head=K.NP - 2,
                 single_action=K.HID + 1)
    if fam in least:
        assert zero.sum() >= least[fam]
    if fam == "huber_placed":
        assert zero[:K.QW2].all() and K.QW2 == 43_872
    if fam in K.DEAD_ZERO:
        assert all(zero[K.tensor_slice(k)].all() for k in K.DEAD_ZERO[fam])
    if fam == "single_action":
        other = 1 - int(c["place"][-1])
        assert zero[K.QW2:K.QB2].reshape(2, K.HID)[other].all() and zero[K.QB2 + other]
    # 6. a bad index reads a valid row: the same bits as the batch with -1 -> 0 and total -> total - 1
    if fam == "bad_index":
        assert (c["idx"] != c["eidx"]).sum() == 2
        eng.sample(c["eidx"])
        eng.target()
        assert np.array_equal(alone[0], _bits(eng.next_actions)) and np.array_equal(alone[1], _bits(eng.target_action_quantiles))
        eng.grad()
        _, bits3 = _result(eng)
        assert all(np.array_equal(a, b) for a, b in zip(bits, bits3)), "an index outside the ring does not act as the nearest valid row"
    # 7. train_step(idx) from fresh optimizer state with the taus forced: the same bits, parameters that are one Adam step on this gradient
    step = _engine(c)
    step.train_step(c["idx"])
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "train_step's gradient / loss / target / current / a* are not grad()'s bits"
    p = c["params"].copy(); m = np.zeros_like(p); v = np.zeros_like(p)
    R.adam_step(p, _np(eng.grads), m, v, 1, eps=0.01 / mb)                                  # the engine's Adam: eps = 1e-2 / batch_size
    after = _np(step.q.flat)
    assert step.optimizer.step_count == 1 and step.update_index == 1
    assert np.abs(after - p).max() <= R.BOUND_PARAM_ABS
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits


# ---- mi_iqn_forward -----------------------------------------------------------------------------------------------------------------------------------------------
SENTINEL = f32(-12345.5)
FORWARD = ((3, 1, "both"), (3, 2, "both"), (3, 31, "both"), (3, 32, "q_only"), (3, 33, "both"), (3, 63, "quantiles_only"), (3, 64, "both"), (1025, 5, "both"))


def _forward_inputs():
    rng = np.random.default_rng(77)
    return R.init_realistic(rng), rng


@pytest.mark.parametrize("n,k,outs", FORWARD, ids=["n%d_K%d_%s" % f for f in FORWARD])
def test_forward_api_at_every_k_and_past_the_grid(n, k, outs):
    """mi_iqn_forward through _native_iqn at K = 1, 2, 31, 32, 33, 63, 64 (`lane < K ? lane : K - 1`, the `(t >> 1) < K` store guard, the mean over K) and at 1,025
    rows (the grid has 1,024 workgroups: workgroup 0 walks two rows) against _iqn_ref.forward in float64.  taus and obs are views into buffers that hold NaN outside
    the view; quantiles and q are views into buffers prefilled with a sentinel, which must be intact outside the view.  quantiles=None and q=None are run once each."""
    import torch
    from deep_rl_amd import _native_iqn as N
    dev = torch.device("cuda", 0)
    params, rng = _forward_inputs()
    obs = (rng.uniform(-1, 1, (n, 4)) * np.array(K.D.OBS_RANGE)).astype(f32)
    taus = K._grid(rng, (n, k))
    taus[0, 0], taus[n - 1, k - 1] = 0.0, K.TAU_TOP
    ref = R.forward(params, obs, taus, np.float64)

    def view(a, lead, tail, fill):                                        # a device buffer [lead | a | tail] of `fill` around a copy of a -> (buffer, view)
        buf = torch.full((lead + a.size + tail,), float(fill), dtype=torch.float32, device=dev)
        v = buf[lead:lead + a.size]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, f32).reshape(-1)))
        return buf, v

    p = torch.from_numpy(params).to(dev)
    _ob, o = view(obs, 8, 5, np.nan)                                      # (the view stays 16-byte aligned, as the call requires of obs)
    _tb, t = view(taus, 3, 7, np.nan)
    qb, qv = view(np.full((n, k, 2), SENTINEL), 5, 9, SENTINEL)
    ab, av = view(np.full((n, 2), SENTINEL), 1, 6, SENTINEL)
    assert o.data_ptr() % 16 == 0 and t.data_ptr() % 16 != 0
    N.check(N.lib().mi_iqn_forward(N.ptr(p), N.ptr(o), N.ptr(t), n, k, N.ptr(qv) if outs != "q_only" else None, N.ptr(av) if outs != "quantiles_only" else None,
                                   N.stream_ptr(dev)), "mi_iqn_forward")
    torch.cuda.synchronize()
    quant, q = _np(qv).reshape(n, k, 2), _np(av).reshape(n, 2)
    qb, ab = _np(qb), _np(ab)
    assert (qb[:5] == SENTINEL).all() and (qb[5 + n * k * 2:] == SENTINEL).all() and (ab[:1] == SENTINEL).all() and (ab[1 + 2 * n:] == SENTINEL).all()
    scale = max(1.0, float(np.abs(ref["quantiles"]).max()))
    fig = dict(n=n, k=k)
    if outs == "q_only":
        assert (quant == SENTINEL).all()                                  # quantiles = NULL: nothing of that size is written anywhere we can see
    else:
        assert np.isfinite(quant).all()
        fig["quantiles_rel"] = float(np.abs(quant - ref["quantiles"]).max() / scale)
        assert fig["quantiles_rel"] <= R.BOUND_QUANT_REL
    if outs == "quantiles_only":
        assert (q == SENTINEL).all()
    else:
        assert np.isfinite(q).all()
        fig["q_abs"] = float(np.abs(q - ref["q"]).max())
        assert fig["q_abs"] <= R.BOUND_Q_ABS
    if outs == "both":                                                    # q is the ascending sum of the launch's own quantiles over K, bit for bit
        s = np.zeros((n, 2), f32)
        for j in range(k):
            s = (s + quant[:, j]).astype(f32)
        assert _same((s / f32(k)).astype(f32), q)
    print("forward", fig, "scale", scale)
    record("forward_n%d_K%d" % (n, k), fig)
