"""qr_grad_kernel, qr_target_kernel, qr_forward_kernel and qr_reduce_kernel (deep_rl_amd/csrc/mi_qr.hip; torso and slab sum of mi_torso.h / mi_ring.h) on the placed
edge cases of tests/_qrdqn_edge_cases.py (validated on the CPU by tests/test_qrdqn_edge_cases_cpu.py) against FLOAT64 AUTOGRAD, through QRDQNEngine with forced
indices: every tail of the slab sum, a target head that ties bit for bit, whole batches with lg == 0 and lg == gamma, gamma 0 and 1, u at exactly 0, +-1, one step to
either side of +-1 and far out through the gradient launch, all-linear and all-quadratic batches, pre-activations of exactly 0, a dead layer, one stored action (either
one), indices outside the ring.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_qrdqn_edge_cases.BOUND = max(8 x the f32 restatement's measured distance from float64, the shipped bound of tests/_qrdqn_ref.py), per family and figure.  No case and
no row is excluded, action comparisons included.  Observed maxima go to qrdqn_edge_gpu_maxima.json in the tests' results directory (a copy: profiles/)."""
import json
import os

import numpy as np
import pytest

import _qrdqn_edge_cases as K
import _qrdqn_ref as X
from test_gpu_qrdqn import _make, _np

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(t):
    a = _np(t).copy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def record(key, value):
    path = os.path.join(X.results_dir(), "qrdqn_edge_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
    for k in K.FIGURES:
        fam[k] = max(fam.get(k, 0.0), value[k])
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _engine(c):
    import torch
    N, S = c["ring"]
    eng = _make(n=N, slots=S, batch_size=c["mb"], params=c["params"], target=c["target"], gamma=c["gamma"], max_episodes_logged=0)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S                                    # min(global_step, slots) * N: every transition of the ring is stored
    return eng


def _result(eng):
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target=_np(eng.target_quantiles).astype(np.float64),
               current=_np(eng.current).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64))
    return got, [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_quantiles), _bits(eng.current), _bits(eng.next_actions)]


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(i):
    import torch
    c = K.make_case(i)
    fam, e, mb = c["family"], c["exp"], c["mb"]
    rows = np.arange(mb)
    eng = _engine(c)
    assert (eng.N, eng.slots, eng.batch_size) == (c["ring"][0], c["ring"][1], mb) and f32(eng.gamma) == f32(c["gamma"])
    # 1. mi_qr_target is the gradient launch's first pass; a second launch gives the same bits
    eng.sample(c["idx"])
    eng.target()
    alone = (_bits(eng.next_actions), _bits(eng.target_quantiles))
    eng.grad()
    got, bits = _result(eng)
    assert np.array_equal(alone[0], bits[4]) and np.array_equal(alone[1], bits[2]), "mi_qr_target is not the gradient launch's first pass"
    eng.grad()
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    # 2. finite everywhere; a* is float64's on every row
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    # 3. the targets, bit for bit, from the device's own quantiles at the successors: a product, then a sum (include/mi_qr.h)
    _Xb, A, Xn, Rw, Tm = K.batch_of(c)
    theta = _np(eng.target_network.get_quantiles(torch.from_numpy(Xn)))
    q = _np(eng.target_network.get_q_values(torch.from_numpy(Xn)))
    assert theta.shape == (mb, 2, K.NQ) and q.shape == (mb, 2)
    assert np.array_equal((q[:, 1] > q[:, 0]).astype(np.int64), got["next_actions"])
    lg = np.where(Tm != 0, f32(0), f32(c["gamma"])).astype(f32)[:, None]
    tg, cur = _np(eng.target_quantiles), _np(eng.current)
    want = (Rw.astype(f32)[:, None] + (lg * theta[rows, got["next_actions"]]).astype(f32)).astype(f32)
    assert _same(want, tg), "target is not f32(r + f32(lg * theta[a*])) of the device's own quantiles"
    reward = np.repeat(Rw.astype(f32)[:, None], K.NQ, axis=1)
    if fam == "target_tie":
        assert _same(q[:, 0], q[:, 1]) and not got["next_actions"].any()                            # the collapsed head ties bit for bit; a tie goes to action 0
    if c["name"] in ("terminal_all_9", "gamma_0_17", "huber_placed_9"):
        assert _same(tg, reward), "target is not the reward bit for bit"
    if fam == "huber_placed":
        b3 = c["params"][K.B3:].reshape(2, K.NQ)
        assert _same(cur, b3[A]), "current is not b3 of the stored action bit for bit"
        u = tg[:, None, :] - cur[:, :, None]
        for v in K.HUBER_U:
            assert (u == f32(v)).any(), v
    # the loss stage has no fma and the header fixes its order: from the device's own current and target the restatement gives the device's loss
    rl, _d = X.huber_rows(cur, tg)
    loss_bits = bool(f32(X.sum_rows_slabs(rl) * (f32(1.0) / f32(mb * K.NQ))) == f32(got["loss"]))
    assert loss_bits, "the loss through qr_grad_kernel has not the bits of _qrdqn_ref.huber_rows + sum_rows_slabs"   # every case, huber_placed's edges among them
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
    if fam in ("huber_placed", "kink_placed", "dead", "single_action"):
        assert zero.sum() >= {"huber_placed": 10_764, "kink_placed": 4 * 4 + 4 + 4 * K.H1 + 4, "dead": K.B3, "single_action": K.NQ * K.H2 + K.NQ}[fam]
    if fam == "huber_placed":
        assert zero[:K.W3].all()
    if fam == "dead":
        assert zero[:K.B3].all()
    if fam == "single_action":
        other = 1 - int(c["place"][-1])
        assert zero[K.W3:K.B3].reshape(2, K.NQ, K.H2)[other].all() and zero[K.B3:].reshape(2, K.NQ)[other].all()
    # 6. a bad index reads a valid row: the same bits as the batch with -1 -> 0 and total -> total - 1
    if fam == "bad_index":
        assert (c["idx"] != c["eidx"]).sum() == 2
        eng.sample(c["eidx"])
        eng.target()
        assert np.array_equal(alone[0], _bits(eng.next_actions)) and np.array_equal(alone[1], _bits(eng.target_quantiles))
        eng.grad()
        _, bits3 = _result(eng)
        assert all(np.array_equal(a, b) for a, b in zip(bits, bits3)), "an index outside the ring does not act as the nearest valid row"
    # 7. train_step(idx) from fresh optimizer state: the same bits, parameters that are one Adam step on this gradient
    step = _engine(c)
    step.train_step(c["idx"])
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "train_step's gradient / loss / target / current / a* are not grad()'s bits"
    p = c["params"].copy(); m = np.zeros_like(p); v = np.zeros_like(p)
    X.adam_step(p, _np(eng.grads), m, v, 1)
    after = _np(step.q.flat)
    assert step.optimizer.step_count == 1 and step.update_index == 1
    assert np.abs(after - p).max() <= 1e-6
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits
