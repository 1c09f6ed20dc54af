"""c51_grad_kernel, c51_target_kernel, c51_forward_kernel and c51_reduce_kernel (deep_rl_amd/csrc/mi_c51.hip; torso and slab sum of mi_torso.h / mi_ring.h) on the
placed edge cases of tests/_c51_edge_cases.py (validated on the CPU by tests/test_c51_edge_cases_cpu.py) against FLOAT64 AUTOGRAD, through C51Engine with forced
indices: every tail of the slab sum, a target head that ties bit for bit, whole batches with live == 0 and live == 1, gamma 0 and 1, b at exactly 0, 100 and 99.5 and
far past the clamp, softmaxes saturated until f32 holds exact zeros, pre-activations of exactly 0, a dead layer, one stored action, indices outside the ring.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_c51_edge_cases.BOUND = max(8 x the f32 restatement's measured distance from float64, the shipped bound of tests/_c51_ref.py), per family and figure.  No case and no
row is excluded, action comparisons included.  Observed maxima go to c51_edge_gpu_maxima.json in the tests' results directory (a copy: profiles/)."""
import json
import os

import numpy as np
import pytest

import _c51_edge_cases as K
import _c51_ref as X
from test_gpu_c51 import _make, _np

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(t):
    a = _np(t).copy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def record(key, value):
    path = os.path.join(X.results_dir(), "c51_edge_gpu_maxima.json")
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
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target_probs=_np(eng.target_probs).astype(np.float64),
               probs=_np(eng.probs).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64))
    return got, [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_probs), _bits(eng.probs), _bits(eng.next_actions)]


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(i):
    import torch
    c = K.make_case(i)
    fam, e, mb = c["family"], c["exp"], c["mb"]
    eng = _engine(c)
    assert (eng.N, eng.slots, eng.batch_size) == (c["ring"][0], c["ring"][1], mb) and f32(eng.gamma) == f32(c["gamma"])
    # 1. mi_c51_target is the gradient launch's first pass; a second launch gives the same bits
    eng.sample(c["idx"])
    eng.target()
    alone = (_bits(eng.next_actions), _bits(eng.target_probs))
    eng.grad()
    got, bits = _result(eng)
    assert np.array_equal(alone[0], bits[4]) and np.array_equal(alone[1], bits[2]), "mi_c51_target is not the gradient launch's first pass"
    eng.grad()
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    # 2. finite everywhere; a* is float64's on every row
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    # 3. the projection, bit for bit, of the device's own next-distribution
    _Xb, _A, Xn, Rw, Tm = K.batch_of(c)
    P = _np(eng.target_network.get_probs(torch.from_numpy(Xn)))
    q = _np(eng.target_network.get_q_values(torch.from_numpy(Xn)))
    assert np.array_equal((q[:, 1] > q[:, 0]).astype(np.int64), got["next_actions"])
    nextp = P[np.arange(mb), got["next_actions"]]
    tp = _np(eng.target_probs)
    assert np.array_equal(X.project(nextp, Rw, Tm, c["gamma"])[0].view(np.uint32), tp.view(np.uint32)), "target_probs are not project() of the device's next_probs"
    if fam == "target_tie":
        assert np.array_equal(q[:, 0].copy().view(np.uint32), q[:, 1].copy().view(np.uint32)) and not got["next_actions"].any()   # a tie goes to action 0
    if c["name"] == "gamma_1_17":
        assert sorted(K.gamma1_identities(tp, nextp, Rw, Tm == 0)) == sorted(K.GAMMA_REWARDS.tolist())
    if c["name"] == "terminal_all_9":
        assert ((tp != 0).sum(-1) <= 2).all() and np.abs(tp.astype(np.float64).sum(-1) - 1).max() <= K.NA * 2.0 ** -23
    if fam == "edge_rewards":
        for row, (r, atoms) in enumerate(K.EDGE_REWARDS):
            assert Rw[row] == f32(r) and tuple(np.flatnonzero(tp[row])) == atoms, (r, np.flatnonzero(tp[row]))
    # 4. the figures against float64
    got["q"] = q.astype(np.float64)
    fig = K.figures(e, got)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=mb))
    assert set(fig) == set(K.FIGURES)
    assert not K.within(fig, fam), (c["name"], K.within(fig, fam))
    # 5. exact zeros stay exact
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    if fam in ("kink_placed", "dead", "single_action"):
        assert zero.sum() >= {"kink_placed": 4 * 4 + 4 + 4 * K.H1 + 4, "dead": K.B3, "single_action": K.NA * K.H2 + K.NA}[fam]
    # 6. a bad index reads a valid row: the same bits as the batch with -1 -> 0 and total -> total - 1
    if fam == "bad_index":
        assert (c["idx"] != c["eidx"]).sum() == 2
        eng.sample(c["eidx"])
        eng.target()
        assert np.array_equal(alone[0], _bits(eng.next_actions)) and np.array_equal(alone[1], _bits(eng.target_probs))
        eng.grad()
        _, bits3 = _result(eng)
        assert all(np.array_equal(a, b) for a, b in zip(bits, bits3)), "an index outside the ring does not act as the nearest valid row"
    # 7. train_step(idx) from fresh optimizer state: the same bits, parameters that are one Adam step on this gradient
    step = _engine(c)
    step.train_step(c["idx"])
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "train_step's gradient / loss / target_probs / probs / a* are not grad()'s bits"
    p = c["params"].copy(); m = np.zeros_like(p); v = np.zeros_like(p)
    X.adam_step(p, _np(eng.grads), m, v, 1)
    after = _np(step.q.flat)
    assert step.optimizer.step_count == 1 and step.update_index == 1
    assert np.abs(after - p).max() <= 1e-6
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits
