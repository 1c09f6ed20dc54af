"""dqn_td_kernel<8> / <16>, dqn_reduce_kernel / dqn_reduce2_kernel, the PER weight, |td| and priority path and the dueling pack / unpack (deep_rl_amd/csrc/mi_dqn.hip)
on the synthetic rings of tests/_dqn_cases.py (validated on the CPU by tests/test_dqn_cases_cpu.py) against FLOAT64 AUTOGRAD, through DQNEngine, PERDQNEngine and
DuelingDQNEngine with forced indices: rewards that differ at the row and at its successor with the row's OWN reward poisoned, whole batches with live == 0 and with
live == 1, gamma 0 and 1, Q values of 30 ... 300, pre-activations of exactly 0, dead layers, a bit-for-bit target tie, placed importance weights (0 among them),
priorities over 15 decades at alpha 0.6 / 1.0 and beta beta_0 / 1, and the form boundaries (8 rows per group, 63 / 64 slabs, 2,048 / 2,049 rows, 258 groups of 16 on
256 workgroups).  Every other expectation of these kernels in the suite comes from oracle/cpu_ref.c, which derives the same backward pass by hand as the kernel does
(the plain-DQN image of the dueling head included), or from the one golden trace of the reference run; this reference does not.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_dqn_cases.BOUND = max(8 x the f32 oracle's measured distance from float64, the bar of test_gpu_dqn.py / test_gpu_per.py / test_gpu_dueling.py), per engine kind, family
and figure; converged has loose ones of its own.  No case and no row is excluded.  Observed maxima go to dqn_gpu_maxima.json in the tests' results directory (a copy is
kept as profiles/dqn_gpu_maxima.json, the figures in docs/LEDGER.md).  Not covered: rings of 2^32 transitions or more (they need tens of GB)."""
import json
import os

import numpy as np
import pytest
import torch

import _dqn_cases as K
from _c51_ref import results_dir

pytestmark = pytest.mark.gpu
LR = 2.5e-4
TRAIN_STEP_CASES = ("dead_l2_5", "kink_placed_8")        # (the dueling engine does not run `dead`: kink_placed_8 and kink_placed_24 there)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _engine(dev, c, kind):
    """the way test_gpu_dqn.py / test_gpu_per.py / test_gpu_dueling.py build theirs, with the case's ring, batch and gamma; the whole ring valid"""
    from test_gpu_dqn import _engine as dqn_engine
    from test_gpu_dueling import _engine as dueling_engine
    from test_gpu_per import _engine as per_engine

    (N, S), kw = c["ring"], dict(batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0)
    if kind == "dqn":
        eng = dqn_engine(dev, N, S, params=c["params"], **kw)
    elif kind == "per":
        eng = per_engine(dev, N, S, params=c["params"], alpha=c["alpha"], beta_0=K.BETA_0, total_timesteps=c["total_timesteps"], **kw)
    else:
        eng = dueling_engine(dev, N, S, params=c["dparams"], **kw)
    eng.target.load_flat(c["dtarget" if kind == "dueling" else "target"])
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S                                    # min(global_step, slots) * N: every transition of the ring is stored
    if kind == "per":
        eng.priorities.copy_(torch.from_numpy(c["priorities"]))
        eng.refresh_sums()
        eng.max_priority.fill_(float(c["max_priority"]))
        assert float(np.float32(eng.beta())) == c["beta"]
    return eng


def _sample(eng, c, kind):
    eng.sample(c["idx"])
    if kind == "per" and c["placed_weights"] is not None:
        eng.weights.copy_(torch.from_numpy(c["placed_weights"]))


def _bits(t):
    return t.detach().cpu().numpy().copy().view(np.uint32)


def _result(eng, kind):
    """what one td_grad() left: the `got` dict of K.figures() and its bits"""
    g = eng.dueling_grads if kind == "dueling" else eng.grads
    got = dict(grads=g.cpu().numpy().astype(np.float64), loss=float(eng.loss.item()))
    bits = [_bits(g), _bits(eng.loss), _bits(eng.grads)]
    if kind == "per":
        got.update(td_abs=eng.td_abs.cpu().numpy().astype(np.float64), weights=eng.weights.cpu().numpy().astype(np.float64),
                   prio=eng.priorities.cpu().numpy().reshape(-1).astype(np.float64), max_priority=float(eng.max_priority.item()))
        bits += [_bits(eng.td_abs), _bits(eng.weights), _bits(eng.priorities), _bits(eng.max_priority)]
    return got, bits


def _record(key, value):
    path = os.path.join(results_dir(), "dqn_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
    for k in K.FIGURES:
        if k in value:
            fam[k] = max(fam.get(k, 0.0), value[k])
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("kind,i", K.RUNS, ids=K.RUN_IDS)
def test_case_against_float64(dev, kind, i):
    c = K.make_case(i)
    fam, e = c["family"], c["exp"][kind]
    eng = _engine(dev, c, kind)
    assert (eng.N, eng.slots, eng.batch_size, eng.gamma) == (c["ring"][0], c["ring"][1], c["mb"], c["gamma"])
    _sample(eng, c, kind)
    eng.td_grad()
    got, bits = _result(eng, kind)
    eng.td_grad()
    again, bits2 = _result(eng, kind)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    fig = K.figures(e, got, kind)
    per_tensor = K.tensor_errors(got["grads"], e["grads"], kind)
    print(kind, c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, {k: float("%.3g" % v) for k, v in per_tensor.items()}, got["loss"], e["loss"])
    _record("%s/%s" % (kind, c["name"]), dict(fig, family=fam, mb=c["mb"]))
    assert set(fig) == set(K.BAR[kind])
    assert not K.within(fig, fam, kind), (kind, c["name"], K.within(fig, fam, kind), per_tensor)
    zero = K.zero_mask(e)
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    if kind == "per":
        if c["placed_weights"] is not None:
            assert np.array_equal(got["weights"], c["placed_weights"].astype(np.float64))
        if c["prio"] == "same":
            assert (got["weights"] == 1.0).all()
        if c["mp"] == "above":                             # above every |td|: it stays bit for bit
            assert np.array_equal(_bits(eng.max_priority), np.array([c["max_priority"]], np.float32).view(np.uint32))
        untouched = np.ones(len(got["prio"]), bool); untouched[c["idx"]] = False
        assert np.array_equal(got["prio"][untouched], c["priorities"].reshape(-1)[untouched].astype(np.float64)), "a priority outside the batch was written"
        assert np.array_equal(got["prio"][c["idx"]], got["td_abs"])
    if c["name"] == "terminal_all_9":                      # live == 0 in every row: another target vector, the same bits
        other = np.random.default_rng(99).normal(0, 1, K.DNP).astype(np.float32)[:eng.target.flat.numel()]
        eng.target.load_flat(other)                        # (the batch and its weights stay: PER's first td_grad() has scattered new priorities, a second sample() would weigh by those)
        eng.td_grad()
        _, bits3 = _result(eng, kind)
        assert all(np.array_equal(a, b) for a, b in zip(bits, bits3)), "the target net reaches a batch whose successors are all terminated"


@pytest.mark.parametrize("kind,i", [r for r in K.RUNS if K.SPECS[r[1]]["name"] in TRAIN_STEP_CASES or (r[0] == "dueling" and K.SPECS[r[1]]["family"] == "kink_placed")],
                         ids=lambda v: v if isinstance(v, str) else K.NAMES[v])
def test_one_call_train_step_on_exact_zero_gradients(dev, kind, i):
    """eng.train_step(idx) from fresh optimizer state: gradient and loss are td_grad()'s bits; a parameter whose gradient is exactly 0 keeps its bits and both its moments
    stay 0; every other one moves against its gradient by at most lr — Adam's first step is lr g / (|g| + eps), within 1e-6 of itself on the hardware sqrt / rcp, and p - step is rounded once"""
    c = K.make_case(i)
    ref = _engine(dev, c, kind)
    _sample(ref, c, kind)
    ref.td_grad()
    _, want = _result(ref, kind)
    eng = _engine(dev, c, kind)
    if kind == "per" and c["placed_weights"] is not None:
        pytest.fail("the one-call PER step draws its weights itself: not a case for this test")
    flat = eng.q.flat
    before = flat.cpu().numpy().copy()
    eng.train_step(c["idx"])
    got, bits = _result(eng, kind)
    assert eng.optimizer.step_count == 1
    assert all(np.array_equal(a, b) for a, b in zip(bits[:3], want[:3])), "train_step's gradient / loss are not td_grad()'s bits"
    if kind == "per":
        assert all(np.array_equal(a, b) for a, b in zip(bits[3:], want[3:])), "train_step's |td| / weights / priorities / max_priority are not td_grad()'s bits"
    g = got["grads"]
    after = flat.cpu().numpy()
    m, v = eng.optimizer.exp_avg.cpu().numpy(), eng.optimizer.exp_avg_sq.cpu().numpy()
    zero = g == 0
    assert zero.sum() >= (K.HEAD if c["name"] == "dead_l2_5" else 4 * 4 + 4 + 4 * K.H1 + 4)
    assert np.array_equal(before[zero].view(np.uint32), after[zero].view(np.uint32)) and not m[zero].any() and not v[zero].any()
    moved = after.astype(np.float64) - before.astype(np.float64)
    nz = ~zero
    assert (moved[nz] * g[nz] <= 0).all(), "a parameter moved along its gradient"
    half_ulp = 0.5 * np.spacing(np.maximum(np.abs(before[nz]), np.abs(after[nz]))).astype(np.float64)   # the one rounding of p - step, in the binade the result lands in
    over = np.abs(moved[nz]) - (LR * (1 + 1e-6) + half_ulp)
    assert (over <= 0).all(), ("a first Adam step larger than lr", over.max(), before[nz][over.argmax()], after[nz][over.argmax()], g[nz][over.argmax()])
    step = LR * np.abs(g[nz]) / (np.abs(g[nz]) + 1e-8)
    sure = step > np.spacing(np.abs(before[nz])).astype(np.float64)       # the step is more than the parameter's spacing: it cannot round away
    assert sure.sum() > 0 and (moved[nz][sure] != 0).all() and (m[nz] != 0).all()
    if kind == "dueling":                                  # the plain-DQN image follows the stepped parameters
        img = eng.q.eff.clone()
        eng.q.repack()
        assert torch.equal(img, eng.q.eff)
