"""The SAC kernels (deep_rl_amd/csrc/mi_sac.hip, mi_sac_rowgroup.inc) on the synthetic cases of tests/_sac_cases.py (validated on the CPU by
tests/test_sac_cases_cpu.py) against FLOAT64 AUTOGRAD: a saturated tanh squash (u == +-1), the +1e-6 of the log-prob correction, both ends of the log-std clamp,
bit-for-bit ties of min(Q1, Q2), batches of 1 / 5 / 16 / 17 / 40 rows around the 16-row group, rings down to two slots, terminated rows and wrapping successors —
through SACEngine, Actor and SoftQNetwork with forced indices and noise.  Every other SAC expectation in the suite comes from oracle/cpu_ref.c, which derives the
same backward pass by hand as the kernels do; this reference does not.

Every case runs in both launch forms of the actor / critic kernels: as launched by default (sibling workgroups per row group: the tie weights of mi_sac.hip's
`split` branch) and under mi_sac_set_max_cus(2), which sends a small batch through the single-workgroup form (its own tie arithmetic).  Each form is held to
float64 on its own; nothing here requires the two to agree with each other (on the MI355X their figures came out equal in every digit: the split form scales a
unit-weight backward pass by the routing weight afterwards, which is exact).

Bounds: _sac_cases.BOUND (8 x the f32 oracle's measured distance from float64, per family and figure; band B has loose ones of its own).  Nothing is excluded.
Observed maxima go to sac_gpu_maxima.json in the tests' results directory (a copy is kept as profiles/sac_gpu_maxima.json, the figures in docs/LEDGER.md)."""
import json
import os

import numpy as np
import pytest
import torch

import _sac_cases as K
from _c51_ref import results_dir
from test_gpu_sac import _engine

pytestmark = pytest.mark.gpu
f32 = np.float32
TE = K.TARGET_ENTROPY


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    return cpu_ref


@pytest.fixture(params=["default", "one_workgroup"])
def form(request, dev):
    """the launch form of the row-group kernels.  mi_sac_set_max_cus is process-wide and the engine reads it when it is built (and at every launch): set before the
    engine exists, back to 0 afterwards whatever the test did"""
    from deep_rl_amd import _native as N

    L = N.lib()
    try:
        if request.param == "one_workgroup":
            N.check(L.mi_sac_set_max_cus(2), "mi_sac_set_max_cus")
            assert L.mi_sac_usable_cus() == 2            # sac_roles: row groups x 2 > 2 / 2 -> one role
        else:
            assert L.mi_sac_usable_cus() >= 24           # three row groups x four roles fit into half of the CUs: sibling roles run
        yield request.param
    finally:
        L.mi_sac_set_max_cus(0)


def _record(key, value):
    path = os.path.join(results_dir(), "sac_gpu_maxima.json")
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


def _np(t):
    return t.detach().cpu().numpy()


def _build(dev, c):
    eng = _engine(dev, c["n_envs"], c["slots"], actor=c["actor"], q=c["q"], qt=c["qt"], batch_size=c["batch"])
    eng.observations.copy_(torch.from_numpy(c["obs"])); eng.actions.copy_(torch.from_numpy(c["actions"]))
    eng.rewards.copy_(torch.from_numpy(c["rewards"])); eng.terminated.copy_(torch.from_numpy(c["term"]))
    eng.alpha.fill_(float(f32(c["alpha"])))
    eng.sample(c["idx"])
    return eng


def _rows(c):
    n, slots, idx = c["n_envs"], c["slots"], c["idx"]
    flat = c["obs"].reshape(-1, 3)
    return flat[((idx // n + 1) % slots) * n + idx % n], flat[idx]


def _set_alpha_state(eng, c):
    eng.log_alpha.copy_(torch.tensor([c["log_alpha"]], dtype=torch.float32)); eng._alpha_m.copy_(torch.tensor([0.01])); eng._alpha_v.copy_(torch.tensor([0.002]))
    eng.alpha_steps = 6


def _run(dev, R, c, form):
    """every comparison of one case in one launch form"""
    fam, e = c["family"], c["exp"]
    eng = _build(dev, c)
    assert eng._owed_fits == (form == "default")       # the engine saw the knob: under 2 CUs no launch may carry an owed alpha step either
    nxt, cur = _rows(c)
    eps = {p: torch.from_numpy(c["eps_" + p]) for p in ("critic", "actor", "alpha")}
    got = {}
    # ---- per row: Actor.get_action at the rows and draws of each consumer
    for p, rows in (("critic", nxt), ("actor", cur), ("alpha", cur)):
        a, lp = eng.actor.get_action(torch.from_numpy(rows), eps[p])
        got[p] = dict(action=_np(a)[:, 0], logp=_np(lp))
        assert np.isfinite(got[p]["action"]).all() and np.isfinite(got[p]["logp"]).all()
        sat = np.abs(e[p]["z"]) >= 16 - 1e-6
        if fam in ("C", "AC"):
            assert sat.any() and (fam == "AC" or sat.all())
            assert np.array_equal(got[p]["action"][sat], 2.0 * np.sign(e[p]["z"][sat]).astype(f32))          # exactly +-2
    # ---- whole batch: gradients and losses, each call twice
    eng.critic_grad(eps["critic"])
    got["critic"].update(grads=_np(eng.q_grads).copy(), losses=_np(eng.q_losses).copy())
    eng.critic_grad(eps["critic"])
    assert np.array_equal(_np(eng.q_grads), got["critic"]["grads"]) and np.array_equal(_np(eng.q_losses), got["critic"]["losses"])
    eng.actor_grad(eps["actor"])
    out = _np(eng.actor_out).copy()
    got["actor"].update(grads=_np(eng.actor_grads).copy(), loss=float(out[0]), mlp=float(out[1]))
    eng.actor_grad(eps["actor"])
    assert np.array_equal(_np(eng.actor_grads), got["actor"]["grads"]) and np.array_equal(_np(eng.actor_out), out)
    _set_alpha_state(eng, c)
    eng.update_alpha(eps["alpha"])
    ao, la1 = _np(eng.alpha_out).copy(), _np(eng.log_alpha).copy()
    got["alpha"].update(mlp=float(-ao[1]) - TE, loss=float(ao[0]))        # alpha_out = {alpha_loss, d alpha_loss / d log_alpha = -(mean logp + target entropy)}
    _set_alpha_state(eng, c)
    eng.update_alpha(eps["alpha"])
    assert np.array_equal(_np(eng.alpha_out), ao) and np.array_equal(_np(eng.log_alpha), la1)
    for p in got:
        assert all(np.isfinite(v).all() for v in got[p].values()), p
    fig = K.figures(e, got)
    print(c["name"], form, {k: float("%.3g" % v) for k, v in fig.items()})
    _record("%s/%s" % (c["name"], form), dict(fig, family=fam, batch=c["batch"]))
    assert abs(float(ao[1]) - e["alpha"]["grad"]) <= K.BOUND[fam]["mlp"]
    assert not K.within(fig, fam), (c["name"], form, K.within(fig, fam))
    if fam == "clamp20":      # ls == +-1: nothing reaches the log-std head
        a, b = K.AC["WL"][0], K.AC["BL"][1]
        assert not got["actor"]["grads"][a:b].any()
    # ---- the alpha step is Adam on exactly that gradient
    la = np.array([c["log_alpha"]], f32); m = np.array([0.01], f32); v = np.array([0.002], f32)
    R.adam_step(la, np.array([ao[1]], f32), m, v, 7, 1e-3, eps=1e-8)
    assert abs(float(la1[0]) - la[0]) < 1e-6 and abs(float(eng.alpha) - np.exp(la[0])) < 1e-6
    # ---- the fused updates step the parameters by Adam on exactly these gradients
    eng.alpha.fill_(float(f32(c["alpha"])))
    p0 = c["q"].copy(); m = np.zeros_like(p0); v = np.zeros_like(p0)
    R.adam_step(p0, got["critic"]["grads"], m, v, 1, 1e-3, eps=1e-8)
    eng.update_critic(eps["critic"])
    assert np.array_equal(_np(eng.q_grads), got["critic"]["grads"]) and np.array_equal(_np(eng.q_losses), got["critic"]["losses"])
    assert np.abs(_np(eng.q_flat) - p0).max() <= 1e-9 + 2e-7 * np.abs(p0).max()
    assert np.array_equal(_np(eng.qt_flat), c["qt"])                       # (no polyak step was asked for)
    eng.q_flat.copy_(torch.from_numpy(c["q"]).to(dev))                     # the actor update reads the critics: back to the case's
    p0 = c["actor"].copy(); m = np.zeros_like(p0); v = np.zeros_like(p0)
    R.adam_step(p0, got["actor"]["grads"], m, v, 1, 3e-4, eps=1e-8)
    eng.update_actor(eps["actor"])
    assert np.array_equal(_np(eng.actor_grads), got["actor"]["grads"]) and np.array_equal(_np(eng.actor_out), out)
    assert np.abs(_np(eng.actor.flat) - p0).max() <= 1e-9 + 2e-7 * np.abs(p0).max()
    eng.check()
    eng.close()
    return got


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=[s[0] for s in K.SPECS])
def test_case_against_float64(dev, R, form, i):
    _run(dev, R, K.make_case(i), form)


@pytest.mark.parametrize("batch", K.TIE_BATCHES)
def test_tie_of_the_two_critics_routes_half_and_half(dev, R, form, batch):
    """q1 == q2 bit for bit on the tie rows, with d q1 / da = 1 and d q2 / da = 2: d(-min Q)/da is -1.5 there and -1 on the rows where critic 2 lies above.  The
    tie is made from the action the DEVICE gives (b3 = -a)."""
    import deep_rl_amd as D

    env = D.make("Pendulum-v1", num_envs=1, device=dev)
    actor = D.Actor(env)
    actor.load_flat(K.tie_actor())
    a, _ = actor.get_action(torch.tensor([[1.0, 0.0, 0.0]]), torch.tensor([K.TIE_EPS]))
    c = K.make_tie_case(batch, _np(a)[0, 0])
    _, cur = _rows(c)
    a, _ = actor.get_action(torch.from_numpy(cur), torch.from_numpy(c["eps_actor"]))
    assert (_np(a)[:, 0] == c["a"]).all()                                   # zero weights: the same action on every row
    c = K.finish_tie(c)
    t = c["tie_rows"]
    assert K.conditions_met(c) and t.sum() >= 2 and (~t).sum() >= 2         # (the conditions again, with the device's a)
    got = _run(dev, R, c, form)
    assert (got["actor"]["action"] == c["a"]).all()
    q1, q2 = D.SoftQNetwork(env), D.SoftQNetwork(env)
    q1.load_flat(c["q"][:K.SQ_NP]); q2.load_flat(c["q"][K.SQ_NP:])
    v1, v2 = _np(q1(torch.from_numpy(cur), a)), _np(q2(torch.from_numpy(cur), a))
    assert np.array_equal(v1[t], v2[t]) and (v1 == c["a"]).all() and (v2[~t] > v1[~t] + K.Q_MARGIN).all()
    # the wrong routings lie far outside the bound that _run has just held the device to (tests/test_sac_cases_cpu.py: test_teeth_tie_routing)
    for w in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
        assert K.rel(got["actor"]["grads"], K.actor_eval(c, tie_weights=w)["grads"]) > 10 * K.BOUND["tie"]["grad"]
