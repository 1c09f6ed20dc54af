"""torch restatement of the Munchausen DQN target, loss and gradient (include/mi_mdqn.h) — TEST INFRASTRUCTURE (tests/test_mdqn_cases_cpu.py validates and measures
it, the GPU tests use it).

The reference has no munchausen_dqn.py.  This is dqn.py's TD update with the target of Vieillard, Pietquin and Geist (2020), in the paper's own form, on the
[slots][N] time-major ring of the engines, in float64 or float32; Qt is the TARGET network, hp = (alpha, tau, clip_lo) rounded to float32 first:
    nx = ((i // N + 1) % slots) * N + i % N
    bonus      = clamp(tau * log_softmax(Qt(obs[i]) / tau)[a[i]], clip_lo, 0)
    pi, lp     = softmax(Qt(obs[nx]) / tau), log_softmax(Qt(obs[nx]) / tau)
    soft_value = sum_a pi_a (Qt(obs[nx])_a - tau lp_a)                         (the sum over the actions, not the closed form the kernel uses)
    target     = r[nx] + alpha bonus + f32(gamma) soft_value (1 - terminated[nx])          under no_grad
    old = Q_online(obs[i])[a[i]];  loss = mean((target - old)^2)
AUTOGRAD produces every gradient — there is no hand-written backward in this file.  The network, the flat layout and the successor rule are tests/_dqn_cases.py's
(q_values, successor), imported unchanged.

`variant=` names a deliberately WRONG reading, used only by the CPU test to show that the cases tell it from the right one:
  no_clip                     the bonus is not clipped
  bonus_from_online           the log-policy of the ONLINE network
  bonus_at_successor          the log-policy at obs[nx] instead of obs[i]
  hard_max                    the target network's maximum in the place of the soft value
  entropy_sign_flipped        sum_a pi_a (q_a + tau ln pi_a)
  bonus_masked_by_terminated  the bonus multiplied by (1 - terminated[nx])

Figures (figures()).  "target", "current", "bonus", "soft_value": max |x - x64|, absolute.  "loss": |x - ref| / |ref|.  "grad": max |g - ref| / max |ref|.  A NaN
where the reference is finite makes the figure inf.

Bounds.  MEASURED[family][figure] is what tests/test_mdqn_cases_cpu.py measures for the FLOAT32 torch evaluation of these same formulas against the float64 one, the
maximum over the family's cases (the test ties the constants to the measurement: the constant covers the measured figure and is at most 1.25 x it).
BOUND[family][figure] = max(8 x MEASURED, BAR): 8 is the convention of tests/_c51_ref.py, tests/_dqn_cases.py and tests/_ddqn_ref.py for "another f32 evaluation in
another summation order", BAR is _dqn_cases.BAR["dqn"] — gradient 1e-5 of max |g|, loss 2e-5 — and nothing for the other figures.  CLOSE_Q[family] = 2 x the
soft_value bound: the seeds keep the target network's two action values at every successor at least that far apart (the target_tie case aside, where they are equal
bit for bit).  CLOSE_CLIP[family] = 2 x the bonus bound: no row's tau ln pi_a lies that close to clip_lo (nor, in the clip family, to 0 unless it is exactly 0;
tests/_mdqn_cases.py says why only there).  MEASURED_CHAIN / BOUND_CHAIN: the same for the losses (relative) and the final parameters (absolute) of the 51 chained updates of chain().  No bound comes from the kernel's output.
"""
import numpy as np
import torch

import _ddqn_ref as DD
import _dqn_cases as D
from _c51_ref import results_dir  # noqa: F401  (the GPU tests write their maxima there)

f32 = np.float32
NP, H1, H2 = D.NP, D.H1, D.H2
VARIANTS = ("no_clip", "bonus_from_online", "bonus_at_successor", "hard_max", "entropy_sign_flipped", "bonus_masked_by_terminated")
FIGURES = ("target", "current", "bonus", "soft_value", "loss", "grad")
FAMILIES = ("plain", "clip", "tau_1", "tau_underflow", "alpha", "terminal", "gamma", "target_tie", "kink_placed", "ddqn_identity")
HP = dict(alpha=0.9, tau=0.03, clip_lo=-1.0)

# measured by tests/test_mdqn_cases_cpu.py: torch float32 against torch float64, maximum over the family's cases      (measured: the figure in the same position)
MEASURED = {
    "plain": dict(target=2.90e-07, current=2.20e-07, bonus=2.60e-07, soft_value=2.10e-07, loss=6.00e-08, grad=2.60e-07),   # 2.56e-07 1.98e-07 2.36e-07 1.87e-07 5.39e-08 2.33e-07
    "clip": dict(target=1.50e-06, current=3.00e-06, bonus=1.50e-06, soft_value=1.30e-06, loss=1.40e-07, grad=1.40e-07),   # 1.35e-06 2.68e-06 1.36e-06 1.19e-06 1.24e-07 1.26e-07
    "tau_1": dict(target=2.10e-07, current=1.70e-07, bonus=6.30e-08, soft_value=2.00e-07, loss=1.10e-07, grad=4.90e-07),   # 1.86e-07 1.55e-07 5.65e-08 1.77e-07 9.71e-08 4.34e-07
    "tau_underflow": dict(target=1.20e-07, current=1.10e-07, bonus=1.60e-07, soft_value=8.80e-08, loss=1.50e-07, grad=1.40e-07),   # 1.08e-07 9.86e-08 1.41e-07 7.86e-08 1.33e-07 1.28e-07
    "alpha": dict(target=1.10e-07, current=7.20e-08, bonus=8.20e-08, soft_value=1.30e-07, loss=8.90e-09, grad=1.80e-07),   # 1.02e-07 6.40e-08 7.31e-08 1.12e-07 7.97e-09 1.64e-07
    "terminal": dict(target=2.70e-07, current=1.20e-07, bonus=1.60e-07, soft_value=1.20e-07, loss=2.20e-08, grad=2.30e-07),   # 2.39e-07 1.05e-07 1.40e-07 1.06e-07 1.93e-08 2.09e-07
    "gamma": dict(target=2.50e-07, current=2.50e-07, bonus=2.10e-07, soft_value=1.60e-07, loss=1.50e-07, grad=2.80e-07),   # 2.26e-07 2.23e-07 1.90e-07 1.44e-07 1.30e-07 2.48e-07
    "target_tie": dict(target=1.60e-07, current=9.10e-08, bonus=1.00e-09, soft_value=9.20e-08, loss=1.50e-07, grad=1.60e-07),   # 1.46e-07 8.13e-08 8.94e-10 8.20e-08 1.31e-07 1.42e-07
    "kink_placed": dict(target=1.40e-07, current=1.50e-07, bonus=1.70e-07, soft_value=7.90e-08, loss=1.00e-07, grad=2.40e-07),   # 1.27e-07 1.38e-07 1.56e-07 7.03e-08 9.24e-08 2.11e-07
    "ddqn_identity": dict(target=1.40e-07, current=1.20e-07, bonus=1.70e-07, soft_value=1.20e-07, loss=6.80e-08, grad=3.10e-07),   # 1.24e-07 1.07e-07 1.56e-07 1.11e-07 6.09e-08 2.77e-07
}
MEASURED_CHAIN = dict(loss=3.3e-7, params=2.7e-7)                                                # 2.97e-7 2.39e-7
BAR = dict(loss=D.BAR["dqn"]["loss"], grad=D.BAR["dqn"]["grad"])
BOUND = {fam: {k: max(8.0 * v, BAR.get(k, 0.0)) for k, v in m.items()} for fam, m in MEASURED.items()}
BOUND_CHAIN = dict(loss=max(8.0 * MEASURED_CHAIN["loss"], BAR["loss"]), params=8.0 * MEASURED_CHAIN["params"])
CLOSE_Q = {fam: 2.0 * b["soft_value"] for fam, b in BOUND.items()}
CLOSE_CLIP = {fam: 2.0 * b["bonus"] for fam, b in BOUND.items()}
LR, ADAM_EPS, BETAS = DD.LR, DD.ADAM_EPS, DD.BETAS
_t, _dist, adam_step = DD._t, DD._dist, DD.adam_step


def forward(params, x, dtype=torch.float64):
    """-> Q [rows, 2] as float64 numpy"""
    return DD.forward(params, x, dtype)


def td_loss(p, target, ring, idx, gamma, dtype, hp=None, variant=None):
    """p: the online vector as a torch tensor (requires_grad for a gradient); ring = dict(observations [S][N][4], actions, rewards, terminated [S][N]); hp =
    dict(alpha, tau, clip_lo) -> (loss, dict of the intermediate torch tensors)"""
    assert variant is None or variant in VARIANTS
    hp = dict(HP, **(hp or {}))
    alpha, tau, clip_lo = (float(f32(hp[k])) for k in ("alpha", "tau", "clip_lo"))
    S, N = ring["actions"].shape
    idx = np.asarray(idx, np.int64)
    nx = D.successor(idx, N, S)
    flat = lambda k: ring[k].reshape((N * S,) + ring[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    rows = torch.arange(len(idx))
    acts = torch.from_numpy(flat("actions")[idx])
    with torch.no_grad():
        xi, xn, tg = _t(obs[idx], dtype), _t(obs[nx], dtype), _t(target, dtype)
        qt_next, _, _ = D.q_values(tg, xn, "dqn")
        if variant == "bonus_from_online":
            qt_row = D.q_values(p.detach(), xi, "dqn")[0]
        elif variant == "bonus_at_successor":
            qt_row = qt_next
        else:
            qt_row = D.q_values(tg, xi, "dqn")[0]
        slp = tau * torch.log_softmax(qt_row / tau, dim=1)[rows, acts]
        bonus = slp if variant == "no_clip" else torch.clamp(slp, clip_lo, 0.0)
        pi, lp = torch.softmax(qt_next / tau, dim=1), torch.log_softmax(qt_next / tau, dim=1)
        if variant == "hard_max":
            soft = qt_next.max(dim=1).values
        elif variant == "entropy_sign_flipped":
            soft = (pi * (qt_next + tau * lp)).sum(dim=1)
        else:
            soft = (pi * (qt_next - tau * lp)).sum(dim=1)
        r = _t(flat("rewards")[nx], dtype)
        live = _t(1.0 - flat("terminated")[nx].astype(np.float64), dtype)
        used = bonus * live if variant == "bonus_masked_by_terminated" else bonus
        tgt = r + alpha * used + float(f32(gamma)) * soft * live
        a_next = torch.argmax(qt_next, dim=1)
    q, z1, z2 = D.q_values(p, xi, "dqn")
    old = q[rows, acts]
    loss = ((tgt - old) ** 2).mean()
    return loss, dict(next_actions=a_next, target=tgt, current=old, bonus=bonus, slp=slp, soft_value=soft, q_row=q, qt_row=qt_row, qt_next=qt_next, live=live, z1=z1, z2=z2)


def evaluate(c, dtype=torch.float64, variant=None, target=None):
    """a case of tests/_mdqn_cases.py -> dict(grads, loss, next_actions, target, current, bonus, slp, soft_value, q_row, qt_row, qt_next, live, z1, z2) as float64 /
    int64 numpy"""
    p = _t(c["params"], dtype, True)
    loss, aux = td_loss(p, c["target"] if target is None else target, c, c["idx"], c["gamma"], dtype, c["hp"], variant)
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    out = {k: d(v) for k, v in aux.items() if k != "next_actions"}
    out.update(grads=d(p.grad), loss=float(loss.item()), next_actions=aux["next_actions"].numpy().astype(np.int64))
    return out


def figures(exp, got, family=None):
    """exp: evaluate()'s float64 result; got: grads, loss, target, current, bonus, soft_value from another evaluation or the device"""
    f = {k: _dist(got[k], exp[k]) for k in ("target", "current", "bonus", "soft_value")}
    f["loss"] = _dist([got["loss"]], [exp["loss"]]) / abs(exp["loss"])
    f["grad"] = _dist(got["grads"], exp["grads"]) / float(np.abs(exp["grads"]).max())
    return f


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def chain(ring, indices, params, target, dtype=torch.float64, sync_after=25, gamma=0.99, hp=None):
    """len(indices) updates chained through Adam from zero moments, the target network synced behind update `sync_after` -> (losses [n], final parameters) float64"""
    p = _t(params, dtype, True)
    tgt = _t(target, dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = []
    for k, idx in enumerate(indices):
        p.grad = None
        loss, _ = td_loss(p, tgt, ring, idx, gamma, dtype, hp)
        loss.backward()
        losses.append(float(loss.item()))
        with torch.no_grad():
            adam_step(p, p.grad, m, v, k + 1)
            if k == sync_after:
                tgt = p.detach().clone()
    return np.array(losses, np.float64), p.detach().numpy().astype(np.float64)


CHAIN_UPDATES, CHAIN_BATCH, CHAIN_STEPS = DD.CHAIN_UPDATES, DD.CHAIN_BATCH, DD.CHAIN_STEPS
chain_data = DD.chain_data   # the ring and the indices of the Double DQN chain, built on the CPU
