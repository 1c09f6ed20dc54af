"""torch restatement of the prioritized dueling Double DQN target, loss and gradient (include/mi_pdd.h) — TEST INFRASTRUCTURE (tests/test_pdd_cases_cpu.py validates
and measures it, the GPU tests use it).

The reference has no script that combines the three.  This is dqn.py's TD update on the [slots][N] time-major ring of the engines, in float64 or float32, with the
dueling network of dueling_dqn.py:36-40, the double target and per.py's weighted loss:
    nx = ((i // N + 1) % slots) * N + i % N
    Q(x) = value(h) + (adv(h) - adv(h).mean over the two actions of each row),  h = features(x)
    a* = argmax_a Q_online(obs[nx])                              (torch.argmax: the first index on a tie)
    target = r[nx] + f32(gamma) Q_target(obs[nx])[a*] (1 - terminated[nx])          under no_grad
    old = Q_online(obs[i])[a[i]];  td = target - old;  loss = mean(w td^2), w = 1 without weights;  td_abs = |td| (unweighted)
AUTOGRAD produces every gradient — there is no hand-written backward in this file, which is what makes it independent of pdd_grad_kernel
(deep_rl_amd/csrc/mi_pdd.hip).  The network, the flat 11,019-element layout and the successor rule are tests/_dqn_cases.py's (features, q_values kind "dueling",
successor), imported unchanged.

`variant=` names a deliberately WRONG reading, used only by the CPU test to show that the cases tell it from the right one:
  dqn_max            the target network's own maximum (no double target)
  value_from_online  the online network's value of a* (no target network at all)
  argmax_at_row      a* from obs[i] instead of obs[nx]
  mean_over_batch    the advantage mean taken over the whole batch (adv.mean()) instead of over the two actions of each row
  weights_ignored    w = 1 whatever the weights are
  weight_squared     (w td)^2
  td_abs_weighted    td_abs = |w td| (this one moves no gradient: it is told apart by the td_abs figure)

Figures (figures()).  "q": max |q - q64| over the online values at obs[i] and obs[nx] and the target values at obs[nx], absolute.  "target", "current", "td_abs":
max |x - x64|, absolute — in the scale family relative to max |target64|.  "loss": |x - ref| / |ref|.  "grad": max |g - ref| / max |ref|.  A NaN where the reference
is finite makes the figure inf.  The device writes no action values out: its "q" figure is the forward API's on the case's observations.

Bounds.  MEASURED[family][figure] is what tests/test_pdd_cases_cpu.py measures for the FLOAT32 torch evaluation of these same formulas against the float64 one, the
maximum over the family's cases (the test ties the constants to the measurement: the constant covers the measured figure and is at most 1.25 x it).
BOUND[family][figure] = max(8 x MEASURED, BAR): 8 is the convention of tests/_c51_ref.py, tests/_dqn_cases.py and tests/_ddqn_ref.py for "another f32 evaluation in
another summation order", BAR is _dqn_cases.BAR["dqn"] — gradient 1e-5 of max |g|, loss 2e-5 — and nothing for q, target, current and td_abs.  CLOSE_Q[family] = 2 x
the q bound: the cases' seeds keep the online network's two action values at every successor at least that far apart (the tie cases aside, where they are equal bit
for bit), so no row is left out of any comparison.  MEASURED_CHAIN / BOUND_CHAIN: the same for the losses (relative) and the final parameters (absolute) of the 51
chained weighted updates of chain().  No bound comes from the kernel's output.
"""
import numpy as np
import torch

import _ddqn_ref as DD
import _dqn_cases as D
from _c51_ref import results_dir  # noqa: F401  (the GPU tests write their maxima there)

f32 = np.float32
NP, H1, H2 = D.DNP, D.H1, D.H2
VARIANTS = ("dqn_max", "value_from_online", "argmax_at_row", "mean_over_batch", "weights_ignored", "weight_squared", "td_abs_weighted")
FIGURES = ("q", "target", "current", "td_abs", "loss", "grad")
FAMILIES = ("plain", "weights", "synced", "online_tie", "terminal", "gamma", "scale", "adv_tie", "kink_placed")

# measured by tests/test_pdd_cases_cpu.py: torch float32 against torch float64, maximum over the family's cases      (measured: the figure in the same position)
MEASURED = {
    "plain": dict(q=3.2e-7, target=1.6e-7, current=3.2e-7, td_abs=3.4e-7, loss=3.3e-7, grad=4.2e-7),              # 2.86e-7 1.41e-7 2.86e-7 3.01e-7 2.92e-7 3.80e-7
    "weights": dict(q=2.7e-7, target=2.4e-7, current=2.0e-7, td_abs=2.9e-7, loss=1.4e-7, grad=2.9e-7),            # 2.41e-7 2.10e-7 1.76e-7 2.55e-7 1.26e-7 2.58e-7
    "synced": dict(q=1.6e-7, target=1.5e-7, current=1.4e-7, td_abs=2.1e-7, loss=8.4e-8, grad=9.9e-8),             # 1.40e-7 1.32e-7 1.24e-7 1.91e-7 7.59e-8 8.94e-8
    "online_tie": dict(q=1.03e-7, target=9.4e-8, current=8.1e-8, td_abs=1.4e-7, loss=1.7e-7, grad=2.0e-7),        # 9.32e-8 8.48e-8 7.29e-8 1.27e-7 1.50e-7 1.75e-7
    "terminal": dict(q=2.5e-7, target=2.6e-7, current=1.8e-7, td_abs=3.1e-7, loss=1.8e-7, grad=2.5e-7),           # 2.19e-7 2.33e-7 1.63e-7 2.76e-7 1.63e-7 2.22e-7
    "gamma": dict(q=1.9e-7, target=9.3e-8, current=1.5e-7, td_abs=2.0e-7, loss=6.4e-8, grad=4.3e-7),              # 1.69e-7 8.43e-8 1.32e-7 1.77e-7 5.74e-8 3.83e-7
    "scale": dict(q=5.6e-6, target=1.2e-7, current=2.2e-7, td_abs=2.1e-7, loss=5.9e-8, grad=2.6e-7),              # 5.05e-6 1.04e-7 1.99e-7 1.84e-7 5.33e-8 2.29e-7
    "adv_tie": dict(q=1.3e-7, target=8.4e-8, current=7.7e-8, td_abs=9.2e-8, loss=1.3e-7, grad=1.9e-7),            # 1.09e-7 7.59e-8 6.98e-8 8.28e-8 1.13e-7 1.70e-7
    "kink_placed": dict(q=1.5e-7, target=5.4e-8, current=1.3e-7, td_abs=9.7e-8, loss=2.0e-7, grad=3.9e-7),        # 1.34e-7 4.82e-8 1.14e-7 8.81e-8 1.76e-7 3.54e-7
}
MEASURED_CHAIN = dict(loss=4.8e-7, params=2.9e-7)                                                                 # 4.38e-7 2.60e-7
BAR = dict(loss=D.BAR["dqn"]["loss"], grad=D.BAR["dqn"]["grad"])
BOUND = {fam: {k: max(8.0 * v, BAR.get(k, 0.0)) for k, v in m.items()} for fam, m in MEASURED.items()}
BOUND_CHAIN = dict(loss=max(8.0 * MEASURED_CHAIN["loss"], BAR["loss"]), params=8.0 * MEASURED_CHAIN["params"])
CLOSE_Q = {fam: 2.0 * b["q"] for fam, b in BOUND.items()}
LR, ADAM_EPS, BETAS = DD.LR, DD.ADAM_EPS, DD.BETAS
adam_step = DD.adam_step


def _t(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def q_values(p, x, variant=None):
    """-> (Q [rows, 2], z1, z2) of the dueling vector p"""
    if variant != "mean_over_batch":
        return D.q_values(p, x, "dueling")
    h2, z1, z2 = D.features(p, x)
    s = lambda k, shape: p[D.DUEL[k][0]:D.DUEL[k][1]].reshape(shape)   # noqa: E731
    adv = h2 @ s("Wa", (2, H2)).T + s("ba", (2,))
    return (h2 @ s("Wv", (1, H2)).T + s("bv", (1,))) + (adv - adv.mean()), z1, z2


def forward(params, x, dtype=torch.float64):
    """-> Q [rows, 2] as float64 numpy"""
    with torch.no_grad():
        q, _, _ = q_values(_t(params, dtype), _t(np.asarray(x).reshape(-1, 4), dtype))
    return q.numpy().astype(np.float64)


def td_loss(p, target, ring, idx, gamma, weights, dtype, variant=None):
    """p: the online vector as a torch tensor (requires_grad for a gradient); ring = dict(observations [S][N][4], actions, rewards, terminated [S][N]); weights: [batch]
    or None -> (loss, dict of the intermediate torch tensors)"""
    assert variant is None or variant in VARIANTS
    S, N = ring["actions"].shape
    idx = np.asarray(idx, np.int64)
    nx = D.successor(idx, N, S)
    flat = lambda k: ring[k].reshape((N * S,) + ring[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    with torch.no_grad():
        xn = _t(obs[nx], dtype)
        qn, _, _ = q_values(p.detach(), _t(obs[idx], dtype) if variant == "argmax_at_row" else xn, variant)
        qt, _, _ = q_values(_t(target, dtype), xn, variant)
        a_star = torch.argmax(qn, dim=1)
        rows = torch.arange(len(idx))
        if variant == "dqn_max":
            value = qt.max(dim=1).values
        elif variant == "value_from_online":
            value = q_values(p.detach(), xn, variant)[0][rows, a_star]
        else:
            value = qt[rows, a_star]
        r = _t(flat("rewards")[nx], dtype)
        live = _t(1.0 - flat("terminated")[nx].astype(np.float64), dtype)
        tgt = r + float(f32(gamma)) * value * live
        w = torch.ones(len(idx), dtype=dtype) if weights is None or variant == "weights_ignored" else _t(np.asarray(weights, f32), dtype)
    q, z1, z2 = q_values(p, _t(obs[idx], dtype), variant)
    old = q[rows, torch.from_numpy(flat("actions")[idx])]
    td = tgt - old
    loss = ((w * td) ** 2).mean() if variant == "weight_squared" else (w * td ** 2).mean()
    td_abs = (w * td).detach().abs() if variant == "td_abs_weighted" else td.detach().abs()
    return loss, dict(next_actions=a_star, target=tgt, current=old, td_abs=td_abs, q_row=q, q_next=qn, q_target=qt, live=live, z1=z1, z2=z2)


def evaluate(c, dtype=torch.float64, variant=None, target=None):
    """a case of tests/_pdd_cases.py -> dict(grads, loss, next_actions, target, current, td_abs, q_row, q_next, q_target, live, z1, z2) as float64 / int64 numpy"""
    p = _t(c["params"], dtype, True)
    loss, aux = td_loss(p, c["target"] if target is None else target, c, c["idx"], c["gamma"], c["weights"], dtype, variant)
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    out = {k: d(v) for k, v in aux.items() if k != "next_actions"}
    out.update(grads=d(p.grad), loss=float(loss.item()), next_actions=aux["next_actions"].numpy().astype(np.int64))
    return out


_dist = DD._dist


def figures(exp, got, family):
    """exp: evaluate()'s float64 result; got: grads, loss, target, current, td_abs (and q_row, q_next, q_target, or "q" / "q_ref" pairs) from another evaluation or
    the device"""
    f = {}
    scale = float(np.abs(exp["target"]).max()) if family == "scale" else 1.0
    for k in ("target", "current", "td_abs"):
        f[k] = _dist(got[k], exp[k]) / scale
    f["loss"] = _dist([got["loss"]], [exp["loss"]]) / abs(exp["loss"])
    f["grad"] = _dist(got["grads"], exp["grads"]) / float(np.abs(exp["grads"]).max())
    if "q_row" in got:
        f["q"] = max(_dist(got[k], exp[k]) for k in ("q_row", "q_next", "q_target"))
    elif "q" in got:
        f["q"] = _dist(got["q"], got["q_ref"])
    return f


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def chain(ring, indices, weights, params, target, dtype=torch.float64, sync_after=25, gamma=0.99):
    """len(indices) weighted updates chained through Adam from zero moments, the target network synced behind update `sync_after`
    -> (losses [n], final parameters) float64"""
    p = _t(params, dtype, True)
    tgt = _t(target, dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = []
    for k, idx in enumerate(indices):
        p.grad = None
        loss, _ = td_loss(p, tgt, ring, idx, gamma, weights[k], dtype)
        loss.backward()
        losses.append(float(loss.item()))
        with torch.no_grad():
            adam_step(p, p.grad, m, v, k + 1)
            if k == sync_after:
                tgt = p.detach().clone()
    return np.array(losses, np.float64), p.detach().numpy().astype(np.float64)


CHAIN_STEPS, CHAIN_UPDATES, CHAIN_BATCH, CHAIN_SEED = DD.CHAIN_STEPS, DD.CHAIN_UPDATES, DD.CHAIN_BATCH, DD.CHAIN_SEED


def chain_data(R):
    """the ring of the chained-update tests, built on the CPU alone (R = oracle.cpu_ref): _ddqn_ref.chain_data's ring and uniform batches, two independently drawn
    dueling vectors, and placed weights for the CPU measurement (U(0.05, 1) as f32, the largest of each batch set to 1 — what an importance weight looks like; the
    GPU test feeds the float64 chain the device's own indices and weights instead) -> (ring, indices [51][128], weights [51][128], params, target)"""
    ring, indices, _, _ = DD.chain_data(R)
    rng = np.random.default_rng([CHAIN_SEED, 2016])
    params, target = D.init_params(rng)[1], D.init_params(rng)[1]
    weights = rng.uniform(0.05, 1.0, indices.shape).astype(f32)
    weights[np.arange(len(weights)), weights.argmax(axis=1)] = 1.0
    return ring, indices, weights, params, target
