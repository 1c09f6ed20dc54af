"""torch restatement of the Double DQN target, loss and gradient (include/mi_ddqn.h) — TEST INFRASTRUCTURE (tests/test_ddqn_cases_cpu.py validates and measures it,
the GPU tests use it).

The reference has no double_dqn.py.  This is dqn.py's TD update with the target replaced, on the [slots][N] time-major ring of the engines, in float64 or float32:
    nx = ((i // N + 1) % slots) * N + i % N
    a* = argmax_a Q_online(obs[nx])                              (torch.argmax: the first index on a tie)
    target = r[nx] + f32(gamma) Q_target(obs[nx])[a*] (1 - terminated[nx])          under no_grad
    old = Q_online(obs[i])[a[i]];  loss = mean((target - old)^2)
AUTOGRAD produces every gradient — there is no hand-written backward in this file, which is what makes it independent of ddqn_grad_kernel
(deep_rl_amd/csrc/mi_ddqn.hip) and of oracle/cpu_ref.c, which derive the backward by hand.  The network, the flat layout and the successor rule are
tests/_dqn_cases.py's (features, q_values, successor), imported unchanged.

`variant=` names a deliberately WRONG reading, used only by the CPU test to show that the cases tell it from the right one:
  dqn_max            the target network's own maximum (plain DQN)
  value_from_online  the online network's value of a* (no target network at all)
  argmax_at_row      a* from obs[i] instead of obs[nx]
  tie_takes_last     a* = 1 on a bit-for-bit tie

Figures (figures()).  "q": max |q - q64| over the online values at obs[i] and obs[nx] and the target values at obs[nx], absolute.  "target", "current": max |x - x64|,
absolute — in the scale family relative to max |target64|.  "loss": |x - ref| / |ref|.  "grad": max |g - ref| / max |ref|.  A NaN where the reference is finite
makes the figure inf.  The device writes no action values out: its "q" figure is the forward API's on the case's observations.

Bounds.  MEASURED[family][figure] is what tests/test_ddqn_cases_cpu.py measures for the FLOAT32 torch evaluation of these same formulas against the float64 one,
the maximum over the family's cases (the test ties the constants to the measurement: the constant covers the measured figure and is at most 1.25 x it).
BOUND[family][figure] = max(8 x MEASURED, BAR): 8 is the convention of tests/_c51_ref.py and tests/_dqn_cases.py for "another f32 evaluation in another summation
order", BAR is _dqn_cases.BAR["dqn"] — gradient 1e-5 of max |g|, loss 2e-5 — and nothing for the figures the suite holds DQN to no bar on.  CLOSE_Q[family] = 2 x the
q bound: the cases' seeds keep the online network's two action values at every successor at least that far apart (the online_tie case aside, where they are equal
bit for bit), so no row is left out of any comparison.  MEASURED_CHAIN / BOUND_CHAIN: the same for the losses (relative) and the final parameters (absolute) of
the 51 chained updates of chain().  No bound comes from the kernel's output.
"""
import numpy as np
import torch

import _dqn_cases as D
from _c51_ref import results_dir  # noqa: F401  (the GPU tests write their maxima there)

f32 = np.float32
NP, H1, H2 = D.NP, D.H1, D.H2
VARIANTS = ("dqn_max", "value_from_online", "argmax_at_row", "tie_takes_last")
FIGURES = ("q", "target", "current", "loss", "grad")
FAMILIES = ("plain", "synced", "online_tie", "terminal", "gamma", "scale", "kink_placed")

# measured by tests/test_ddqn_cases_cpu.py: torch float32 against torch float64, maximum over the family's cases      (measured: the figure in the same position)
MEASURED = {
    "plain": dict(q=3.2e-7, target=2.1e-7, current=2.7e-7, loss=2.1e-7, grad=2.7e-7),            # 2.84e-7 1.88e-7 2.39e-7 1.87e-7 2.43e-7
    "synced": dict(q=1.6e-7, target=1.5e-7, current=8.2e-8, loss=7.8e-8, grad=1.3e-7),           # 1.40e-7 1.36e-7 7.39e-8 7.08e-8 1.17e-7
    "online_tie": dict(q=1.1e-7, target=9.9e-8, current=1.1e-7, loss=1.2e-7, grad=2.3e-7),       # 1.00e-7 8.94e-8 1.00e-7 1.01e-7 2.06e-7
    "terminal": dict(q=1.3e-7, target=1.1e-7, current=1.1e-7, loss=9.8e-8, grad=2.3e-7),         # 1.11e-7 9.61e-8 9.86e-8 8.86e-8 2.01e-7
    "gamma": dict(q=2.0e-7, target=1.2e-7, current=1.1e-7, loss=7.1e-8, grad=3.2e-7),            # 1.82e-7 1.07e-7 1.02e-7 6.38e-8 2.89e-7
    "scale": dict(q=3.9e-6, target=2.4e-7, current=2.3e-7, loss=3.8e-9, grad=2.3e-7),            # 3.54e-6 2.16e-7 2.09e-7 3.43e-9 2.05e-7
    "kink_placed": dict(q=2.5e-7, target=1.25e-7, current=4.5e-8, loss=1.15e-8, grad=1.45e-7),   # 2.23e-7 1.12e-7 4.07e-8 1.04e-8 1.31e-7
}
MEASURED_CHAIN = dict(loss=3.3e-7, params=5.1e-7)                                                # 2.95e-7 4.59e-7
BAR = dict(loss=D.BAR["dqn"]["loss"], grad=D.BAR["dqn"]["grad"])
BOUND = {fam: {k: max(8.0 * v, BAR.get(k, 0.0)) for k, v in m.items()} for fam, m in MEASURED.items()}
BOUND_CHAIN = dict(loss=max(8.0 * MEASURED_CHAIN["loss"], BAR["loss"]), params=8.0 * MEASURED_CHAIN["params"])
CLOSE_Q = {fam: 2.0 * b["q"] for fam, b in BOUND.items()}
LR, ADAM_EPS, BETAS = 2.5e-4, 1e-8, (0.9, 0.999)


def _t(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def forward(params, x, dtype=torch.float64):
    """-> Q [rows, 2] as float64 numpy"""
    with torch.no_grad():
        q, _, _ = D.q_values(_t(params, dtype), _t(np.asarray(x).reshape(-1, 4), dtype), "dqn")
    return q.numpy().astype(np.float64)


def td_loss(p, target, ring, idx, gamma, dtype, variant=None):
    """p: the online vector as a torch tensor (requires_grad for a gradient); ring = dict(observations [S][N][4], actions, rewards, terminated [S][N])
    -> (loss, dict of the intermediate torch tensors)"""
    assert variant is None or variant in VARIANTS
    S, N = ring["actions"].shape
    idx = np.asarray(idx, np.int64)
    nx = D.successor(idx, N, S)
    flat = lambda k: ring[k].reshape((N * S,) + ring[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    with torch.no_grad():
        xn = _t(obs[nx], dtype)
        qn, _, _ = D.q_values(p.detach(), _t(obs[idx], dtype) if variant == "argmax_at_row" else xn, "dqn")
        qt, _, _ = D.q_values(_t(target, dtype), xn, "dqn")
        a_star = (qn[:, 1] >= qn[:, 0]).long() if variant == "tie_takes_last" else torch.argmax(qn, dim=1)
        rows = torch.arange(len(idx))
        if variant == "dqn_max":
            value = qt.max(dim=1).values
        elif variant == "value_from_online":
            value = D.q_values(p.detach(), xn, "dqn")[0][rows, a_star]
        else:
            value = qt[rows, a_star]
        r = _t(flat("rewards")[nx], dtype)
        live = _t(1.0 - flat("terminated")[nx].astype(np.float64), dtype)
        tgt = r + float(f32(gamma)) * value * live
    q, z1, z2 = D.q_values(p, _t(obs[idx], dtype), "dqn")
    old = q[rows, torch.from_numpy(flat("actions")[idx])]
    loss = ((tgt - old) ** 2).mean()
    return loss, dict(next_actions=a_star, target=tgt, current=old, q_row=q, q_next=qn, q_target=qt, live=live, z1=z1, z2=z2)


def evaluate(c, dtype=torch.float64, variant=None, target=None):
    """a case of tests/_ddqn_cases.py -> dict(grads, loss, next_actions, target, current, q_row, q_next, q_target, live, z1, z2) as float64 / int64 numpy"""
    p = _t(c["params"], dtype, True)
    loss, aux = td_loss(p, c["target"] if target is None else target, c, c["idx"], c["gamma"], dtype, variant)
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    out = {k: d(v) for k, v in aux.items() if k != "next_actions"}
    out.update(grads=d(p.grad), loss=float(loss.item()), next_actions=aux["next_actions"].numpy().astype(np.int64))
    return out


def _dist(g, r):
    g, r = np.asarray(g, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    assert np.isfinite(r).all(), "the float64 reference itself is not finite"
    return float(np.abs(g - r).max()) if np.isfinite(g).all() else np.inf


def figures(exp, got, family):
    """exp: evaluate()'s float64 result; got: grads, loss, target, current (and q_row, q_next, q_target, or "q" / "q_ref" pairs) from another evaluation or the device"""
    f = {}
    scale = float(np.abs(exp["target"]).max()) if family == "scale" else 1.0
    f["target"] = _dist(got["target"], exp["target"]) / scale
    f["current"] = _dist(got["current"], exp["current"]) / scale
    f["loss"] = _dist([got["loss"]], [exp["loss"]]) / abs(exp["loss"])
    top = float(np.abs(exp["grads"]).max())
    f["grad"] = _dist(got["grads"], exp["grads"]) / top
    if "q_row" in got:
        f["q"] = max(_dist(got[k], exp[k]) for k in ("q_row", "q_next", "q_target"))
    elif "q" in got:
        f["q"] = _dist(got["q"], got["q_ref"])
    return f


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def adam_step(p, g, m, v, step, lr=LR, betas=BETAS, eps=ADAM_EPS):
    """torch's single-tensor Adam on numpy float64 (or torch tensors of any dtype), in place; step is 1-based"""
    b1, b2 = betas
    m *= b1; m += (1 - b1) * g
    v *= b2; v += (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p -= (lr / bc1) * m / (v ** 0.5 / bc2 ** 0.5 + eps)


def chain(ring, indices, params, target, dtype=torch.float64, sync_after=25, gamma=0.99):
    """len(indices) updates chained through Adam from zero moments, the target network synced behind update `sync_after` -> (losses [n], final parameters) float64"""
    p = _t(params, dtype, True)
    tgt = _t(target, dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = []
    for k, idx in enumerate(indices):
        p.grad = None
        loss, _ = td_loss(p, tgt, ring, idx, gamma, dtype)
        loss.backward()
        losses.append(float(loss.item()))
        with torch.no_grad():
            adam_step(p, p.grad, m, v, k + 1)
            if k == sync_after:
                tgt = p.detach().clone()
    return np.array(losses, np.float64), p.detach().numpy().astype(np.float64)


CHAIN_STEPS, CHAIN_UPDATES, CHAIN_BATCH, CHAIN_SEED, CHAIN_LS = 600, 51, 128, 7, 100


def chain_data(R):
    """the ring and the batches of the chained-update test, built on the CPU alone (R = oracle.cpu_ref): N = 1, 600 keyed steps under fixed parameters (the keyed
    random action before step 100, epsilon-greedy after it), slots = 601; the indices are R.dqn_sample's -> (ring, indices [51][128], params, target)"""
    rng = np.random.default_rng(CHAIN_SEED)
    params, target = D.init_params(rng)[0], D.init_params(rng)[0]
    R.set_sincos_mode("fdlibm")
    try:
        env = R.VecCartPole(1, seed=CHAIN_SEED)
        st = R.ReplayStorage(CHAIN_STEPS + 1, 1)
        obs_cur = env.reset(); st.observations[0] = obs_cur
        for g in range(0, CHAIN_STEPS, 50):
            R.dqn_act_steps(env, params, st, obs_cur, 50, g, learning_starts=CHAIN_LS, total_timesteps=CHAIN_STEPS)
    finally:
        R.set_sincos_mode("libm")
    ring = dict(observations=st.observations.copy(), actions=st.actions.copy(), rewards=st.rewards.copy(), terminated=st.terminated.copy())
    indices = np.stack([R.dqn_sample(CHAIN_SEED, k, CHAIN_STEPS, CHAIN_BATCH) for k in range(CHAIN_UPDATES)])
    return ring, indices, params, target
