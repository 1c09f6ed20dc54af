"""torch restatement of the n-step prioritized dueling Double DQN target, loss and gradient (include/mi_nstep.h) — TEST INFRASTRUCTURE (tests/test_nstep_cases_cpu.py
validates and measures it, the GPU tests use it).

The reference has no script with multi-step returns.  This is tests/_pdd_ref.py's TD update with one change, the target: the walk along the [slots][N] ring is a
plain Python loop over the rows, one step at a time, exactly as the header writes it —
    s_1 = succ(s_0); R = r[s_1]; g = gamma; m = 1
    while m < n and not terminated[s_m] and s_m != H:  m += 1; s_m = succ(s_{m-1}); R = R + g r[s_m]; g = g gamma
    lg = 0 if terminated[s_m] else g
    a* = argmax_a Q_online(obs[s_m]);  target = R + lg Q_target(obs[s_m])[a*]          under no_grad
    old = Q_online(obs[i])[a[i]];  td = target - old;  loss = mean(w td^2), w = 1 without weights;  td_abs = |td| (unweighted);  horizon = m
— in float64 or in float32 (numpy scalars of the dtype: every product and every sum rounds once, nothing fused), with gamma the float32 the device holds.  The walk
READS only what it uses: a cell beyond the stop is never touched, so it may hold NaN.  AUTOGRAD produces every gradient.  The network is _pdd_ref.q_values, imported.

`variant=` names a deliberately WRONG reading, used only by the CPU test to show that the cases tell it from the right one:
  one_step              n = 1 whatever n_step says
  through_termination   a terminated step does not end the walk (the last step's flag alone decides the bootstrap)
  across_head           the head does not end the walk
  gamma_n_always        the bootstrap is weighted gamma ** n after a shorter walk too
  bootstrap_at_n        obs[s_n] instead of obs[s_m]
  undiscounted_rewards  R = r_1 + r_2 + ... (the bootstrap keeps its gamma ** m)
  mask_by_multiply      all n rewards are read and those beyond the stop multiplied by 0

Figures: _pdd_ref.figures, unchanged ("q" over the online values at obs[i] and obs[s_m] and the target values at obs[s_m]).  horizon and next_actions are compared
exactly, never through a figure.

Bounds, by the rule of _pdd_ref.py with no new number.  MEASURED[family][figure] is what tests/test_nstep_cases_cpu.py measures for the FLOAT32 evaluation of these
same formulas against the float64 one, the maximum over the family's cases (the test ties the constants to the measurement: the constant covers the measured figure
and is at most 1.25 x it).  BOUND[family][figure] = max(8 x MEASURED, BAR), BAR = _dqn_cases.BAR["dqn"] (gradient 1e-5 of max |g|, loss 2e-5; nothing for q, target,
current, td_abs).  CLOSE_Q[family] = 2 x the q bound: the cases' seeds keep the online network's two action values at EVERY bootstrap observation at least that far
apart, so no row is left out of any comparison.  MEASURED_CHAIN / BOUND_CHAIN: the same for the 51 chained updates of chain().  No bound comes from the kernel's
output.
"""
import numpy as np
import torch

import _dqn_cases as D
import _pdd_ref as P
from _c51_ref import results_dir  # noqa: F401  (the GPU tests write their maxima there)

f32 = np.float32
NP, H1, H2 = P.NP, P.H1, P.H2
MAX_N = 16
VARIANTS = ("one_step", "through_termination", "across_head", "gamma_n_always", "bootstrap_at_n", "undiscounted_rewards", "mask_by_multiply")
FIGURES = P.FIGURES
FAMILIES = ("plain", "weights", "synced", "gamma", "scale", "kink_placed")

# measured by tests/test_nstep_cases_cpu.py: torch float32 against torch float64, maximum over the family's cases      (measured: the figure in the same position)
MEASURED = {
    "plain": dict(q=3.5e-07, target=1.2e-06, current=2.3e-07, td_abs=1.2e-06, loss=2.1e-07, grad=5.6e-07),            # 3.17e-07 1.06e-06 2.03e-07 1.09e-06 1.88e-07 5.08e-07
    "weights": dict(q=2.1e-07, target=2.4e-07, current=2.1e-07, td_abs=3.6e-07, loss=6.1e-08, grad=2.2e-07),          # 1.86e-07 2.18e-07 1.86e-07 3.20e-07 5.50e-08 2.00e-07
    "synced": dict(q=1.9e-07, target=2.1e-07, current=1.3e-07, td_abs=3.2e-07, loss=1.04e-07, grad=1e-07),            # 1.72e-07 1.82e-07 1.11e-07 2.84e-07 9.38e-08 9.00e-08
    "gamma": dict(q=1.9e-07, target=2.7e-07, current=1.3e-07, td_abs=1.5e-07, loss=1.2e-07, grad=2.3e-07),            # 1.72e-07 2.38e-07 1.14e-07 1.33e-07 1.07e-07 2.07e-07
    "scale": dict(q=7.2e-06, target=1.3e-07, current=1.3e-07, td_abs=1.3e-07, loss=6.5e-08, grad=1.1e-07),            # 6.54e-06 1.16e-07 1.18e-07 1.12e-07 5.89e-08 9.95e-08
    "kink_placed": dict(q=2.5e-07, target=1.6e-07, current=9.9e-08, td_abs=2.5e-07, loss=3e-08, grad=2.7e-07),        # 2.22e-07 1.40e-07 8.98e-08 2.22e-07 2.68e-08 2.37e-07
}
MEASURED_CHAIN = dict(loss=1.7e-07, params=2.2e-07)                                                                   # 1.46e-07 1.99e-07
BAR = dict(loss=D.BAR["dqn"]["loss"], grad=D.BAR["dqn"]["grad"])
BOUND = {fam: {k: max(8.0 * v, BAR.get(k, 0.0)) for k, v in m.items()} for fam, m in MEASURED.items()}
BOUND_CHAIN = dict(loss=max(8.0 * MEASURED_CHAIN["loss"], BAR["loss"]), params=8.0 * MEASURED_CHAIN["params"])
CLOSE_Q = {fam: 2.0 * b["q"] for fam, b in BOUND.items()}
LR, ADAM_EPS, BETAS = P.LR, P.ADAM_EPS, P.BETAS
adam_step = P.adam_step
_t = P._t
q_values = P.q_values
figures = P.figures


def walk(ring, idx, n_step, head, gamma, np_dtype=np.float64, variant=None):
    """the walk of every row of idx, one row and one step at a time -> (at [rows] flat index of s_m, R [rows], lg [rows], m [rows]); R and lg in np_dtype"""
    assert variant is None or variant in VARIANTS
    S, N = ring["actions"].shape
    assert 1 <= n_step <= MAX_N and n_step < S and 0 <= head < S
    rew, term = ring["rewards"], ring["terminated"]
    T = np_dtype
    gam = T(f32(gamma))
    n = 1 if variant == "one_step" else int(n_step)
    at, Rs, lgs, ms = [], [], [], []
    for i in np.asarray(idx, np.int64).tolist():
        s, e = i // N, i % N
        s = (s + 1) % S
        R, g, m = T(rew[s, e]), gam, 1
        if variant == "mask_by_multiply":
            alive, sk, gk = T(1), s, gam
            for _ in range(1, n):
                if term[sk, e] or sk == head:
                    alive = T(0)
                sk = (sk + 1) % S
                R = T(R + T(T(gk * T(rew[sk, e])) * alive))
                gk = T(gk * gam)
        while m < n and (variant == "through_termination" or not term[s, e]) and (variant == "across_head" or s != head):
            m += 1
            s = (s + 1) % S
            if variant == "undiscounted_rewards":
                R = T(R + T(rew[s, e]))
            elif variant != "mask_by_multiply":
                R = T(R + T(g * T(rew[s, e])))
            g = T(g * gam)
        if variant == "gamma_n_always":
            g = gam
            for _ in range(1, n):
                g = T(g * gam)
        lg = T(0) if term[s, e] else g
        if variant == "bootstrap_at_n":
            s = (i // N + n) % S
        at.append(s * N + e); Rs.append(R); lgs.append(lg); ms.append(m)
    return np.array(at, np.int64), np.array(Rs, np_dtype), np.array(lgs, np_dtype), np.array(ms, np.int64)


def td_loss(p, target, ring, idx, n_step, head, gamma, weights, dtype, variant=None):
    """p: the online vector as a torch tensor (requires_grad for a gradient); ring = dict(observations [S][N][4], actions, rewards, terminated [S][N]); weights: [batch]
    or None -> (loss, dict of the intermediate torch tensors)"""
    S, N = ring["actions"].shape
    idx = np.asarray(idx, np.int64)
    at, R, lg, m = walk(ring, idx, n_step, head, gamma, np.float64 if dtype == torch.float64 else np.float32, variant)
    flat = lambda k: ring[k].reshape((N * S,) + ring[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    rows = torch.arange(len(idx))
    with torch.no_grad():
        xn = _t(obs[at], dtype)
        qn, _, _ = q_values(p.detach(), xn)
        qt, _, _ = q_values(_t(target, dtype), xn)
        a_star = torch.argmax(qn, dim=1)
        tgt = torch.from_numpy(R) + torch.from_numpy(lg) * qt[rows, a_star]
        assert tgt.dtype == dtype
        w = torch.ones(len(idx), dtype=dtype) if weights is None else _t(np.asarray(weights, f32), dtype)
    q, z1, z2 = q_values(p, _t(obs[idx], dtype))
    old = q[rows, torch.from_numpy(flat("actions")[idx])]
    td = tgt - old
    loss = (w * td ** 2).mean()
    live = torch.from_numpy(1.0 - flat("terminated")[at].astype(np.float64))   # (0 where step m terminated; lg is 0 there, and everywhere when gamma is 0)
    return loss, dict(next_actions=a_star, target=tgt, current=old, td_abs=td.detach().abs(), q_row=q, q_next=qn, q_target=qt, live=live, z1=z1, z2=z2,
                      horizon=torch.from_numpy(m), at=torch.from_numpy(at), R=torch.from_numpy(R), lg=torch.from_numpy(lg))


def evaluate(c, dtype=torch.float64, variant=None, target=None):
    """a case of tests/_nstep_cases.py (or any dict with params, target, the ring, idx, n_step, head, gamma, weights) -> dict(grads, loss, next_actions, horizon, at,
    target, current, td_abs, q_row, q_next, q_target, live, R, lg, z1, z2) as float64 / int64 numpy"""
    p = _t(c["params"], dtype, True)
    loss, aux = td_loss(p, c["target"] if target is None else target, c, c["idx"], c["n_step"], c["head"], c["gamma"], c["weights"], dtype, variant)
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    ints = ("next_actions", "horizon", "at")
    out = {k: d(v) for k, v in aux.items() if k not in ints}
    out.update(grads=d(p.grad), loss=float(loss.item()), **{k: aux[k].numpy().astype(np.int64) for k in ints})
    return out


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def chain(ring, indices, weights, params, target, n_step, heads, dtype=torch.float64, sync_after=25, gamma=0.99):
    """len(indices) weighted updates chained through Adam from zero moments, the target network synced behind update `sync_after`; heads: the head slot of every
    update (or one for all) -> (losses [n], final parameters) float64"""
    p = _t(params, dtype, True)
    tgt = _t(target, dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = []
    for k, idx in enumerate(indices):
        p.grad = None
        loss, _ = td_loss(p, tgt, ring, idx, n_step, int(heads if np.isscalar(heads) else heads[k]), gamma, None if weights is None else weights[k], dtype)
        loss.backward()
        losses.append(float(loss.item()))
        with torch.no_grad():
            adam_step(p, p.grad, m, v, k + 1)
            if k == sync_after:
                tgt = p.detach().clone()
    return np.array(losses, np.float64), p.detach().numpy().astype(np.float64)


CHAIN_STEPS, CHAIN_UPDATES, CHAIN_BATCH, CHAIN_SEED, CHAIN_N = P.CHAIN_STEPS, P.CHAIN_UPDATES, P.CHAIN_BATCH, P.CHAIN_SEED, 3
chain_data = P.chain_data   # §18's CPU-built ring, uniform batches, placed weights, two independent dueling vectors
