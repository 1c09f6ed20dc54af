"""numpy / torch restatement of the noisy-net draw and of the noisy n-step prioritized dueling Double DQN update (include/mi_noisy.h) — TEST INFRASTRUCTURE
(tests/test_noisy_cases_cpu.py validates and measures it, the GPU tests use it).

Two parts.
  THE DRAW.  normal(seed, a, b, stream, dtype) restates z_c, c < 171, on tests/_reinforce_ref.philox: u1 and u2 are the header's float32 numbers in both, the logarithm, the
  square roots, the cosine and the products are numpy's in float32 (every operation rounds once) or in float64.  xi_of(z) = sgn(z) sqrt(|z|); eps_of(xi) lays the
  171 factors over the 255 head elements.  The comparison of the device's draw is xi |xi| against the float64 z, absolute.
  THE UPDATE.  tests/_nstep_ref.py's TD update with one change: both networks are evaluated through the effective vector cat(torso, mu + sigma * eps), eps an
  INPUT (the CPU cases feed the float32 restatement's xi, the GPU tests the DEVICE's own from mi_nz_noise), with AUTOGRAD through mu + sigma * eps producing the
  gradient in mu and in sigma.  ONE online sample serves obs[i] and obs[s_m]; the target's is its own.  _pdd_ref and _nstep_ref are imported, not edited.

`variant=` names a deliberately WRONG reading, used only by the CPU test to show that every noisy case tells it from the right one:
  no_noise                      eps == 0 in both networks
  target_shares_online_sample   the target network is evaluated under the online sample
  fresh_sample_for_argmax       a* comes from the online network under ANOTHER sample (the case's xi_alt) than the one that serves obs[i]
  f_missing                     eps from z, not from xi = f(z)
  bias_uses_input_factor        a bias takes an input factor (bv: xi_0, ba[j]: xi_{85 + j}) instead of its output factor
  streams_share_factors         the advantage stream's weights use the value stream's input factors xi_k instead of xi_{85 + k}
  sigma_grad_unscaled           d loss / d sigma_t = g_t
  sigma_grad_by_xi_not_eps      d loss / d sigma_t = g_t * (the output factor alone)

Figures: _pdd_ref.figures' six ("grad" over the 11,019 means and torso) and "grad_sigma": the distance over the 255 sigma gradients relative to their largest
(0 when both are exactly zero everywhere, inf when only the reference's are).  horizon and next_actions are compared exactly, never through a figure.

Bounds, by the rule of _pdd_ref.py with no new number.  MEASURED[family][figure] is what tests/test_noisy_cases_cpu.py measures for the FLOAT32 evaluation of these
same formulas against the float64 one under the same noise, the maximum over the family's cases (the test ties the constants to the measurement: the constant covers
the measured figure and is at most 1.25 x it).  BOUND[family][figure] = max(8 x MEASURED, BAR), BAR = _dqn_cases.BAR["dqn"] (gradients 1e-5 of max |g|, loss 2e-5;
nothing for q, target, current, td_abs).  CLOSE_Q[family] = 2 x the q bound.  MEASURED_DRAW["z"]: the float32 restatement's xi |xi| against the float64 z over
DRAW_SAMPLES samples, absolute; the device's bound is 8 x it.  MEASURED_CHAIN / BOUND_CHAIN: the same for the 51 chained updates.  No bound comes from the kernel's
output.
"""
import numpy as np
import torch

import _dqn_cases as D
import _nstep_ref as X
import _pdd_ref as P
from _c51_ref import results_dir  # noqa: F401  (the GPU tests write their maxima there)
from _reinforce_ref import philox

f32 = np.float32
NP, NP_MEAN, HEAD, SIGMA, NHEAD, NXI, H2 = 11274, P.NP, 10764, 11019, 255, 171, P.H2
STREAM_ACT, STREAM_LEARN = 13, 14
VARIANTS = ("no_noise", "target_shares_online_sample", "fresh_sample_for_argmax", "f_missing", "bias_uses_input_factor", "streams_share_factors",
            "sigma_grad_unscaled", "sigma_grad_by_xi_not_eps")
FIGURES = P.FIGURES + ("grad_sigma",)
FAMILIES = ("sigma_0", "default", "sigma_x8", "off", "synced", "weights_zero")
SIGMA_0 = 0.5

# measured by tests/test_noisy_cases_cpu.py: torch float32 against torch float64 under the same noise, maximum over the family's cases   (measured: same position)
MEASURED = {
    "sigma_0": dict(q=7.07e-06, target=1.31e-07, current=1.28e-07, td_abs=2.45e-07, loss=6.36e-08, grad=3.69e-07, grad_sigma=1.76e-07),       # 6.54e-06 1.21e-07 1.18e-07 2.26e-07 5.89e-08 3.41e-07 1.62e-07
    "default": dict(q=2.73e-07, target=1.26e-06, current=2.28e-07, td_abs=1.76e-06, loss=2.08e-07, grad=4.21e-07, grad_sigma=3.51e-07),       # 2.52e-07 1.16e-06 2.11e-07 1.63e-06 1.92e-07 3.90e-07 3.24e-07
    "sigma_x8": dict(q=1.28e-06, target=7.33e-07, current=1.28e-06, td_abs=1.1e-06, loss=2.57e-07, grad=2.04e-07, grad_sigma=1.73e-07),       # 1.18e-06 6.79e-07 1.18e-06 1.01e-06 2.38e-07 1.88e-07 1.60e-07
    "off": dict(q=1.89e-07, target=2.36e-07, current=1.34e-07, td_abs=3.47e-07, loss=1.16e-07, grad=2.24e-07, grad_sigma=0.0),                # 1.74e-07 2.18e-07 1.23e-07 3.20e-07 1.07e-07 2.07e-07 0
    "synced": dict(q=2.14e-07, target=2.48e-07, current=1.21e-07, td_abs=1.63e-07, loss=3.83e-08, grad=1.95e-07, grad_sigma=1.62e-07),        # 1.98e-07 2.29e-07 1.11e-07 1.51e-07 3.54e-08 1.80e-07 1.50e-07
    "weights_zero": dict(q=2.23e-07, target=2.18e-07, current=2.23e-07, td_abs=2.93e-07, loss=6.98e-08, grad=1.79e-07, grad_sigma=2.23e-07),  # 2.06e-07 2.01e-07 2.06e-07 2.71e-07 6.46e-08 1.65e-07 2.06e-07
}
MEASURED_DRAW = dict(z=1.65e-06)                                                                                                          # 1.53e-06
MEASURED_CHAIN = dict(loss=1.4e-07, params=2.2e-07)
DRAW_SAMPLES = 4096
BAR = dict(loss=D.BAR["dqn"]["loss"], grad=D.BAR["dqn"]["grad"], grad_sigma=D.BAR["dqn"]["grad"])
BOUND = {fam: {k: max(8.0 * v, BAR.get(k, 0.0)) for k, v in m.items()} for fam, m in MEASURED.items()}
BOUND_DRAW = dict(z=8.0 * MEASURED_DRAW["z"])
BOUND_CHAIN = dict(loss=max(8.0 * MEASURED_CHAIN["loss"], BAR["loss"]), params=8.0 * MEASURED_CHAIN["params"])
CLOSE_Q = {fam: 2.0 * b["q"] for fam, b in BOUND.items()}
LR, ADAM_EPS, BETAS = P.LR, P.ADAM_EPS, P.BETAS
adam_step = P.adam_step
_t = P._t
walk = X.walk


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------------
def normal(seed, a, b, stream, dtype=np.float32):
    """z_c, c < 171, of the sample (seed, a, b, stream); a and b broadcast -> (..., 171) in dtype"""
    a, b = np.broadcast_arrays(np.asarray(a, np.uint64), np.asarray(b, np.uint64))
    c = np.arange(NXI, dtype=np.uint64)
    r = philox(int(seed), a[..., None], b[..., None] * np.uint64(256) + c, int(stream))
    T = dtype
    # u1 and u2 are the header's FLOAT32 numbers in both precisions: (float)(r[0] >> 8) + 0.5f rounds once r[0] >> 8 reaches 2^23, and that rounding is the
    # contract's (where it gives u1 = 1 the draw is exactly 0), not an error of the float32 evaluation
    u1 = (((r[..., 0] >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)).astype(T)
    u2 = ((r[..., 1] >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(T)
    assert u1.dtype == T and u2.dtype == T
    z = np.sqrt(T(-2.0) * np.log(u1)) * np.cos(T(6.28318530717958647692) * u2)
    assert z.dtype == T
    return z


def xi_of(z):
    return (np.sign(z) * np.sqrt(np.abs(z))).astype(z.dtype)


def xi(seed, a, b, stream, dtype=np.float32):
    return xi_of(normal(seed, a, b, stream, dtype))


# the factors of head element t: (output factor, input factor or -1 for a bias)
_CO = np.concatenate([np.full(H2, H2), [H2], np.repeat([2 * H2 + 1, 2 * H2 + 2], H2), [2 * H2 + 1, 2 * H2 + 2]]).astype(np.int64)
_CI = np.concatenate([np.arange(H2), [-1], H2 + 1 + np.tile(np.arange(H2), 2), [-1, -1]]).astype(np.int64)
assert _CO.shape == _CI.shape == (NHEAD,)


def eps_of(x, variant=None):
    """the 255 element noises in head order from the 171 factors x (numpy of either dtype or a torch tensor); products in x's own precision"""
    co, ci = _CO, _CI.copy()
    if variant == "bias_uses_input_factor":
        co = co.copy()
        co[H2] = 0; co[NHEAD - 2] = H2 + 1; co[NHEAD - 1] = H2 + 2
    if variant == "streams_share_factors":
        ci[H2 + 1:NHEAD - 2] = np.tile(np.arange(H2), 2)
    if variant == "f_missing":
        x = x * abs(x)
    w = ci >= 0
    if isinstance(x, torch.Tensor):
        wt = torch.from_numpy(w)
        return torch.where(wt, x[co] * x[np.where(w, ci, 0)], x[co])
    return np.where(w, x[co] * x[np.where(w, ci, 0)], x[co]).astype(x.dtype)


def effective(p, eps):
    """the 11,019-float dueling vector the sample eps makes of the 11,274-float p (torch; eps None: the means)"""
    if eps is None:
        return p[:NP_MEAN]
    return torch.cat([p[:HEAD], p[HEAD:SIGMA] + p[SIGMA:] * eps])


def forward(params, x, xi_sample=None, dtype=torch.float64):
    """-> Q [rows, 2] as float64 numpy under the sample with factors xi_sample (None: the mean network)"""
    with torch.no_grad():
        eps = None if xi_sample is None else eps_of(_t(xi_sample, dtype))
        q, _, _ = P.q_values(effective(_t(params, dtype), eps), _t(np.asarray(x).reshape(-1, 4), dtype))
    return q.numpy().astype(np.float64)


# ---- the update ------------------------------------------------------------------------------------------------------------------------------------
def td_loss(p, target, ring, idx, n_step, head, gamma, weights, dtype, xi_on, xi_tg, noisy=1, variant=None, xi_alt=None):
    """_nstep_ref.td_loss on the effective heads.  p: the 11,274-float online vector as a torch tensor; xi_on / xi_tg: the 171 factors of the online and of the target
    sample (ignored with noisy == 0) -> (loss, dict of the intermediate torch tensors)"""
    assert variant is None or variant in VARIANTS
    S, N = ring["actions"].shape
    idx = np.asarray(idx, np.int64)
    at, R, lg, m = walk(ring, idx, n_step, head, gamma, np.float64 if dtype == torch.float64 else np.float32)
    flat = lambda k: ring[k].reshape((N * S,) + ring[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    rows = torch.arange(len(idx))
    on = noisy and variant != "no_noise"
    ev = variant if variant in ("f_missing", "bias_uses_input_factor", "streams_share_factors") else None
    e_on = eps_of(_t(xi_on, dtype), ev) if on else None
    e_tg = eps_of(_t(xi_on if variant == "target_shares_online_sample" else xi_tg, dtype), ev) if on else None
    e_arg = eps_of(_t(xi_alt, dtype), ev) if on and variant == "fresh_sample_for_argmax" else e_on
    with torch.no_grad():
        xn = _t(obs[at], dtype)
        qn, _, _ = P.q_values(effective(p.detach(), e_arg), xn)
        qt, _, _ = P.q_values(effective(_t(target, dtype), e_tg), xn)
        a_star = torch.argmax(qn, dim=1)
        tgt = torch.from_numpy(R) + torch.from_numpy(lg) * qt[rows, a_star]
        assert tgt.dtype == dtype
        w = torch.ones(len(idx), dtype=dtype) if weights is None else _t(np.asarray(weights, f32), dtype)
    q, z1, z2 = P.q_values(effective(p, e_on), _t(obs[idx], dtype))   # (eps None: sigma is not in the graph and its gradient is exact zeros)
    old = q[rows, torch.from_numpy(flat("actions")[idx])]
    td = tgt - old
    loss = (w * td ** 2).mean()
    live = torch.from_numpy(1.0 - flat("terminated")[at].astype(np.float64))
    return loss, dict(next_actions=a_star, target=tgt, current=old, td_abs=td.detach().abs(), q_row=q, q_next=qn, q_target=qt, live=live, z1=z1, z2=z2,
                      horizon=torch.from_numpy(m), at=torch.from_numpy(at), R=torch.from_numpy(R), lg=torch.from_numpy(lg))


def evaluate(c, dtype=torch.float64, variant=None, xi_on=None, xi_tg=None):
    """a case of tests/_noisy_cases.py -> dict(grads [11,274], loss, next_actions, horizon, at, target, current, td_abs, q_row, q_next, q_target, live, R, lg, z1,
    z2) as float64 / int64 numpy; xi_on / xi_tg replace the case's own factors (the GPU tests: the device's)"""
    p = _t(c["params"], dtype, True)
    xo, xt = c["xi_on"] if xi_on is None else xi_on, c["xi_tg"] if xi_tg is None else xi_tg
    loss, aux = td_loss(p, c["target"], c, c["idx"], c["n_step"], c["head"], c["gamma"], c["weights"], dtype, xo, xt, c["noisy"], variant, c.get("xi_alt"))
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    ints = ("next_actions", "horizon", "at")
    out = {k: d(v) for k, v in aux.items() if k not in ints}
    g = d(p.grad)
    if variant == "sigma_grad_unscaled":
        g[SIGMA:] = g[HEAD:SIGMA]
    elif variant == "sigma_grad_by_xi_not_eps":
        g[SIGMA:] = g[HEAD:SIGMA] * np.asarray(xo, np.float64)[_CO]
    out.update(grads=g, loss=float(loss.item()), **{k: aux[k].numpy().astype(np.int64) for k in ints})
    return out


def figures(exp, got, ring_family):
    """_pdd_ref.figures with the gradient split: "grad" over the first 11,019 elements, "grad_sigma" over the 255 sigmas"""
    mean = lambda r: dict(r, grads=np.asarray(r["grads"])[:NP_MEAN])   # noqa: E731
    f = P.figures(mean(exp), mean(got), ring_family)
    es, gs = np.asarray(exp["grads"], np.float64)[SIGMA:], np.asarray(got["grads"], np.float64)[SIGMA:]
    top = float(np.abs(es).max())
    if top > 0:
        f["grad_sigma"] = P._dist(gs, es) / top
    else:
        f["grad_sigma"] = 0.0 if not gs.any() else np.inf
    return f


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def chain(ring, indices, weights, params, target, n_step, heads, xi_pairs, dtype=torch.float64, sync_after=25, gamma=0.99):
    """_nstep_ref.chain on 11,274-float vectors; xi_pairs[k] = (xi_on, xi_tg) of update k -> (losses [n], final parameters) float64"""
    p = _t(params, dtype, True)
    tgt = _t(target, dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = []
    for k, idx in enumerate(indices):
        p.grad = None
        loss, _ = td_loss(p, tgt, ring, idx, n_step, int(heads if np.isscalar(heads) else heads[k]), gamma, None if weights is None else weights[k], dtype,
                          xi_pairs[k][0], xi_pairs[k][1])
        loss.backward()
        losses.append(float(loss.item()))
        with torch.no_grad():
            adam_step(p, p.grad, m, v, k + 1)
            if k == sync_after:
                tgt = p.detach().clone()
    return np.array(losses, np.float64), p.detach().numpy().astype(np.float64)


CHAIN_STEPS, CHAIN_UPDATES, CHAIN_BATCH, CHAIN_SEED, CHAIN_N = X.CHAIN_STEPS, X.CHAIN_UPDATES, X.CHAIN_BATCH, X.CHAIN_SEED, X.CHAIN_N


def default_sigma(scale=1.0):
    return np.full(NHEAD, f32(SIGMA_0 / np.sqrt(H2)) * f32(scale), f32)


def chain_data(R):
    """_nstep_ref.chain_data's ring, batches, weights and dueling vectors, each vector extended by the default sigma, and the learning samples of updates 0 .. 50
    from the float32 restatement -> (ring, indices, weights, params [11,274], target [11,274], xi_pairs)"""
    ring, indices, weights, params, target = X.chain_data(R)
    ext = lambda v: np.concatenate([v.astype(f32), default_sigma()])   # noqa: E731
    u = np.arange(len(indices), dtype=np.uint64)
    on, tg = xi(CHAIN_SEED, u, 0, STREAM_LEARN), xi(CHAIN_SEED, u, 1, STREAM_LEARN)
    return ring, indices, weights, ext(params), ext(target), list(zip(on, tg))
