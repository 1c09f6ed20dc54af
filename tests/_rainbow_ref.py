"""numpy / torch restatement of Rainbow's draw and update (include/mi_rainbow.h) — TEST INFRASTRUCTURE (tests/test_rainbow_cases_cpu.py validates and measures
it, the GPU tests use it).

Two parts.
  THE DRAW.  normal(seed, a, b, stream, dtype) restates z_c, c < 321, on tests/_reinforce_ref.philox with the counter b * 512 + c and tests/_noisy_ref.py's
  expression (xi_of is that module's).  factors(xi) lays the 321 numbers over the 153 head rows: fin [153, 84], fout [153]; eps_of(fin, fout) is the element noise
  in head order [13,005], products in the inputs' own precision (float32: the device's bits).
  THE UPDATE.  The whole update in torch with the element noise as an INPUT (the CPU cases feed the float32 restatement's, the GPU tests the DEVICE's own from
  mi_rb_noise): the n-step walk of tests/_nstep_ref.py, a* from the online network at obs[s_m] under the online sample, the target network's distribution of a*
  under the target sample, the categorical projection on the run-time support, the importance-weighted cross-entropy with the 1e-8 inside the log, AUTOGRAD through
  mu + sigma * eps for the gradient in mu and in sigma, prio = max(rowloss, 0).  float64, or float32 for the measurement.

`variant=` names a deliberately WRONG reading, used only by the CPU test:
  no_noise                      eps == 0 in both networks
  target_shares_online_sample   the target network is evaluated under the online sample
  argmax_by_target_net          a* is the TARGET network's argmax
  one_step_projection           gamma where gamma^m belongs
  projection_unclamped          tz is not clamped: mass beyond the support is lost
  l_equals_u_mass_dropped       wl = (u - b) p without the l == u term
  dueling_mean_missing          logits = v + A
  weights_ignored               w == 1
  priority_weighted             prio = w * rowloss
  sigma_grad_unscaled           d loss / d sigma_t = g_t
  eps_inside_softmax_not_log    rowloss = -sum m log_softmax(l): no 1e-8 inside the log

Figures.  probs, target_probs: largest absolute distance.  q: the same over q at obs[i], and the online and target q at obs[s_m].  prio: largest absolute
distance of the row losses over max(1, the largest).  loss: relative.  grad: the distance over the 23,769 torso and mu elements relative to their largest; grad_sigma:
the same over the 13,005 sigmas (0 when both are exactly zero, inf when only the reference's are).  horizon and next_actions are compared exactly.

Bounds, by the rule of tests/_pdd_ref.py with no new number.  MEASURED[family][figure] is what tests/test_rainbow_cases_cpu.py measures for the FLOAT32 evaluation
of these same formulas against the float64 one under the same noise, the maximum over the family's cases (the constant covers the measurement and is at most
1.25 x it).  BOUND = max(8 x MEASURED, BAR), BAR = _dqn_cases.BAR["dqn"] (gradients 1e-5, loss 2e-5; nothing for the others).  CLOSE_Q[family] = 2 x the q bound.
"""
import numpy as np
import torch

import _dqn_cases as D
import _noisy_ref as Z
import _nstep_ref as X
import _pdd_ref as P
from _c51_ref import results_dir  # noqa: F401  (the GPU tests write their maxima there)
from _reinforce_ref import philox

f32 = np.float32
NA, H2, NROWS, NXI = 51, 84, 153, 321
TORSO, HEAD, BV, WA, BA, SIGMA, NHEAD, NP = 10764, 10764, 15048, 15099, 23667, 23769, 13005, 36774
NP_MEAN = SIGMA
STREAM_ACT, STREAM_LEARN = 13, 14
VARIANTS = ("no_noise", "target_shares_online_sample", "argmax_by_target_net", "one_step_projection", "projection_unclamped", "l_equals_u_mass_dropped",
            "dueling_mean_missing", "weights_ignored", "priority_weighted", "sigma_grad_unscaled", "eps_inside_softmax_not_log")
FIGURES = ("probs", "q", "target_probs", "prio", "loss", "grad", "grad_sigma")
FAMILIES = ("sigma_0", "default", "sigma_x8", "off", "synced", "weights_zero")
SIGMA_0 = 0.5

# measured by tests/test_rainbow_cases_cpu.py: torch float32 against torch float64 under the same noise, maximum over the family's cases
MEASURED = {
    "sigma_0": dict(probs=1.03e-06, q=0.000241, target_probs=2.81e-06, prio=9.19e-07, loss=1.57e-07, grad=1.69e-06, grad_sigma=1.24e-06),       # 9.55e-07 0.000223 2.6e-06 8.51e-07 1.45e-07 1.57e-06 1.15e-06
    "default": dict(probs=2.07e-08, q=5.92e-07, target_probs=7.44e-06, prio=1.88e-06, loss=1.31e-07, grad=2.17e-06, grad_sigma=2.13e-06),       # 1.91e-08 5.48e-07 6.88e-06 1.74e-06 1.21e-07 2.01e-06 1.97e-06
    "sigma_x8": dict(probs=1.59e-07, q=1.65e-06, target_probs=1.65e-06, prio=6.87e-07, loss=4.54e-08, grad=1.39e-06, grad_sigma=1.29e-06),      # 1.48e-07 1.53e-06 1.53e-06 6.36e-07 4.2e-08 1.29e-06 1.19e-06
    "off": dict(probs=9.18e-09, q=4.63e-07, target_probs=2.12e-06, prio=3.14e-07, loss=4.58e-08, grad=1.18e-06, grad_sigma=0.0),                # 8.5e-09 4.28e-07 1.96e-06 2.91e-07 4.24e-08 1.1e-06 0
    "synced": dict(probs=9.11e-09, q=3.32e-07, target_probs=1.12e-06, prio=1.8e-07, loss=1.12e-07, grad=9.69e-07, grad_sigma=8.44e-07),         # 8.43e-09 3.08e-07 1.04e-06 1.66e-07 1.04e-07 8.98e-07 7.82e-07
    "weights_zero": dict(probs=1.26e-08, q=3.5e-07, target_probs=3e-07, prio=1.62e-07, loss=1.11e-07, grad=4.37e-07, grad_sigma=3.01e-07),      # 1.16e-08 3.24e-07 2.78e-07 1.5e-07 1.03e-07 4.05e-07 2.79e-07
}
MEASURED_DRAW = dict(z=1.89e-06)                                                                                                          # 1.75e-06
MEASURED_CHAIN = dict(loss=9.1e-08, params=3.45e-07)                                                                                     # 8.43e-08 3.19e-07
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
xi_of = Z.xi_of


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------------
def normal(seed, a, b, stream, dtype=np.float32):
    """z_c, c < 321, of the sample (seed, a, b, stream); a and b broadcast -> (..., 321) in dtype.  _noisy_ref.normal with the counter b * 512 + c."""
    a, b = np.broadcast_arrays(np.asarray(a, np.uint64), np.asarray(b, np.uint64))
    c = np.arange(NXI, dtype=np.uint64)
    r = philox(int(seed), a[..., None], b[..., None] * np.uint64(512) + c, int(stream))
    T = dtype
    u1 = (((r[..., 0] >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)).astype(T)   # the header's FLOAT32 numbers in both precisions
    u2 = ((r[..., 1] >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(T)
    z = np.sqrt(T(-2.0) * np.log(u1)) * np.cos(T(6.28318530717958647692) * u2)
    assert z.dtype == T
    return z


def xi(seed, a, b, stream, dtype=np.float32):
    return xi_of(normal(seed, a, b, stream, dtype))


# head row r: its output factor's index, and where its 84 input factors start
_FO = np.concatenate([84 + np.arange(NA), 219 + np.arange(2 * NA)]).astype(np.int64)
_FI = np.concatenate([np.zeros(NA), np.full(2 * NA, 135)]).astype(np.int64)


def factors(x):
    """the 321 numbers of one sample -> (fin [153, 84], fout [153]) as head row r uses them"""
    x = np.asarray(x)
    return x[_FI[:, None] + np.arange(H2)[None, :]], x[_FO]


def eps_of(fin, fout):
    """the element noise in head order [13,005]: Wv, bv, Wa, ba; a weight's is fout * fin (one product in the inputs' precision), a bias's is fout"""
    w = fout[:, None] * fin
    return np.concatenate([w[:NA].reshape(-1), fout[:NA], w[NA:].reshape(-1), fout[NA:]]).astype(fin.dtype)


def eps(seed, a, b, stream, dtype=np.float32):
    return eps_of(*factors(xi(seed, a, b, stream, dtype)))


# ---- the network -----------------------------------------------------------------------------------------------------------------------------------
def effective(p, e):
    """the 23,769-float vector (torso, effective head) the element noise e makes of the 36,774-float p (torch; e None: the means)"""
    if e is None:
        return p[:SIGMA]
    return torch.cat([p[:HEAD], p[HEAD:SIGMA] + p[SIGMA:] * e])


def atoms(support, dtype):
    lo, hi = _t(f32(support[0]), dtype), _t(f32(support[1]), dtype)
    dz = (hi - lo) / 50
    return lo, hi, dz, lo + dz * torch.arange(NA, dtype=dtype)


def dist(pe, x, support, variant=None):
    """-> (probs [rows, 2, 51], q [rows, 2]) of the effective vector pe"""
    h2, _, _ = D.features(pe, x)
    v = h2 @ pe[HEAD:BV].reshape(NA, H2).T + pe[BV:WA]
    adv = (h2 @ pe[WA:BA].reshape(2 * NA, H2).T + pe[BA:SIGMA]).reshape(-1, 2, NA)
    if variant == "dueling_mean_missing":
        logit = v[:, None, :] + adv
    else:
        logit = v[:, None, :] + (adv - 0.5 * (adv[:, 0] + adv[:, 1])[:, None, :])
    p = torch.softmax(logit, dim=-1)
    z = atoms(support, pe.dtype)[3]
    return p, (p * z).sum(-1), logit


def forward(params, x, support, e=None, dtype=torch.float64):
    """-> (probs [rows, 2, 51], q [rows, 2]) as float64 numpy under the element noise e (None: the mean network)"""
    with torch.no_grad():
        p, q, _ = dist(effective(_t(params, dtype), None if e is None else _t(e, dtype)), _t(np.asarray(x).reshape(-1, 4), dtype), support)
    return p.numpy().astype(np.float64), q.numpy().astype(np.float64)


def project(pn, R, lg, support, dtype, variant=None):
    """the categorical projection of the distributions pn [rows, 51] -> (m [rows, 51], dict of counts of the placed edges)"""
    lo, hi, dz, z = atoms(support, dtype)
    tz = R[:, None] + lg[:, None] * z[None, :]
    if variant != "projection_unclamped":
        tz = torch.minimum(torch.maximum(tz, lo), hi)
    b = (tz - lo) / dz
    l, u = torch.floor(b), torch.ceil(b)
    same = (l == u).to(dtype)
    wl = ((u + (0 if variant == "l_equals_u_mass_dropped" else same)) - b) * pn
    wu = (b - l) * pn
    rows = len(R)
    m = torch.zeros(rows * NA, dtype=dtype)
    off = (torch.arange(rows) * NA)[:, None]
    for idx, wgt in ((l, wl), (u, wu)):   # index_add_ on the CPU adds in order: the lower contributions in ascending (row, j), then the upper ones
        k = idx.to(torch.int64)
        ok = (k >= 0) & (k < NA)
        m.index_add_(0, (k + off)[ok], wgt[ok])
    edges = dict(at_lo=(tz == lo), at_hi=(tz == hi), same=(l == u))
    return m.reshape(rows, NA), edges


def loss_of(p, target, ring, idx, n_step, head, gamma, weights, dtype, support, e_on, e_tg, noisy=1, variant=None):
    """p: the 36,774-float online vector as a torch tensor; e_on / e_tg: the element noise [13,005] of the online and of the target sample (ignored with
    noisy == 0) -> (loss, dict of the intermediate torch tensors)"""
    assert variant is None or variant in VARIANTS
    S, N = ring["actions"].shape
    idx = np.asarray(idx, np.int64)
    at, R, lg, m_steps = walk(ring, idx, n_step, head, gamma, np.float64 if dtype == torch.float64 else np.float32)
    if variant == "one_step_projection":
        lg = np.where(lg != 0, lg.dtype.type(f32(gamma)), lg)
    flat = lambda k: ring[k].reshape((N * S,) + ring[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    rows = torch.arange(len(idx))
    on = noisy and variant != "no_noise"
    eo = _t(e_on, dtype) if on else None
    et = _t(e_on if variant == "target_shares_online_sample" else e_tg, dtype) if on else None
    with torch.no_grad():
        xn = _t(obs[at], dtype)
        _, qn, _ = dist(effective(p.detach(), eo), xn, support, variant)
        pt, qt, _ = dist(effective(_t(target, dtype), et), xn, support, variant)
        a_star = torch.argmax(qt if variant == "argmax_by_target_net" else qn, dim=1)
        tp, edges = project(pt[rows, a_star], torch.from_numpy(R), torch.from_numpy(lg), support, dtype, variant)
        assert tp.dtype == dtype
        w = torch.ones(len(idx), dtype=dtype) if weights is None or variant == "weights_ignored" else _t(np.asarray(weights, f32), dtype)
    pr, q, logit = dist(effective(p, eo), _t(obs[idx], dtype), support, variant)
    act = torch.from_numpy((flat("actions")[idx] != 0).astype(np.int64))
    pa = pr[rows, act]
    if variant == "eps_inside_softmax_not_log":
        rowloss = -(tp * torch.log_softmax(logit[rows, act], dim=-1)).sum(-1)
    else:
        rowloss = -(tp * torch.log(pa + 1e-8)).sum(-1)
    loss = (w * rowloss).mean()
    prio = torch.clamp(rowloss.detach() * (w if variant == "priority_weighted" else 1.0), min=0.0)
    live = torch.from_numpy(1.0 - flat("terminated")[at].astype(np.float64))
    return loss, dict(next_actions=a_star, target_probs=tp, probs=pa.detach(), prio=prio, q_row=q.detach(), q_next=qn, q_target=qt, live=live,
                      horizon=torch.from_numpy(m_steps), at=torch.from_numpy(at), R=torch.from_numpy(R), lg=torch.from_numpy(lg),
                      **{k: v.to(torch.float64) for k, v in edges.items()})


def evaluate(c, dtype=torch.float64, variant=None, e_on=None, e_tg=None):
    """a case of tests/_rainbow_cases.py -> dict(grads [36,774], loss, next_actions, horizon, at, target_probs, probs, prio, q_row, q_next, q_target, live, R, lg,
    at_lo, at_hi, same) as float64 / int64 numpy; e_on / e_tg replace the case's own element noise (the GPU tests: the device's)"""
    p = _t(c["params"], dtype, True)
    eo, et = c["e_on"] if e_on is None else e_on, c["e_tg"] if e_tg is None else e_tg
    loss, aux = loss_of(p, c["target"], c, c["idx"], c["n_step"], c["head"], c["gamma"], c["weights"], dtype, c["support"], eo, et, c["noisy"], variant)
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    ints = ("next_actions", "horizon", "at")
    out = {k: d(v) for k, v in aux.items() if k not in ints}
    g = d(p.grad)
    if variant == "sigma_grad_unscaled":
        g[SIGMA:] = g[HEAD:SIGMA]
    out.update(grads=g, loss=float(loss.item()), **{k: aux[k].numpy().astype(np.int64) for k in ints})
    return out


def _dist(g, r):
    g, r = np.asarray(g, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    assert np.isfinite(r).all(), "the float64 reference itself is not finite"
    return float(np.abs(g - r).max()) if np.isfinite(g).all() else np.inf


def figures(exp, got):
    """exp: evaluate()'s float64 result; got: another evaluation or the device's outputs under the same names"""
    f = dict(probs=_dist(got["probs"], exp["probs"]), target_probs=_dist(got["target_probs"], exp["target_probs"]),
             q=max(_dist(got[k], exp[k]) for k in ("q_row", "q_next", "q_target") if k in got),
             prio=_dist(got["prio"], exp["prio"]) / max(1.0, float(np.abs(exp["prio"]).max())),
             loss=_dist([got["loss"]], [exp["loss"]]) / abs(exp["loss"]))
    eg, gg = np.asarray(exp["grads"], np.float64), np.asarray(got["grads"], np.float64)
    f["grad"] = _dist(gg[:SIGMA], eg[:SIGMA]) / float(np.abs(eg[:SIGMA]).max())
    top = float(np.abs(eg[SIGMA:]).max())
    if top > 0:
        f["grad_sigma"] = _dist(gg[SIGMA:], eg[SIGMA:]) / top
    else:
        f["grad_sigma"] = 0.0 if not gg[SIGMA:].any() else np.inf
    return f


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def chain(ring, indices, weights, params, target, n_step, heads, support, e_pairs, dtype=torch.float64, sync_after=25, gamma=0.99):
    """_noisy_ref.chain for this update; e_pairs[k] = (e_on, e_tg) of update k -> (losses [n], final parameters) float64"""
    p = _t(params, dtype, True)
    tgt = _t(target, dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = []
    for k, idx in enumerate(indices):
        p.grad = None
        loss, _ = loss_of(p, tgt, ring, idx, n_step, int(heads if np.isscalar(heads) else heads[k]), gamma, None if weights is None else weights[k], dtype, support,
                          e_pairs[k][0], e_pairs[k][1])
        loss.backward()
        losses.append(float(loss.item()))
        with torch.no_grad():
            adam_step(p, p.grad, m, v, k + 1)
            if k == sync_after:
                tgt = p.detach().clone()
    return np.array(losses, np.float64), p.detach().numpy().astype(np.float64)


CHAIN_STEPS, CHAIN_UPDATES, CHAIN_BATCH, CHAIN_SEED, CHAIN_N = X.CHAIN_STEPS, X.CHAIN_UPDATES, X.CHAIN_BATCH, X.CHAIN_SEED, X.CHAIN_N
CHAIN_SUPPORT = (0.0, 100.0)


def default_sigma(scale=1.0):
    return np.full(NHEAD, f32(SIGMA_0 / np.sqrt(H2)) * f32(scale), f32)


def head_means(rng, scale=1.0):
    """13,005 means as NoisyLinear draws them: U(+-1 / sqrt(84)), times scale"""
    return (rng.uniform(-1.0, 1.0, NHEAD) / np.sqrt(H2) * scale).astype(f32)


def vector(torso, rng, sigma_scale=1.0, head_scale=1.0, jitter=False):
    """a 36,774-float network: the given torso, drawn head means, sigma_0 / sqrt(84) x sigma_scale (x U(0.5, 1.5) per element with jitter)"""
    sg = default_sigma(sigma_scale)
    if jitter:
        sg = (sg * rng.uniform(0.5, 1.5, NHEAD).astype(f32)).astype(f32)
    return np.concatenate([np.asarray(torso, f32)[:TORSO], head_means(rng, head_scale), sg]).astype(f32)


def chain_data(R):
    """_nstep_ref.chain_data's ring, batches and weights, the torsos of its two dueling vectors under drawn Rainbow heads with the default sigma, and the element
    noise of updates 0 .. 50 from the float32 restatement -> (ring, indices, weights, params [36,774], target [36,774], e_pairs)"""
    ring, indices, weights, params, target = X.chain_data(R)
    rng = np.random.default_rng([2018, 22])
    u = np.arange(len(indices), dtype=np.uint64)
    on, tg = xi(CHAIN_SEED, u, 0, STREAM_LEARN), xi(CHAIN_SEED, u, 1, STREAM_LEARN)
    pairs = [(eps_of(*factors(a)), eps_of(*factors(b))) for a, b in zip(on, tg)]
    return ring, indices, weights, vector(params, rng), vector(target, rng), pairs
