"""Synthetic SAC cases and their float64 expectations — TEST INFRASTRUCTURE (tests/test_sac_cases_cpu.py validates it, tests/test_gpu_sac_cases.py uses it).

The reference.  Actor.get_action, the critic loss, the actor loss and the alpha loss of sac.py restated with torch in float64 on the CPU (the formulas of
include/mi_rl.h "SAC": ReLU MLPs, L = -5 + 3.5 (tanh(sraw) + 1), z = mean + e^L eps, u = tanh z, action 2 u, logp = N(z; mean, sd) - log(2 (1 - u^2) + 1e-6),
target r + (1 - term) f32(0.99) (min Qt - alpha logp), torch.minimum on the online critics); AUTOGRAD produces every gradient — there is no hand-written backward
in this file, which is what makes it independent of oracle/cpu_ref.c and of the kernels (both derive the same backward by hand).  The same functions run in
torch float32 (`dtype=`) to tell which of oracle and device departs when the two disagree (tests/test_sac_cases_cpu.py: torch's own f32 autograd is itself the
outlier on two cases, through its tanh backward; the variant "slope_from_forward_product" of actor_forward exists to show that, and is used for nothing else).

The cases.  Batch in {1, 5, 16, 17, 40} (row groups hold 16 rows: one row, a partial group, a full one, a second group with one valid row, three groups),
rings (n_envs, slots) in {(1, 2), (3, 7), (2, 30)}, alpha in {0.37, 1e-3, 5}.  Every case with >= 5 rows holds one terminated row and >= 2 rows whose successor
wraps past the ring's end; the (1, 2) ring is used with its wrapping row only.  Each case carries three noise vectors — for the critic update (drawn at the
SUCCESSOR observation), the actor update and the alpha step — so every case runs through all three consumers.
  bands   the pre-tanh value z is PLACED: eps_b = (z_target - mean_b) / sd_b from the float64 forward, the log-std head biased to sraw ~ 1.2 (sd ~ 4, 1 - ls^2 ~ 0.3).
          A: |z| in {0 .. 5}; B: {6 .. 12} (f32 cannot resolve 1 - u^2 against the 1e-6: loose bounds of its own); C: {16, 18, 20} (u == +-1 in f32); AC: A and C mixed.
  clamp   log-std head biased to sraw ~ +-6 (ls within 1.3e-5 of +-1) and +-20 (ls == +-1 in f32 and in float64: d/d sraw == 0, sd == e^2 / e^-5); N(0, 1) noise,
          a draw repeated while its z falls into (5, 16) — with sd = e^2 an untouched N(0, 1) vector puts a third of the rows into band B.
  tie     hand-built critics that tie bit for bit with different action derivatives (make_tie_case).

Conditions (asserted by the CPU test; the seeds in SEEDS were searched with find_seed so that the float64 reference alone meets them): no row is excluded from any
comparison; in the tight families no ReLU pre-activation of any net in any row lies within NEAR_ZERO of 0 (a mask flip is a legitimate f32 outcome that would
otherwise need an exclusion); outside the tie case no |q1 - q2|, online or target, is within Q_MARGIN (a flipped min selector likewise); |eps| <= 6; |loss| >= 0.1 (losses are compared relatively).

Bounds.  tests/test_sac_cases_cpu.py measures oracle/cpu_ref.c (f32) against this reference per family and figure; MEASURED holds what it measured, BOUND = 8 x
(the convention of tests/_c51_ref.py).  Figures: "action" / "logp" per row, absolute; "loss" relative; "mlp" the mean log-prob, absolute; "grad" max |g - ref| over
max |ref| per network; "tensor" the same per parameter tensor against that tensor's own max |ref|, floored at TENSOR_FLOOR x the network's (a tensor whose whole
gradient lies below 1e-6 of the network's is compared in that scale: band C's mean head is exactly 0 in f32 and 1e-17 in float64).
"""
import functools
import math

import numpy as np
import torch

f32 = np.float32
SQ_NP, AC_NP, H = 67329, 67330, 256
SQ = dict(W1=(0, 1024), b1=(1024, 1280), W2=(1280, 66816), b2=(66816, 67072), W3=(67072, 67328), b3=(67328, 67329))
AC = dict(W1=(0, 768), b1=(768, 1024), W2=(1024, 66560), b2=(66560, 66816), WM=(66816, 67072), BM=(67072, 67073), WL=(67073, 67329), BL=(67329, 67330))
GAMMA32 = f32(0.99)
TARGET_ENTROPY = -1.0
NEAR_ZERO = 1e-5
TENSOR_FLOOR = 1e-6
MAX_EPS = 6.0
BAND_A = (0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0)
BAND_B = (6.0, 7.0, 7.6, 8.0, 9.0, 10.0, 12.0)
BAND_C = (16.0, 18.0, 20.0)
ILL = (5.0, 16.0)              # |z| in this open interval: f32 cannot resolve 2 (1 - u^2) against the 1e-6 (band B); clamp cases redraw such rows

# (name, family, batch, (n_envs, slots), alpha)
SPECS = (
    ("A_40", "A", 40, (2, 30), 0.37),
    ("A_1", "A", 1, (1, 2), 5.0),
    ("B_17", "B", 17, (3, 7), 0.37),
    ("B_5", "B", 5, (2, 30), 1e-3),
    ("C_16", "C", 16, (3, 7), 1e-3),
    ("C_1", "C", 1, (1, 2), 0.37),
    ("AC_17", "AC", 17, (2, 30), 5.0),
    ("AC_5", "AC", 5, (3, 7), 0.37),
    ("clamp_p6_17", "clamp6", 17, (3, 7), 0.37),
    ("clamp_m6_16", "clamp6", 16, (2, 30), 5.0),
    ("clamp_p20_5", "clamp20", 5, (3, 7), 0.37),
    ("clamp_m20_40", "clamp20", 40, (2, 30), 0.37),
    ("clamp_p20_1", "clamp20", 1, (1, 2), 1e-3),
)
SRAW = {"clamp_p6_17": 6.0, "clamp_m6_16": -6.0, "clamp_p20_5": 20.0, "clamp_m20_40": -20.0, "clamp_p20_1": 20.0}
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (6, 0, 0, 0, 1, 0, 1, 0, 2, 3, 5, 3, 4)
TIE_BATCHES = (5, 17)
TIGHT = ("A", "C", "AC", "clamp6", "clamp20", "tie")
FIGURES = ("action", "logp", "loss", "mlp", "grad", "tensor")

# measured by tests/test_sac_cases_cpu.py: the f32 oracle (oracle/cpu_ref.c) against this file's float64, maximum over the family's cases -> device bound = 8 x.
# AC is not measured on its own: its bound is the larger of A's and C's.
MEASURED_Q_ABS = 2.4e-7        # a critic's value, absolute, over every case (2.38e-7)
MEASURED = {                   # (measured: the figure in the same position of the comment)
    "A": dict(action=4.7e-7, logp=1.6e-4, loss=4.4e-5, mlp=3.0e-5, grad=2.2e-6, tensor=5.7e-6),             # 4.65e-7 1.51e-4 4.35e-5 2.98e-5 2.14e-6 5.62e-6
    "B": dict(action=5.9e-8, logp=9.9e-2, loss=5.1e-3, mlp=3.9e-2, grad=4.8e-2, tensor=6.7e-2),             # 5.83e-8 9.89e-2 5.04e-3 3.85e-2 4.79e-2 6.61e-2
    # C: f32 gives action == +-2 and a mean head with NO gradient (1 - u^2 == 0) where float64 has 2 - 5e-14 and 2e-8 of the network's: "action" and "tensor" measure that
    "C": dict(action=5.1e-14, logp=2.5e-6, loss=4.1e-7, mlp=8.3e-7, grad=1.4e-6, tensor=1.9e-2),            # 5.06e-14 2.44e-6 4.05e-7 8.22e-7 1.35e-6 1.86e-2
    # clamp6: "tensor" is the log-std head, whose whole gradient carries the factor 1 - ls^2 = 2.5e-5 that f32 forms from an ls 200 ulp below 1
    "clamp6": dict(action=3.6e-7, logp=5.7e-5, loss=2.1e-6, mlp=1.4e-6, grad=9.1e-7, tensor=4.6e-4),        # 3.53e-7 5.64e-5 2.08e-6 1.33e-6 9.08e-7 4.60e-4
    "clamp20": dict(action=3.6e-7, logp=3.8e-5, loss=5.0e-6, mlp=7.7e-6, grad=7.9e-7, tensor=7.9e-7),       # 3.57e-7 3.71e-5 4.97e-6 7.68e-6 7.88e-7 7.88e-7
    "tie": dict(action=2.3e-8, logp=1.4e-7, loss=4.9e-7, mlp=1.4e-7, grad=9.1e-8, tensor=1.4e-7),           # 2.24e-8 1.38e-7 4.83e-7 1.38e-7 9.06e-8 1.34e-7
}
MEASURED["AC"] = {k: max(MEASURED["A"][k], MEASURED["C"][k]) for k in FIGURES}
BOUND = {fam: {k: 8.0 * v for k, v in m.items()} for fam, m in MEASURED.items()}
Q_MARGIN = 8.0 * MEASURED_Q_ABS


# ---- the reference: sac.py's formulas in torch, any dtype, gradients by autograd ---------------------------------------------------
def _t(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def _sl(p, lay, name, shape=None):
    a, b = lay[name]
    v = p[a:b]
    return v if shape is None else v.reshape(shape)


def q_forward(p, obs, act):
    """SoftQNetwork.forward: -> (q [B], [z1, z2] pre-activations)"""
    x = torch.cat([obs, act.reshape(-1, 1)], 1)
    z1 = x @ _sl(p, SQ, "W1", (H, 4)).T + _sl(p, SQ, "b1")
    z2 = torch.relu(z1) @ _sl(p, SQ, "W2", (H, H)).T + _sl(p, SQ, "b2")
    return torch.relu(z2) @ _sl(p, SQ, "W3") + _sl(p, SQ, "b3"), [z1, z2]


def actor_forward(p, obs, eps, variant=None):
    """Actor.get_action with the draws of rsample() supplied -> dict(action, logp, mean, sd, ls, sraw, z, u, pre)"""
    z1 = obs @ _sl(p, AC, "W1", (H, 3)).T + _sl(p, AC, "b1")
    z2 = torch.relu(z1) @ _sl(p, AC, "W2", (H, H)).T + _sl(p, AC, "b2")
    h2 = torch.relu(z2)
    mean = h2 @ _sl(p, AC, "WM") + _sl(p, AC, "BM")
    sraw = h2 @ _sl(p, AC, "WL") + _sl(p, AC, "BL")
    ls = torch.tanh(sraw)
    if variant == "clamp_derivative_dropped":       # d ls / d sraw taken as 1
        ls = ls.detach() + sraw - sraw.detach()
    L = -5.0 + 0.5 * (2.0 - -5.0) * (ls + 1.0)
    sd = torch.exp(L)
    z = mean + sd * eps                              # Normal(mean, sd).rsample()
    u = torch.tanh(z)
    if variant == "slope_from_forward_product":      # FLOAT32 DIAGNOSTIC ONLY (never the reference): tanh's slope taken as the forward's own rounded 1 - u u, as the oracle
        w = u.detach()                               # and the kernels do; torch's f32 tanh backward forms 1 - u^2 with one rounding, which then differs from the 1 - u u
        u = w + (1.0 - w * w) * (z - z.detach())     # inside the log by up to 3e-8 — against 1 - u^2 = 1.8e-4 at |z| = 5 that is 1.7e-4 of the row's gradient
    log_scale = torch.log(sd)
    if variant == "alpha_c_dropped":                 # the -log(sd) term of Normal.log_prob loses its gradient: dL misses -alpha c
        log_scale = log_scale.detach()
    logp = -((z - mean) ** 2) / (2.0 * sd * sd) - log_scale - math.log(math.sqrt(2.0 * math.pi))
    logp = logp - torch.log(2.0 * (1.0 - u * u) + (0.0 if variant == "no_1e-6" else 1e-6))
    return dict(action=2.0 * u, logp=logp, mean=mean, sd=sd, ls=ls, sraw=sraw, z=z, u=u, pre=[z1, z2])


def _ring(c, dtype):
    n, slots = c["n_envs"], c["slots"]
    i = np.asarray(c["idx"], np.int64)
    nx = ((i // n + 1) % slots) * n + i % n
    obs = _t(c["obs"].reshape(-1, 3), dtype)
    return i, nx, obs


def critic_eval(c, dtype=torch.float64, variant=None):
    """sac.py:170-184 + backward -> dict(losses [2], grads [2 SQ_NP], action / logp of the successor rows, q values, pre-activations)"""
    i, nx, obs = _ring(c, dtype)
    alpha = float(f32(c["alpha"]))
    q = _t(c["q"], dtype, True); qt = _t(c["qt"], dtype); ap = _t(c["actor"], dtype)
    with torch.no_grad():
        a = actor_forward(ap, obs[nx], _t(c["eps_critic"], dtype))
        q1t, p1 = q_forward(qt[:SQ_NP], obs[nx], a["action"])
        q2t, p2 = q_forward(qt[SQ_NP:], obs[nx], a["action"])
        mq = torch.minimum(q1t, q2t) - alpha * a["logp"]
        live = 1.0 - _t(c["term"].reshape(-1)[nx], dtype)
        if variant == "term_ignored":
            live = torch.ones_like(live)
        y = _t(c["rewards"].reshape(-1)[nx], dtype) + live * _t(GAMMA32, dtype) * mq
    act = _t(c["actions"].reshape(-1)[i], dtype)
    q1, p3 = q_forward(q[:SQ_NP], obs[i], act)
    q2, p4 = q_forward(q[SQ_NP:], obs[i], act)
    l1, l2 = torch.mean((q1 - y) ** 2), torch.mean((q2 - y) ** 2)
    (l1 + l2).backward()
    return dict(losses=np.array([l1.item(), l2.item()]), grads=q.grad.numpy().astype(np.float64), action=a["action"].numpy(), logp=a["logp"].numpy(), z=a["z"].numpy(),
                sd=a["sd"].numpy(), ls=a["ls"].numpy(), qgap=(q1t - q2t).abs().numpy(), q=np.stack([q1.detach().numpy(), q2.detach().numpy(), q1t.numpy(), q2t.numpy()]),
                pre=[x.detach().numpy() for x in a["pre"] + p1 + p2 + p3 + p4])


def actor_eval(c, dtype=torch.float64, variant=None, tie_weights=None):
    """sac.py:193-197 + backward -> dict(loss, mlp, grads [AC_NP], ...).  tie_weights (w1, w2): on the rows of c["tie_rows"] min(q1, q2) is replaced by the surrogate
    w1 q1 + w2 q2 (torch.min's half / half routing is (0.5, 0.5)); the other rows keep torch.minimum."""
    i, _, obs = _ring(c, dtype)
    alpha = float(f32(c["alpha"]))
    ap = _t(c["actor"], dtype, True); q = _t(c["q"], dtype)
    a = actor_forward(ap, obs[i], _t(c["eps_actor"], dtype), variant)
    q1, p1 = q_forward(q[:SQ_NP], obs[i], a["action"])
    q2, p2 = q_forward(q[SQ_NP:], obs[i], a["action"])
    mq = torch.minimum(q1, q2)
    if tie_weights is not None:
        tie = torch.tensor(c["tie_rows"])
        mq = torch.where(tie, tie_weights[0] * q1 + tie_weights[1] * q2, mq)
    loss = torch.mean(alpha * a["logp"] - mq)
    loss.backward()
    d = lambda x: x.detach().numpy()
    return dict(loss=loss.item(), mlp=a["logp"].mean().item(), grads=ap.grad.numpy().astype(np.float64), action=d(a["action"]), logp=d(a["logp"]), z=d(a["z"]), sd=d(a["sd"]),
                ls=d(a["ls"]), sraw=d(a["sraw"]), qgap=d((q1 - q2).abs()), q=np.stack([d(q1), d(q2)]), pre=[d(x) for x in a["pre"] + p1 + p2])


def alpha_eval(c, log_alpha, dtype=torch.float64):
    """sac.py:203-208 -> dict(mlp, loss, grad = d alpha_loss / d log_alpha by autograd, action / logp rows)"""
    i, _, obs = _ring(c, dtype)
    with torch.no_grad():
        a = actor_forward(_t(c["actor"], dtype), obs[i], _t(c["eps_alpha"], dtype))
    la = _t([float(f32(log_alpha))], dtype, True)
    loss = torch.mean(-la * (a["logp"] + TARGET_ENTROPY))
    loss.backward()
    return dict(mlp=a["logp"].mean().item(), loss=loss.item(), grad=la.grad.item(), action=a["action"].numpy(), logp=a["logp"].numpy(), z=a["z"].numpy())


# ---- figures ------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def tensor_errors(g, ref, lay):
    """-> {tensor: max |g - ref| over max(that tensor's max |ref|, TENSOR_FLOOR x the network's max |ref|)}"""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    return {k: float(np.abs(g[a:b] - ref[a:b]).max() / max(np.abs(ref[a:b]).max(), TENSOR_FLOOR * top)) for k, (a, b) in lay.items()}


def figures(exp, got):
    """exp / got: dicts with any of critic / actor / alpha (the *_eval results, or the same keys from the oracle or the device) -> {figure: value}; a figure that is
    not finite comes out as inf"""
    f = {k: 0.0 for k in FIGURES}
    up = lambda k, v: f.__setitem__(k, max(f[k], float(v) if np.isfinite(v) else np.inf))
    for part in ("critic", "actor", "alpha"):
        if part not in got:
            continue
        e, g = exp[part], got[part]
        if "action" in g:
            up("action", np.abs(np.asarray(g["action"], np.float64) - e["action"]).max())
            up("logp", np.abs(np.asarray(g["logp"], np.float64) - e["logp"]).max())
        if part == "critic" and "grads" in g:
            for k in range(2):
                sl = slice(k * SQ_NP, (k + 1) * SQ_NP)
                up("loss", abs(g["losses"][k] - e["losses"][k]) / abs(e["losses"][k]))
                up("grad", rel(g["grads"][sl], e["grads"][sl]))
                up("tensor", max(tensor_errors(g["grads"][sl], e["grads"][sl], SQ).values()))
        if part == "actor" and "grads" in g:
            up("loss", abs(g["loss"] - e["loss"]) / abs(e["loss"]))
            up("mlp", abs(g["mlp"] - e["mlp"]))
            up("grad", rel(g["grads"], e["grads"]))
            up("tensor", max(tensor_errors(g["grads"], e["grads"], AC).values()))
        if part == "alpha" and "mlp" in g:
            up("mlp", abs(g["mlp"] - e["mlp"]))
            if "loss" in g:
                up("loss", abs(g["loss"] - e["loss"]) / abs(e["loss"]))
    return f


def oracle_eval(R, c):
    """the f32 oracle (oracle/cpu_ref.py as R) on a case -> the `got` dict of figures()"""
    st = R.SacStorage(c["slots"], c["n_envs"])
    st.observations[:] = c["obs"]; st.actions[:] = c["actions"]; st.rewards[:] = c["rewards"]; st.terminated[:] = c["term"]
    n, slots, idx = c["n_envs"], c["slots"], c["idx"]
    nx = ((idx // n + 1) % slots) * n + idx % n
    flat = c["obs"].reshape(-1, 3)
    got = {}
    a, lp = R.sac_actor_sample(c["actor"], flat[nx], c["eps_critic"])
    g, l = R.sac_critic_grads(c["q"], c["qt"], c["actor"], st, idx, c["eps_critic"], c["alpha"])
    got["critic"] = dict(action=a, logp=lp, grads=g, losses=l)
    a, lp = R.sac_actor_sample(c["actor"], flat[idx], c["eps_actor"])
    g, loss, mlp = R.sac_actor_grads(c["actor"], c["q"], st, idx, c["eps_actor"], c["alpha"])
    got["actor"] = dict(action=a, logp=lp, grads=g, loss=loss, mlp=mlp)
    a, lp = R.sac_actor_sample(c["actor"], flat[idx], c["eps_alpha"])
    mlp = R.sac_mean_logp(c["actor"], st, idx, c["eps_alpha"])
    got["alpha"] = dict(action=a, logp=lp, mlp=mlp, loss=float(-f32(c["log_alpha"])) * (mlp + TARGET_ENTROPY))
    return got


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the family's bound"""
    return {k: (v, factor * BOUND[family][k]) for k, v in fig.items() if not v <= factor * BOUND[family][k]}


# ---- case construction --------------------------------------------------------------------------------------------------------------
def rand_nets(rng):
    """torch-default-like init (the layouts of include/mi_rl.h; as tests/test_gpu_sac.py::_rand_nets) -> actor [AC_NP], two critics [2 SQ_NP]"""
    def lin(o, i):
        b = 1.0 / np.sqrt(i)
        return [rng.uniform(-b, b, (o, i)).astype(f32), rng.uniform(-b, b, o).astype(f32)]
    qs = [np.concatenate([x.reshape(-1) for x in lin(H, 4) + lin(H, H) + lin(1, H)]) for _ in range(2)]
    actor = np.concatenate([x.reshape(-1) for x in lin(H, 3) + lin(H, H) + lin(1, H) + lin(1, H)])
    return actor, np.concatenate(qs)


def _ring_data(rng, n, slots):
    th = rng.uniform(-np.pi, np.pi, (slots, n))
    obs = np.stack([np.cos(th), np.sin(th), rng.uniform(-8, 8, (slots, n))], -1).astype(f32)
    return obs, rng.uniform(-2, 2, (slots, n)).astype(f32), (-rng.uniform(0, 16.2736044, (slots, n))).astype(f32)     # Pendulum's reward range


def _indices(rng, batch, n, slots):
    """-> (idx, terminated [slots, n]): >= 2 rows in the last slot (their successor is slot 0) and one row whose successor is terminated, where batch >= 5"""
    term = np.zeros((slots, n), np.uint8)
    if batch < 5:
        return np.full(batch, (slots - 1) * n, np.int64), term          # the ring's last slot: the successor wraps
    idx = rng.integers(0, (slots - 1) * n, batch)
    idx[0], idx[1] = (slots - 1) * n, slots * n - 1
    if batch > 16:
        idx[16] = (slots - 1) * n + (n - 1) // 2                       # the lone row of the second row group wraps too
    s, e = divmod(int(idx[2]), n)
    term[(s + 1) % slots, e] = 1
    return idx, term


def _targets(family, batch, shift):
    vals = {"A": BAND_A, "B": BAND_B, "C": BAND_C, "AC": BAND_A + BAND_C}[family]
    both = [s * v for v in vals for s in ((1.0, -1.0) if v else (1.0,))]
    if family == "AC":      # interleave so that even a 5-row batch holds both bands
        a = [x for x in both if abs(x) < 6]; cc = [x for x in both if abs(x) > 6]
        both = [x for pair in zip(a, cc * 3) for x in pair] + a[len(cc * 3):]
    return np.array([both[(shift + b) % len(both)] for b in range(batch)])


def _solve_eps(actor, obs_rows, z_target):
    with torch.no_grad():
        a = actor_forward(_t(actor, torch.float64), _t(obs_rows, torch.float64), torch.zeros(len(obs_rows), dtype=torch.float64))
    return ((z_target - a["mean"].numpy()) / a["sd"].numpy()).astype(f32)


def _draw_eps(rng, actor, obs_rows):
    """N(0, 1) draws; a row is drawn again while its |z| lies in ILL"""
    with torch.no_grad():
        a = actor_forward(_t(actor, torch.float64), _t(obs_rows, torch.float64), torch.zeros(len(obs_rows), dtype=torch.float64))
    mean, sd = a["mean"].numpy(), a["sd"].numpy()
    eps = rng.standard_normal(len(obs_rows)).astype(f32)
    for b in range(len(eps)):
        while ILL[0] < abs(mean[b] + sd[b] * float(eps[b])) < ILL[1]:
            eps[b] = f32(rng.standard_normal())
    return eps


def build(i, seed):
    """case i from `seed`, with its float64 expectations under "exp" and the quantities the conditions are about under "cond" """
    name, family, batch, (n, slots), alpha = SPECS[i]
    rng = np.random.default_rng([i, seed])
    actor, q = rand_nets(rng)
    _, qt = rand_nets(rng)
    a, b = AC["WL"]
    actor[a:b] *= f32(0.1)
    actor[AC["BL"][0]] = f32(SRAW.get(name, 1.2))
    actor[AC["BM"][0]] = f32(0.3 if name in SRAW else 0.0)
    obs, actions, rewards = _ring_data(rng, n, slots)
    idx, term = _indices(rng, batch, n, slots)
    nx = ((idx // n + 1) % slots) * n + idx % n
    flat = obs.reshape(-1, 3)
    if name in SRAW:
        eps = [_draw_eps(rng, actor, flat[r]) for r in (nx, idx, idx)]
    else:
        eps = [_solve_eps(actor, flat[r], _targets(family, batch, sh)) for r, sh in ((nx, 0), (idx, 3), (idx, 7))]
    c = dict(name=name, family=family, batch=batch, n_envs=n, slots=slots, alpha=alpha, actor=actor, q=q, qt=qt, obs=obs, actions=actions, rewards=rewards, term=term,
             idx=idx, eps_critic=eps[0], eps_actor=eps[1], eps_alpha=eps[2], log_alpha=-0.3)
    return finish(c)


def finish(c, tie_weights=None):
    """adds the float64 expectations ("exp") and the condition quantities ("cond") to a case"""
    e = dict(critic=critic_eval(c), actor=actor_eval(c, tie_weights=tie_weights), alpha=alpha_eval(c, c["log_alpha"]))
    pre = np.concatenate([np.abs(x).reshape(-1) for part in ("critic", "actor") for x in e[part]["pre"]])
    pre = pre[pre > 0]          # exactly 0 in float64: a unit whose weights and bias are all 0 (the hand-built tie nets) — 0 in f32 as well, masked in every evaluation
    gaps = [e["critic"]["qgap"]]
    if tie_weights is None:
        gaps.append(e["actor"]["qgap"])
    n, slots, idx = c["n_envs"], c["slots"], c["idx"]
    nx = ((idx // n + 1) % slots) * n + idx % n
    c["exp"] = e
    c["cond"] = dict(min_preact=float(pre.min()), n_preact=int(pre.size), min_qgap=float(np.concatenate(gaps).min()),
                     max_eps=float(max(np.abs(c[k]).max() for k in ("eps_critic", "eps_actor", "eps_alpha"))),
                     min_loss=float(min(abs(e["critic"]["losses"][0]), abs(e["critic"]["losses"][1]), abs(e["actor"]["loss"]), abs(e["alpha"]["loss"]))),
                     wraps=int((idx // n == slots - 1).sum()), terminated=int(c["term"].reshape(-1)[nx].sum()),
                     z=np.concatenate([e[p]["z"] for p in ("critic", "actor", "alpha")]))
    return c


def conditions_met(c):
    k = c["cond"]
    ok = k["max_eps"] <= MAX_EPS and k["min_loss"] >= 0.1 and k["min_qgap"] > Q_MARGIN
    if c["family"] in TIGHT:
        ok = ok and k["min_preact"] > NEAR_ZERO
    return bool(ok)


def find_seed(i, start=0, tries=200):
    for seed in range(start, start + tries):
        if conditions_met(build(i, seed)):
            return seed
    raise RuntimeError("no seed for case %d" % i)


@functools.lru_cache(maxsize=None)
def make_case(i):
    """parameters, ring, indices, forced noise and float64 expectations of case i (cached: treat as read-only)"""
    return build(i, SEEDS[i])


# ---- the tie case -------------------------------------------------------------------------------------------------------------------
TIE_EPS, TIE_MEAN, TIE_SRAW = 0.25, 0.2, -0.5
TIE_SEEDS = {5: 4, 17: 42}      # searched like SEEDS (with the oracle's a; the conditions are asserted again with the device's)


def tie_actor():
    """zero weights, mean 0.2, sraw -0.5: with eps = 0.25 on every row, every row takes the same action a = 2 tanh(0.2 + 0.25 sd) > 0"""
    p = np.zeros(AC_NP, f32)
    p[AC["BM"][0]] = TIE_MEAN; p[AC["BL"][0]] = TIE_SRAW
    return p


def make_tie_case(batch, a, seed=None):
    """a: the action the evaluation under test gives tie_actor() with eps = TIE_EPS, as an f32 (read from the device / the oracle first: the tie is in ITS bits).
    Critic 1: unit 0 = relu(action), W2[0, 0] = 1, W3[0] = 1: q1 = a.  Critic 2: the same unit with W3[0] = 2 and b3 = -a: q2 = 2 a - a = a exactly (every product
    is by 1 or 2, every sum has one non-zero term before the bias); its unit 1 = relu(thetadot) adds thetadot on the rows with thetadot > 0, which breaks the tie
    upward there.  So d(-min Q)/da is -(0.5 * 1 + 0.5 * 2) = -1.5 on the tie rows and -1 (critic 1 alone) on the others."""
    a = f32(a)
    assert a > 0
    n, slots = (3, 7) if batch == 5 else (2, 30)
    rng = np.random.default_rng([99, batch, TIE_SEEDS[batch] if seed is None else seed])
    obs, actions, rewards = _ring_data(rng, n, slots)
    idx, term = _indices(rng, batch, n, slots)
    thd = obs.reshape(-1, 3)[idx, 2]
    q = np.zeros(2 * SQ_NP, f32)
    for k in range(2):
        p = q[k * SQ_NP:(k + 1) * SQ_NP]
        p[SQ["W1"][0] + 0 * 4 + 3] = 1          # unit 0 of layer 1: the action
        p[SQ["W2"][0] + 0 * H + 0] = 1          # carried by unit 0 of layer 2
        p[SQ["W3"][0] + 0] = 1 + k
    p[SQ["b3"][0]] = -a
    p[SQ["W1"][0] + 1 * 4 + 2] = 1              # critic 2, unit 1: relu(thetadot)
    p[SQ["W2"][0] + 1 * H + 1] = 1
    p[SQ["W3"][0] + 1] = 1
    _, qt = rand_nets(rng)
    eps = np.full(batch, TIE_EPS, f32)
    c = dict(name="tie_%d" % batch, family="tie", batch=batch, n_envs=n, slots=slots, alpha=0.37, actor=tie_actor(), q=q, qt=qt, obs=obs, actions=actions, rewards=rewards,
             term=term, idx=idx, eps_critic=eps, eps_actor=eps, eps_alpha=eps, log_alpha=-0.3, tie_rows=thd <= 0, a=a)
    return c


def finish_tie(c, weights=(0.5, 0.5)):
    return finish(c, tie_weights=weights)
