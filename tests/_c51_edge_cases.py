"""Placed edge cases on poisoned replay rings for the C51 kernels (deep_rl_amd/csrc/mi_c51.hip) and their float64 expectation — TEST INFRASTRUCTURE
(tests/test_c51_edge_cases_cpu.py validates and measures it, tests/test_gpu_c51_edge_cases.py uses it).  tests/_c51_cases.py (six random draws) stays as it is.

The reference.  c51.py:132-158 restated with torch in float64 on the CPU: the ReLU MLP 4 -> 120 -> 84 -> 2 x 101 in the flat layout of MI_C51_NPARAMS = 27,934
(W1 b1 W2 b2 W3 b3, row-major [unit][k]; W3 row a * 101 + j is atom j of action a), softmax over the atoms, q = sum p z, the greedy action of the TARGET net at the
successor (torch.argmax: the first index on a tie), the categorical projection (clamp, b, floor / ceil, (l == u), scatter-add) under no_grad, and
loss = -(m * log(p + 1e-8)).sum(-1).mean() on the online net's distribution of the stored action.  AUTOGRAD produces the gradient: there is no hand-written backward
here, which makes it independent of c51_grad_kernel and of _c51_ref.loss_grad / project64, two more derivations by hand (the CPU test holds the three together).
The f32 inputs are cast up; gamma is the f32 value the kernel receives.  The two actions' logits are two matrix products of the same shape, so that a head whose
two halves hold the same bits gives the same bits (one 202-column product need not).  `dtype=` runs the same in float32.  `variant=` names a deliberately WRONG
reading, used only by the CPU test to show that the cases tell it from the right one:
  reward_at_row        r[i] instead of r[nx]                                      (NaN: the own reward is poisoned; a NaN b has no atom index and torch raises)
  terminated_at_row    terminated[i] instead of terminated[nx]
  no_wrap              the successor of the last slot is taken from the last slot  (NaN, likewise)
  tie_takes_last       `>=` instead of `>` in the greedy action: a* = 1 on a bit-for-bit tie (shows in next_actions alone: the two distributions are the same bits)
  no_integral_term     the (l == u) term dropped: the mass of an integral b is lost
  no_clamp             the clamp dropped: the scatter's index leaves [0, 100] and torch raises
  relu_one_at_zero     sub-gradient 1 at a pre-activation of exactly 0
  eps_outside_log      log(p) + 1e-8 instead of log(p + 1e-8)
  stray_action_as_1    the stored action read at the successor, where the poison 2 acts as action 1 (c51_grad_kernel's `!= 0`)
  stray_action_masked  the same stray read with a row of action 2 masked out of loss and gradient
  slab_left_out        the last row's slab is not added (the mean still divides by B)
  mean_over_128        division by MI_C51_MAX_SLABS instead of by B

The storage.  Built the way tests/_ddqn_cases.py builds its rings, on the rings (n_envs, slots) of _dqn_cases.RINGS: (1, 2) for one row, (3, 7) up to 9 rows, (2, 30)
up to 40, (129, 40) beyond.  The batch is drawn WITH repetition; with >= 5 rows two entries are moved into the last slot (their successor wraps to slot 0) and one
entry repeats another; the one-row case sits in the last slot of the two-slot ring.  Every observation and reward that the batch does not reference, as a row or as
a successor, holds NaN; unreferenced actions hold 2, unreferenced terminated flags 1.  The OWN reward of a sampled row that is not another sampled row's successor
holds NaN too and its own flag is 1.  The observation of a sampled row is redrawn until no online pre-activation (float64) of that row lies within NEAR_ZERO of 0,
placed units aside.  Nothing is asked of the target net's pre-activations: ReLU is continuous and nothing is differentiated through the target.
edge_rewards_9 alone has NO repeated index: nine rows with a repetition have at most eight successors, and the family is its nine rewards, one per successor.

Parameters.  _c51_cases.default_init (torch's default scale, head spread x 3), an independent draw for each net.

The families (SPECS).  MI_C51_MAX_SLABS = 128; workgroup g walks rows g, g + 128, ...; rg_reduce (mi_ring.h) adds the slabs in 16 groups x 4 interleaved accumulators.
  plain          batch 1, 5, 16, 17, 48, 49, 64, 65, 127, 129, 300: every tail of the slab sum (the first, second, third and fourth accumulator ending on a full and
                 on a partial pass of 16), one row more than the launch has workgroups, workgroups that walk three rows.  Rewards are _c51_cases.REWARDS dealt in
                 turn (the clamp at both ends, fractional and integral b); about a third of the successors terminated
  target_tie     batch 9: the target head's rows and biases of action 1 are action 0's: q0 == q1 bit for bit, a* is 0 on every row
  terminal       batch 9: every successor terminated (each target_probs row has at most two non-zero atoms); batch 17: none
  gamma          batch 17 at gamma 0.0 and at 1.0; rewards {0, 2, -2, 1, 200, -200} dealt in turn, at gamma 1 each of them on a live row: there the projection is
                 a shift by whole or half atoms and its results are exact in f32 (gamma1_identities)
  edge_rewards   batch 9, every successor terminated, rewards EDGE_REWARDS: b at exactly 0 and 100 (l == u at both ends of the index range), at 99.5 and 0.5, one
                 step past the clamp and far past it, and two interior fractions
  scale          batch 17 with both nets' heads scaled by 30 and by 100: saturated softmax; at x 100 the f32 probabilities hold exact zeros where float64 has 1e-100
                 and less, so loss and gradient run on the + 1e-8 alone
  kink_placed    batch 8: four first-layer units (0, 119 and two more) and four second-layer units (0, 83 and two more) of the online net with zero weights and bias
                 (_dqn_cases._place_params: the torso offsets are the same): pre-activation exactly 0 in every row and every precision
  dead           batch 8: online b2 = -1e3: h2 == 0 in every row, every float64 gradient element outside b3 is exactly 0
  single_action  batch 9: every sampled row stored action 0: rows 101 .. 201 of dW3 and of db3 are exactly 0
  bad_index      batch 5: the indices -1 and slots * n_envs among valid ones; "a bad index reads a valid row": the expectation is that of the same batch with
                 -1 -> 0 and slots * n_envs -> slots * n_envs - 1 ("eidx"); the ring is built (and poisoned) around those rows

Conditions (asserted by the CPU test on the float64 reference; SEEDS holds the first seed from 0 that meets them, find_seed).  NO ROW IS EXCLUDED FROM ANY COMPARISON,
actions included.  With >= 5 rows: >= 2 wrapping rows, >= 1 repeated index (edge_rewards aside), both stored actions among the sampled rows (single_action aside) and,
outside terminal and edge_rewards, >= 1 terminated and >= 1 live successor.  With >= 16 rows a* takes both values.  At least one sampled row has a NaN own reward.
No online pre-activation of a sampled row lies within NEAR_ZERO of 0, placed units aside.  On EVERY successor the target net's |q0 - q1| is >= CLOSE_Q of the family,
target_tie aside, where it is exactly 0.  gamma_1: every reward of GAMMA_REWARDS on a live row.  terminal: all / none terminated.

Figures.  "target_probs", "probs", "q": max |x - x64|, absolute (q: the target net's action values at the successors; the device's are the forward API's).  "loss":
|x - ref| / |ref|.  "grad": max |g - ref| / max |ref|.  A NaN where the reference is finite makes the figure inf.

Bounds.  MEASURED[family][figure] is what tests/test_c51_edge_cases_cpu.py measures for the f32 restatement (_c51_ref.target and loss_grad, the latter through the
restatement's own target_probs) against this file's float64, the maximum over the family's cases (the test ties the constants to the measurement: a constant covers
its figure and is at most 1.25 x it).  BOUND[family][figure] = max(8 x MEASURED, the shipped _c51_ref.BOUND_* that tests/test_gpu_c51_cases.py holds the kernel to).
CLOSE_Q[family] = 2 x the family's q bound.  No bound comes from the kernel's output.

Not asserted, because it does not hold for C51: an all-terminated batch still reads the target net (its probabilities weight the 101 colliding contributions, so
another target vector moves rounding bits of target_probs), and the masses of edge_rewards are 1 - O(2^-23), not exactly 1.
"""
import functools

import numpy as np
import torch

import _c51_cases as K0
import _c51_ref as X
import _dqn_cases as D

f32 = np.float32
NP, NA, H1, H2 = X.NPARAMS, X.N_ATOMS, X.H1, X.H2
W3, B3 = X.OFF["W3"], X.OFF["b3"]
NEAR_ZERO = D.NEAR_ZERO
MAX_SLABS = 128
VARIANTS = ("reward_at_row", "terminated_at_row", "no_wrap", "tie_takes_last", "no_integral_term", "no_clamp", "relu_one_at_zero", "eps_outside_log",
            "stray_action_as_1", "stray_action_masked", "slab_left_out", "mean_over_128")
FIGURES = ("target_probs", "probs", "loss", "grad", "q")
GAMMA_REWARDS = np.array([0.0, 2.0, -2.0, 1.0, 200.0, -200.0], f32)
# (reward, the atoms that hold mass) with every successor terminated: b = (clamp(r) + 100) / 2
EDGE_REWARDS = ((-100.0, (0,)), (100.0, (100,)), (99.0, (99, 100)), (-99.0, (0, 1)), (100.5, (100,)), (-1e6, (0,)), (1e6, (100,)), (0.5, (50, 51)), (-7.25, (46, 47)))


def _spec(name, family, mb, **opt):
    ring = D.RINGS[0] if mb == 1 else D.RINGS[1] if mb <= 9 else D.RINGS[2] if mb <= 40 else D.RINGS[3]
    return dict(dict(name=name, family=family, mb=mb, ring=ring, gamma=0.99, p_term=1.0 / 3.0, head_scale=1.0, place=None, rewards="mixed"), **opt)


SPECS = tuple(_spec("plain_%d" % mb, "plain", mb) for mb in (1, 5, 16, 17, 48, 49, 64, 65, 127, 129, 300)) + (
    _spec("target_tie_9", "target_tie", 9, place="target_tie"),
    _spec("terminal_all_9", "terminal", 9, p_term=1.0),
    _spec("terminal_none_17", "terminal", 17, p_term=0.0),
    _spec("gamma_0_17", "gamma", 17, gamma=0.0, rewards="gamma"),
    _spec("gamma_1_17", "gamma", 17, gamma=1.0, rewards="gamma"),
    _spec("edge_rewards_9", "edge_rewards", 9, p_term=1.0, rewards="edge"),
    _spec("scale_30_17", "scale", 17, head_scale=30.0),
    _spec("scale_100_17", "scale", 17, head_scale=100.0),
    _spec("kink_placed_8", "kink_placed", 8, place="kink"),
    _spec("dead_8", "dead", 8, place="dead"),
    _spec("single_action_9", "single_action", 9, place="single_action"),
    _spec("bad_index_5", "bad_index", 5, place="bad_index"),
)
NAMES = tuple(s["name"] for s in SPECS)
FAMILIES = tuple(dict.fromkeys(s["family"] for s in SPECS))
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0)

# measured by tests/test_c51_edge_cases_cpu.py: the f32 restatement against this file's float64, maximum over the family's cases   (measured: the same position)
MEASURED = {                   # figures in the order of FIGURES
    "plain": dict(target_probs=5.2e-7, probs=2.9e-8, loss=1.8e-7, grad=2.2e-6, q=2.9e-6),             # 4.77e-7 2.64e-8 1.61e-7 1.99e-6 2.63e-6
    "target_tie": dict(target_probs=1.4e-7, probs=1.3e-8, loss=1.9e-7, grad=1.6e-7, q=1.5e-6),        # 1.30e-7 1.19e-8 1.71e-7 1.46e-7 1.38e-6
    "terminal": dict(target_probs=2.6e-7, probs=1.8e-8, loss=1.4e-7, grad=2.5e-7, q=4.5e-6),          # 2.38e-7 1.60e-8 1.29e-7 2.30e-7 4.14e-6
    "gamma": dict(target_probs=2.6e-7, probs=9.9e-9, loss=7.0e-8, grad=4.0e-7, q=2.1e-6),             # 2.38e-7 9.00e-9 6.40e-8 3.62e-7 1.89e-6
    "edge_rewards": dict(target_probs=1.3e-7, probs=1.1e-8, loss=4.0e-8, grad=2.3e-7, q=1.6e-6),      # 1.19e-7 1.03e-8 3.66e-8 2.05e-7 1.46e-6
    # scale: a saturated softmax passes the logits' f32 error (logits of several hundred) on to the probabilities at full weight
    "scale": dict(target_probs=2.4e-6, probs=3.5e-6, loss=6.2e-8, grad=7.7e-6, q=2.7e-4),             # 2.16e-6 3.17e-6 5.59e-8 6.95e-6 2.41e-4
    "kink_placed": dict(target_probs=1.3e-7, probs=8.0e-9, loss=1.0e-8, grad=2.5e-7, q=2.3e-6),       # 1.19e-7 7.32e-9 9.48e-9 2.29e-7 2.07e-6
    "dead": dict(target_probs=1.8e-7, probs=2.2e-9, loss=3.9e-8, grad=1.8e-7, q=1.9e-6),              # 1.63e-7 2.01e-9 3.52e-8 1.65e-7 1.75e-6
    "single_action": dict(target_probs=2.0e-7, probs=6.6e-9, loss=9.9e-9, grad=2.8e-7, q=8.4e-7),     # 1.79e-7 5.97e-9 9.01e-9 2.52e-7 7.61e-7
    "bad_index": dict(target_probs=1.3e-7, probs=6.2e-9, loss=4.2e-8, grad=1.7e-7, q=1.2e-6),         # 1.19e-7 5.68e-9 3.84e-8 1.57e-7 1.07e-6
}
SHIPPED = dict(target_probs=X.BOUND_TARGET_PROBS_ABS, probs=X.BOUND_PROBS_ABS, loss=X.BOUND_LOSS_REL, grad=X.BOUND_GRAD_REL, q=X.BOUND_Q_ABS)
BOUND = {fam: {k: max(8.0 * m[k], SHIPPED[k]) for k in FIGURES} for fam, m in MEASURED.items()}
CLOSE_Q = {fam: 2.0 * b["q"] for fam, b in BOUND.items()}


# ---- the reference: c51.py:132-158 in torch, any dtype, the gradient by autograd ------------------------------------------------------
def _t(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def logits(p, x, variant=None):
    """nn.Sequential(Linear(4, 120), ReLU, Linear(120, 84), ReLU, Linear(84, 202)) on the flat vector p -> (logits [rows, 2, 101], z1, z2)"""
    relu = D._ReluOneAtZero.apply if variant == "relu_one_at_zero" else torch.relu
    s = lambda k, n, shape: p[X.OFF[k]:X.OFF[k] + n].reshape(shape)   # noqa: E731
    z1 = x @ s("W1", 4 * H1, (H1, 4)).T + s("b1", H1, (H1,))
    z2 = relu(z1) @ s("W2", H1 * H2, (H2, H1)).T + s("b2", H2, (H2,))
    h2 = relu(z2)
    w, b = s("W3", 2 * NA * H2, (2, NA, H2)), s("b3", 2 * NA, (2, NA))
    return torch.stack([h2 @ w[0].T + b[0], h2 @ w[1].T + b[1]], dim=1), z1, z2


def project(next_probs, r, live, gamma, variant=None):
    """c51.py:132-154 on torch tensors of one dtype -> (m [rows, 101], b)"""
    atoms = torch.tensor(X.ATOMS.astype(np.float64), dtype=next_probs.dtype)
    tz = r[:, None] + float(f32(gamma)) * atoms[None, :] * live[:, None]
    if variant != "no_clamp":
        tz = torch.clamp(tz, -100.0, 100.0)
    b = (tz + 100.0) / 2.0
    lo, up = b.floor(), b.ceil()
    eq = torch.zeros_like(b) if variant == "no_integral_term" else (lo == up).to(b.dtype)
    m = torch.zeros_like(next_probs)
    m.scatter_add_(1, lo.long(), (up + eq - b) * next_probs)           # (raises on an index outside [0, 100])
    m.scatter_add_(1, up.long(), (b - lo) * next_probs)
    return m, b


def evaluate(c, dtype=torch.float64, variant=None):
    """-> dict(grads, loss, next_actions, target_probs, next_probs (the greedy action's), probs, q (target net, successors), live, b, z1, z2) as float64 / int64 numpy"""
    assert variant is None or variant in VARIANTS
    N, S = c["ring"]
    idx, mb = c["eidx"], c["mb"]
    nx = D.successor(idx, N, S, variant)
    flat = lambda k: c[k].reshape((N * S,) + c[k].shape[2:])   # noqa: E731
    obs = flat("observations")
    rows = torch.arange(mb)
    atoms = torch.tensor(X.ATOMS.astype(np.float64), dtype=dtype)
    with torch.no_grad():
        pt = torch.softmax(logits(_t(c["target"], dtype), _t(obs[nx], dtype))[0], dim=-1)
        q = (pt * atoms).sum(-1)
        a_star = (q[:, 1] >= q[:, 0]).long() if variant == "tie_takes_last" else torch.argmax(q, dim=1)
        nextp = pt[rows, a_star]
        r = _t(flat("rewards")[idx if variant == "reward_at_row" else nx], dtype)
        live = _t(1.0 - flat("terminated")[idx if variant == "terminated_at_row" else nx].astype(np.float64), dtype)
        m, b = project(nextp, r, live, c["gamma"], variant)
    p = _t(c["params"], dtype, True)
    L, z1, z2 = logits(p, _t(obs[idx], dtype), variant)
    act = flat("actions")[nx if variant in ("stray_action_as_1", "stray_action_masked") else idx]
    keep = torch.ones(mb, dtype=dtype)
    if variant == "stray_action_masked":
        keep = _t((act != 2).astype(np.float64), dtype)
    if variant == "slab_left_out":
        keep[mb - 1] = 0.0
    probs = torch.softmax(L, dim=-1)[rows, torch.from_numpy((act != 0).astype(np.int64))]
    logp = torch.log(probs) + 1e-8 if variant == "eps_outside_log" else torch.log(probs + 1e-8)
    rowloss = -(m * logp).sum(-1) * keep
    loss = rowloss.sum() / (MAX_SLABS if variant == "mean_over_128" else mb)
    loss.backward()
    d = lambda x: x.detach().numpy().astype(np.float64)   # noqa: E731
    return dict(grads=d(p.grad), loss=float(loss.item()), next_actions=a_star.numpy().astype(np.int64), target_probs=d(m), next_probs=d(nextp), probs=d(probs), q=d(q),
                live=d(live), b=d(b), z1=d(z1), z2=d(z2))


def batch_of(c):
    """the rows of the case's batch as the kernels gather them -> (X, A, X_next, R, T)"""
    N, S = c["ring"]
    idx = c["eidx"]
    nx = D.successor(idx, N, S)
    flat = lambda k: c[k].reshape((N * S,) + c[k].shape[2:])   # noqa: E731
    return flat("observations")[idx], flat("actions")[idx], flat("observations")[nx], flat("rewards")[nx], flat("terminated")[nx]


def restate32(c):
    """the f32 restatement (tests/_c51_ref.py) on a case, the loss and gradient through its own target_probs -> the `got` dict of figures()"""
    Xb, A, Xn, Rw, Tm = batch_of(c)
    na, m, q = X.target(c["target"], Xn, Rw, Tm, gamma=c["gamma"])
    loss, g, p = X.loss_grad(c["params"], Xb, A, m)
    return dict(grads=g.astype(np.float64), loss=float(loss), next_actions=na, target_probs=m.astype(np.float64), probs=p.astype(np.float64), q=q.astype(np.float64))


# ---- figures ------------------------------------------------------------------------------------------------------------------------
def _dist(g, r):
    g, r = np.asarray(g, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    assert np.isfinite(r).all(), "the float64 reference itself is not finite"
    return float(np.abs(g - r).max()) if np.isfinite(g).all() else np.inf


def figures(exp, got):
    """exp: evaluate()'s float64 result; got: grads, loss, target_probs, probs, q from another evaluation or the device"""
    return dict(target_probs=_dist(got["target_probs"], exp["target_probs"]), probs=_dist(got["probs"], exp["probs"]), q=_dist(got["q"], exp["q"]),
                loss=_dist([got["loss"]], [exp["loss"]]) / abs(exp["loss"]), grad=_dist(got["grads"], exp["grads"]) / float(np.abs(exp["grads"]).max()))


def within(fig, family, factor=1.0):
    """-> the figures that exceed factor x the bound of the family"""
    b = BOUND[family]
    return {k: (v, factor * b[k]) for k, v in fig.items() if not v <= factor * b[k]}


def gamma1_identities(m, p, r, live):
    """the exact f32 results of the projection at gamma 1 on live rows: m, p [rows, 101] f32 (p: the greedy action's next-distribution), r [rows], live [rows] bool
    -> the number of rows checked per reward; raises AssertionError where an identity does not hold bit for bit"""
    m, p = np.asarray(m, f32), np.asarray(p, f32)
    seen = {}
    eq = lambda a, b: np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))   # noqa: E731
    half = f32(0.5)
    for k in np.flatnonzero(live):
        rk = float(r[k])
        seen[rk] = seen.get(rk, 0) + 1
        if rk == 0.0:
            assert eq(m[k], p[k])
        elif rk == 2.0:
            assert eq(m[k, 1:100], p[k, 0:99]) and eq(m[k, 100], p[k, 99] + p[k, 100]) and m[k, 0] == 0
        elif rk == -2.0:
            assert eq(m[k, 1:100], p[k, 2:101]) and eq(m[k, 0], p[k, 0] + p[k, 1]) and m[k, 100] == 0
        elif rk == 1.0:
            assert eq(m[k, 1:100], half * p[k, 1:100] + half * p[k, 0:99]) and eq(m[k, 100], p[k, 100] + half * p[k, 99]) and eq(m[k, 0], half * p[k, 0])
        elif rk == 200.0:
            assert not m[k, :100].any() and abs(float(m[k, 100]) - 1) <= NA * 2.0 ** -23
        elif rk == -200.0:
            assert not m[k, 1:].any() and abs(float(m[k, 0]) - 1) <= NA * 2.0 ** -23
        else:
            raise AssertionError("reward %r is not one of GAMMA_REWARDS" % rk)
    return seen


# ---- case construction --------------------------------------------------------------------------------------------------------------
def _zero_gap(z1, z2, units):
    return D._zero_gap(z1, z2, units)


def _deal(rng, values, n):
    """n draws that hold every value in turn, in random order"""
    return values[rng.permutation(n) % len(values)]


def build(i, seed):
    """case i from `seed`, with its float64 expectation under "exp" and the quantities the conditions are about under "cond" """
    s = SPECS[i]
    rng = np.random.default_rng([i, seed, 51])
    (N, S), mb, place = s["ring"], s["mb"], s["place"]
    cap = N * S
    last = lambda: (S - 1) * N + int(rng.integers(0, N))   # noqa: E731
    idx = rng.integers(0, cap, mb)
    if mb == 1:
        idx[0] = last()
    elif s["rewards"] == "edge":                           # nine distinct rows, two of them in the last slot
        idx = np.concatenate([(S - 1) * N + rng.choice(N, 2, replace=False), rng.choice((S - 1) * N, mb - 2, replace=False)])
        rng.shuffle(idx)
    elif place == "bad_index":
        idx[0], idx[1], idx[2], idx[4] = last(), -1, cap, idx[3]
        rng.shuffle(idx)
    elif mb >= 5:
        idx[0], idx[1], idx[mb - 1] = last(), last(), idx[2]
        rng.shuffle(idx)
    idx = idx.astype(np.int64)
    eidx = np.clip(idx, 0, cap - 1)                        # rg_row_index / c51_target_kernel: a bad index reads a valid row
    nx = D.successor(eidx, N, S)
    rows, succ = np.unique(eidx), np.unique(nx)
    params, target = K0.default_init(rng), K0.default_init(rng)                                    # an independent draw for each net
    if s["head_scale"] != 1.0:
        for v in (params, target):
            v[W3:] = (v[W3:].astype(np.float64) * s["head_scale"]).astype(f32)
    units = D._place_params(dict(place={"kink": "kink", "dead": "dead2"}.get(place), head_scale=1.0), rng, dict(params=params, dparams=params))
    if place == "target_tie":
        target[W3 + NA * H2:B3] = target[W3:W3 + NA * H2]
        target[B3 + NA:] = target[B3:B3 + NA]
    obs = np.full((cap, 4), np.nan, f32)
    ref = np.union1d(rows, succ)
    obs[ref] = D._draw_obs(rng, len(ref))
    for _ in range(100):                                   # a sampled row's observation is redrawn until its online pre-activations are clear of 0
        z1, z2 = X.forward64(params, obs[rows])[2:]
        bad = rows[_zero_gap(z1, z2, units) <= NEAR_ZERO]
        if not len(bad):
            break
        obs[bad] = D._draw_obs(rng, len(bad))
    rewards = np.full(cap, np.nan, f32)
    if s["rewards"] == "edge":
        rewards[nx] = np.array([r for r, _ in EDGE_REWARDS], f32)                                  # row k's successor holds EDGE_REWARDS[k]
    else:
        rewards[succ] = _deal(rng, GAMMA_REWARDS if s["rewards"] == "gamma" else K0.REWARDS, len(succ))
    terminated = np.ones(cap, np.uint8)
    terminated[succ] = rng.random(len(succ)) < s["p_term"]
    actions = np.full(cap, 2, np.int64)
    actions[rows] = 0 if place == "single_action" else rng.integers(0, 2, len(rows))
    c = dict(s, params=params, target=target, idx=idx, eidx=eidx, observations=obs.reshape(S, N, 4), rewards=rewards.reshape(S, N),
             terminated=terminated.reshape(S, N), actions=actions.reshape(S, N), units=units)
    return finish(c)


def finish(c):
    N, S = c["ring"]
    idx, mb = c["eidx"], c["mb"]
    e = c["exp"] = evaluate(c)
    live = e["live"] > 0
    flat = lambda k: c[k].reshape(-1)   # noqa: E731
    r_next = flat("rewards")[D.successor(idx, N, S)]
    c["cond"] = dict(rows=int(len(idx)), wraps=int((idx // N == S - 1).sum()), repeats=int(mb - len(np.unique(idx))),
                     poisoned=float(np.isnan(flat("rewards")[idx]).mean()), zero_gap=float(_zero_gap(e["z1"], e["z2"], c["units"]).min()),
                     terminated=int((~live).sum()), live=int(live.sum()), q_gap=float(np.abs(e["q"][:, 0] - e["q"][:, 1]).min()),
                     a_star=sorted(set(e["next_actions"].tolist())), stored=sorted(set(flat("actions")[idx].tolist())),
                     live_rewards=sorted(set(r_next[live].tolist())), bad=int((c["idx"] != c["eidx"]).sum()))
    return c


def conditions_met(c):
    k, fam, mb = c["cond"], c["family"], c["mb"]
    ok = k["rows"] == mb and k["zero_gap"] > NEAR_ZERO and k["poisoned"] > 0 and np.isfinite(c["exp"]["grads"]).all()
    if mb == 1:
        ok = ok and k["wraps"] == 1
    if mb >= 5:
        ok = ok and k["wraps"] >= 2 and (k["repeats"] >= 1 or fam == "edge_rewards")
        ok = ok and k["stored"] == ([0] if fam == "single_action" else [0, 1])
        if fam not in ("terminal", "edge_rewards"):
            ok = ok and k["terminated"] >= 1 and k["live"] >= 1
    if mb >= 16:
        ok = ok and k["a_star"] == [0, 1]
    if fam in ("terminal", "edge_rewards"):
        ok = ok and k["terminated"] == (mb if c["p_term"] == 1.0 else 0)
    if c["name"] == "gamma_1_17":
        ok = ok and k["live_rewards"] == sorted(GAMMA_REWARDS.tolist())
    if fam == "bad_index":
        ok = ok and k["bad"] == 2 and 0 in c["eidx"] and c["ring"][0] * c["ring"][1] - 1 in c["eidx"]
    if fam == "target_tie":
        ok = ok and k["q_gap"] == 0.0 and k["a_star"] == [0]
    else:
        ok = ok and k["q_gap"] >= CLOSE_Q[fam]
    return bool(ok)


def find_seed(i, start=0, tries=200):
    for seed in range(start, start + tries):
        if conditions_met(build(i, seed)):
            return seed
    raise RuntimeError("no seed for case %d" % i)


@functools.lru_cache(maxsize=None)
def make_case(i):
    """parameters, ring, indices and float64 expectation of case i (cached: treat as read-only)"""
    return build(i, SEEDS[i])
