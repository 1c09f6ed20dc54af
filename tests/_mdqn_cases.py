"""Synthetic replay rings for the Munchausen DQN kernels (deep_rl_amd/csrc/mi_mdqn.hip) and their float64 expectations — TEST INFRASTRUCTURE
(tests/test_mdqn_cases_cpu.py validates it, tests/test_gpu_mdqn_cases.py uses it).  The reference is tests/_mdqn_ref.py.

The storage is built the way tests/_ddqn_cases.py builds its rings, with tests/_dqn_cases.py's helpers: rings (n_envs, slots) = (1, 2) for one row, (3, 7) up to 9
rows, (2, 30) up to 40, (129, 40) beyond; the batch is drawn WITH repetition; with >= 5 rows two entries are moved into the last slot (their successor wraps to slot
0) and one entry repeats another; the one-row case sits in the last slot of the two-slot ring.  Rewards of the successors are distinct draws from N(0, r_std).  Every
observation and reward that the batch does not reference, as a row or as a successor, holds NaN; unreferenced actions hold 2, unreferenced terminated flags 1; the OWN
reward of a sampled row that is not some other sampled row's successor holds NaN too and its own flag is 1.  The observation of a sampled row is redrawn until no
online pre-activation of that row lies within NEAR_ZERO of 0.  The TARGET network is an independent draw, as in _ddqn_cases.py.

The families (SPECS); alpha, tau, clip_lo = 0.9, 0.03, -1.0 unless said.  The gradient launch has MI_MD_MAX_SLABS = 128 workgroups; workgroup g walks rows g, g + 128, ...
  plain          batch 1 (the row in the last slot of the (1, 2) ring), 5 on (3, 7), 129 (workgroup 0 walks two rows), 300 (workgroups 0 .. 43 walk three)
  clip           batch 17, both nets' heads scaled by 30, rewards N(0, 10): >= 3 rows clipped at clip_lo, >= 3 rows strictly inside (clip_lo, 0), >= 1 row exactly 0
  tau_1          batch 17, tau = 1: the entropy term is large
  tau_underflow  batch 17, tau = the largest power of two <= (the smallest float64 gap of the target network's action values over the successors) / 256, so
                 (q_max - q_min) / tau >= 128 at every successor in float32 as well: soft_value is the target network's maximum
  alpha          batch 17: alpha 0.0 and 1.0
  terminal       batch 9: every successor terminated; batch 17: none
  gamma          batch 17: gamma 0.0 and 1.0
  target_tie     batch 9: both target head rows and biases are equal: next_actions are all 0 and tau ln pi_a = -tau ln 2 on every row
  kink_placed    batch 8: four first-layer and four second-layer units of the online net with zero weights and bias: exact zeros in the float64 gradient must be
                 exact zeros on the device
  ddqn_identity  batch 17: target == online bit for bit, alpha = 0, tau as in tau_underflow: every output is Double DQN's

Conditions (asserted by the CPU test on the float64 reference; SEEDS holds the first seed from 0 that meets them, find_seed).  No row is excluded from any
comparison.  With >= 5 rows: >= 2 wrapping rows, >= 1 repeated index, >= 1 terminated successor outside the terminal family.  No online pre-activation of a sampled
row lies within NEAR_ZERO of 0, placed units aside.  On EVERY successor the target network's |q0 - q1| is >= CLOSE_Q of the family (the target_tie case aside, where it
is exactly 0).  No row's tau ln pi_a lies within CLOSE_CLIP of clip_lo; in the clip family none lies within CLOSE_CLIP of 0 either unless it is exactly 0.  That
second clause cannot be asked of the other families: at tau = 0.03 the greedy stored action of a row whose action values lie 0.24 .. 1.1 apart has
tau ln pi_a in (-1e-5, 0) without being 0, which is most rows of a freshly drawn network.  Nothing hangs on it: u_a <= 0 and lse >= 0 make tau ln pi_a <= 0 in every
precision, so the upper end of the clamp never moves a value, near 0 or not.  |loss| >= LOSS_FLOOR.
"""
import functools

import numpy as np

import _dqn_cases as D
import _mdqn_ref as X

f32 = np.float32
NEAR_ZERO, LOSS_FLOOR = D.NEAR_ZERO, D.LOSS_FLOOR
MAX_SLABS = 128


def _spec(name, family, mb, **opt):
    ring = D.RINGS[0] if mb == 1 else D.RINGS[1] if mb <= 9 else D.RINGS[2] if mb <= 40 else D.RINGS[3]
    return dict(dict(name=name, family=family, mb=mb, ring=ring, gamma=0.99, p_term=1.0 / 3.0, head_scale=1.0, r_std=1.0, place=None, hp=dict(X.HP), tau_rule=None), **opt)


_hp = lambda **kw: dict(X.HP, **kw)   # noqa: E731
SPECS = (
    _spec("plain_1", "plain", 1),
    _spec("plain_5", "plain", 5),
    _spec("plain_129", "plain", MAX_SLABS + 1),
    _spec("plain_300", "plain", 300),
    _spec("clip_17", "clip", 17, head_scale=30.0, r_std=10.0),
    _spec("tau_1_17", "tau_1", 17, hp=_hp(tau=1.0)),
    _spec("tau_underflow_17", "tau_underflow", 17, tau_rule="underflow"),
    _spec("alpha_0_17", "alpha", 17, hp=_hp(alpha=0.0)),
    _spec("alpha_1_17", "alpha", 17, hp=_hp(alpha=1.0)),
    _spec("terminal_all_9", "terminal", 9, p_term=1.0),
    _spec("terminal_none_17", "terminal", 17, p_term=0.0),
    _spec("gamma_0_17", "gamma", 17, gamma=0.0),
    _spec("gamma_1_17", "gamma", 17, gamma=1.0),
    _spec("target_tie_9", "target_tie", 9, place="target_tie"),
    _spec("kink_placed_8", "kink_placed", 8, place="kink"),
    _spec("ddqn_identity_17", "ddqn_identity", 17, place="synced", hp=_hp(alpha=0.0), tau_rule="underflow"),
)
NAMES = tuple(s["name"] for s in SPECS)
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (2, 0, 0, 0, 28, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)


def underflow_tau(gaps):
    """the largest power of two <= min(gaps) / 256"""
    return float(2.0 ** np.floor(np.log2(float(np.min(gaps)) / 256.0)))


def build(i, seed):
    """case i from `seed`, with its float64 expectation under "exp" and the quantities the conditions are about under "cond" """
    s = SPECS[i]
    rng = np.random.default_rng([i, seed, 2020])
    (N, S), mb = s["ring"], s["mb"]
    cap = N * S
    last = lambda: (S - 1) * N + int(rng.integers(0, N))   # noqa: E731
    idx = rng.integers(0, cap, mb)
    if mb == 1:
        idx[0] = last()
    if mb >= 5:
        idx[0], idx[1], idx[mb - 1] = last(), last(), idx[2]
        rng.shuffle(idx)
    idx = idx.astype(np.int64)
    nx = D.successor(idx, N, S)
    rows, succ = np.unique(idx), np.unique(nx)
    params, dparams = D.init_params(rng)
    target, dtarget = D.init_params(rng)                                                          # an independent draw
    nets = dict(params=params, dparams=dparams, target=target, dtarget=dtarget)
    units = D._place_params(dict(place=s["place"] if s["place"] in ("kink", "target_tie") else None, head_scale=s["head_scale"]), rng, nets)
    if s["place"] == "synced":
        nets["target"] = params.copy()
    obs = np.full((cap, 4), np.nan, f32)
    ref = np.union1d(rows, succ)
    obs[ref] = D._draw_obs(rng, len(ref))
    for _ in range(100):                                   # a sampled row's observation is redrawn until its online pre-activations are clear of 0
        bad = rows[D._zero_gap(*D._preacts64(params, obs[rows]), units) <= NEAR_ZERO]
        if not len(bad):
            break
        obs[bad] = D._draw_obs(rng, len(bad))
    rewards = np.full(cap, np.nan, f32)
    while True:
        rewards[succ] = rng.normal(0, s["r_std"], len(succ)).astype(f32)
        if len(np.unique(rewards[succ])) == len(succ):
            break
    terminated = np.ones(cap, np.uint8)
    terminated[succ] = rng.random(len(succ)) < s["p_term"]
    actions = np.full(cap, 2, np.int64)
    actions[rows] = rng.integers(0, 2, len(rows))
    hp = dict(s["hp"])
    if s["tau_rule"] == "underflow":                       # from the float64 values of the target network at the successors
        qt = X.forward(nets["target"], obs[nx])
        hp["tau"] = underflow_tau(np.abs(qt[:, 0] - qt[:, 1]))
    c = dict(s, hp=hp, params=nets["params"], target=nets["target"], idx=idx, observations=obs.reshape(S, N, 4), rewards=rewards.reshape(S, N),
             terminated=terminated.reshape(S, N), actions=actions.reshape(S, N), units=units)
    return finish(c)


def finish(c):
    N, S = c["ring"]
    idx, mb = c["idx"], c["mb"]
    e = c["exp"] = X.evaluate(c)
    live = e["live"] > 0
    clip_lo, slp = float(f32(c["hp"]["clip_lo"])), e["slp"]
    inside = (slp > clip_lo) & (slp < 0)
    edge = np.abs(slp - clip_lo)
    if c["family"] == "clip":
        edge = np.minimum(edge, np.where(slp == 0, np.inf, np.abs(slp)))
    c["cond"] = dict(rows=int(len(idx)), wraps=int((idx // N == S - 1).sum()), repeats=int(mb - len(np.unique(idx))),
                     poisoned=float(np.isnan(c["rewards"].reshape(-1)[idx]).mean()), zero_gap=float(D._zero_gap(e["z1"], e["z2"], c["units"]).min()),
                     loss=e["loss"], terminated=int((~live).sum()), q_gap=float(np.abs(e["qt_next"][:, 0] - e["qt_next"][:, 1]).min()),
                     clipped=int((slp < clip_lo).sum()), inside=int(inside.sum()), zero=int((slp == 0).sum()), clip_gap=float(edge.min()),
                     ratio=float((np.abs(e["qt_next"][:, 0] - e["qt_next"][:, 1]) / float(f32(c["hp"]["tau"]))).min()))
    return c


def conditions_met(c):
    k, fam = c["cond"], c["family"]
    ok = k["rows"] == c["mb"] and k["zero_gap"] > NEAR_ZERO and abs(k["loss"]) >= LOSS_FLOOR and k["clip_gap"] >= X.CLOSE_CLIP[fam]
    if c["mb"] >= 5:
        ok = ok and k["wraps"] >= 2 and k["repeats"] >= 1
        if fam != "terminal":
            ok = ok and k["terminated"] >= 1
    if fam == "terminal":
        ok = ok and k["terminated"] == (c["mb"] if c["p_term"] == 1.0 else 0)
    if fam == "target_tie":
        ok = ok and k["q_gap"] == 0.0 and (c["exp"]["next_actions"] == 0).all()
    else:
        ok = ok and k["q_gap"] >= X.CLOSE_Q[fam]
    if fam == "clip":
        ok = ok and k["clipped"] >= 3 and k["inside"] >= 3 and k["zero"] >= 1
    if c["tau_rule"] == "underflow":
        ok = ok and k["ratio"] >= 256.0
    return bool(ok)


def find_seed(i, start=0, tries=400):
    for seed in range(start, start + tries):
        if conditions_met(build(i, seed)):
            return seed
    raise RuntimeError("no seed for case %d" % i)


@functools.lru_cache(maxsize=None)
def make_case(i):
    """parameters, ring, indices and float64 expectations of case i (cached: treat as read-only)"""
    return build(i, SEEDS[i])
