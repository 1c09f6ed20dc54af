"""Synthetic replay rings for the prioritized dueling Double DQN kernels (deep_rl_amd/csrc/mi_pdd.hip) and their float64 expectations — TEST INFRASTRUCTURE
(tests/test_pdd_cases_cpu.py validates it, tests/test_gpu_pdd_cases.py uses it).  The reference is tests/_pdd_ref.py.

The storage is built the way tests/_ddqn_cases.py builds its rings, with tests/_dqn_cases.py's helpers: rings (n_envs, slots) = (1, 2) for one row, (3, 7) for 5 to 9
rows, (2, 30) for 17 and for 129 rows (every row of that ring is drawn about twice), (129, 40) for 300; the batch is drawn WITH repetition; with >= 5 rows two
entries are moved into the last slot (their successor wraps to slot 0) and one entry repeats another; the one-row case sits in the last slot of the two-slot ring.
Observations lie inside CartPole's range.  Rewards of the successors are distinct draws from N(0, r_std).  Every observation and reward that the batch does not
reference, as a row or as a successor, holds NaN; unreferenced actions hold 2, unreferenced terminated flags 1.  The OWN reward of a sampled row that is not some
other sampled row's successor holds NaN too and its own flag is 1.  The observation of a sampled row is redrawn until no online pre-activation of that row lies
within NEAR_ZERO of 0.

Parameters.  The dueling vectors of _dqn_cases.init_params (nn.Linear's default init plus N(0, 0.05) on every element, 11,019 floats).  The TARGET network is an
INDEPENDENT draw of the same kind, not online + noise.

Weights.  None (the launch gets NULL: uniform replay), "one" (every weight 1.0f: must give NULL's bits), "span" (10^U(-3, 0) as f32, one row exactly 1 — the
batch maximum, as per.py:149 leaves it — and one row exactly 0).

The families (SPECS).  The gradient launch has MI_PDD_MAX_SLABS = 128 workgroups; workgroup g walks rows g, g + 128, ...
  plain          weights None: batch 1 (the row in the last slot of the (1, 2) ring), 5 on (3, 7), 129 on (2, 30) (workgroup 0 walks two rows: a one-row tail), 300 on
                 (129, 40) (workgroups 0 .. 43 walk three)
  weights        batch 17 with every weight 1; batch 17 and 300 with the spanning weights
  synced         batch 17: target == online bit for bit
  online_tie     batch 9: both online advantage rows and biases are equal, so the online q ties bit for bit at every successor and a* must be 0 on every row; of the
                 independent target draw and the same draw with its advantage rows swapped, the one with Qt[1] > Qt[0] on at least half the live rows is taken
  terminal       batch 9: every successor terminated (also evaluated with a second, unrelated target vector: nothing may move by a bit); batch 17: none
  gamma          batch 17: gamma 0.0 and 1.0
  scale          batch 17: both nets' heads scaled by 30, rewards N(0, 10)
  adv_tie        batch 17: Wa[0] == Wa[1], ba[0] == ba[1] in BOTH networks: the advantage term vanishes, Q is the value head alone (and every a* is 0)
  kink_placed    batch 8: four first-layer and four second-layer units of the online net with zero weights and bias (_dqn_cases' placement): exact zeros in the
                 float64 gradient must be exact zeros on the device

Conditions (asserted by the CPU test on the float64 reference; SEEDS holds the first seed from 0 that meets them, find_seed).  No row is excluded from any
comparison: the share left out is zero.  With >= 5 rows: >= 2 wrapping rows, >= 1 repeated index, >= 1 terminated successor outside the terminal family, and —
outside synced, adv_tie and the all-terminated case — >= 1 LIVE row on which argmax Q_online(obs[nx]) != argmax Q_target(obs[nx]); a* takes both values on the live
rows, the two tie families and the all-terminated case aside.  No online pre-activation of a sampled row lies within NEAR_ZERO of 0, placed units aside.  On EVERY
successor (terminated ones included: a* is written out for them too) the online net's |q0 - q1| is >= CLOSE_Q of the family, the two tie families aside, where it is
exactly 0.  |loss| >= LOSS_FLOOR, so a relative loss figure means something.  Spanning weights: exactly one 0, at least one 1, the rest in [1e-3, 1].
"""
import functools

import numpy as np

import _dqn_cases as D
import _pdd_ref as X

f32 = np.float32
NEAR_ZERO, LOSS_FLOOR = D.NEAR_ZERO, D.LOSS_FLOOR
MAX_SLABS = 128
TIES = ("online_tie", "adv_tie")


def _spec(name, family, mb, **opt):
    ring = D.RINGS[0] if mb == 1 else D.RINGS[1] if mb <= 9 else D.RINGS[2] if mb <= MAX_SLABS + 1 else D.RINGS[3]
    return dict(dict(name=name, family=family, mb=mb, ring=ring, gamma=0.99, p_term=1.0 / 3.0, head_scale=1.0, r_std=1.0, place=None, wkind=None), **opt)


SPECS = (
    _spec("plain_1", "plain", 1),
    _spec("plain_5", "plain", 5),
    _spec("plain_129", "plain", MAX_SLABS + 1),
    _spec("plain_300", "plain", 300),
    _spec("weights_one_17", "weights", 17, wkind="one"),
    _spec("weights_span_17", "weights", 17, wkind="span"),
    _spec("weights_span_300", "weights", 300, wkind="span"),
    _spec("synced_17", "synced", 17, place="synced"),
    _spec("online_tie_9", "online_tie", 9, place="online_tie"),
    _spec("terminal_all_9", "terminal", 9, p_term=1.0),
    _spec("terminal_none_17", "terminal", 17, p_term=0.0),
    _spec("gamma_0_17", "gamma", 17, gamma=0.0),
    _spec("gamma_1_17", "gamma", 17, gamma=1.0),
    _spec("scale_30_17", "scale", 17, head_scale=30.0, r_std=10.0),
    _spec("adv_tie_17", "adv_tie", 17, place="adv_tie"),
    _spec("kink_placed_8", "kink_placed", 8, place="kink"),
)
NAMES = tuple(s["name"] for s in SPECS)
UNIFORM = tuple(i for i, s in enumerate(SPECS) if s["wkind"] is None)
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 3)


def _tie_adv(v):
    a, b = D.DUEL["Wa"]
    v[a + D.H2:b] = v[a:a + D.H2]
    v[D.DUEL["ba"][0] + 1] = v[D.DUEL["ba"][0]]


def _swap_adv(v):
    w = v.copy()
    a, b = D.DUEL["Wa"]
    w[a:a + D.H2], w[a + D.H2:b] = v[a + D.H2:b], v[a:a + D.H2]
    w[D.DUEL["ba"][0]], w[D.DUEL["ba"][0] + 1] = v[D.DUEL["ba"][0] + 1], v[D.DUEL["ba"][0]]
    return w


def build(i, seed):
    """case i from `seed`, with its float64 expectation under "exp" and the quantities the conditions are about under "cond" """
    s = SPECS[i]
    rng = np.random.default_rng([i, seed, 2016, 3])
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
    qparams, params = D.init_params(rng)
    qtarget, target = D.init_params(rng)                                                          # an independent draw
    nets = dict(params=qparams, dparams=params, target=qtarget, dtarget=target)                   # (_place_params' names: the dueling vectors are "dparams" / "dtarget")
    units = D._place_params(dict(place=s["place"] if s["place"] == "kink" else None, head_scale=s["head_scale"]), rng, nets)
    if s["place"] == "synced":
        nets["dtarget"] = params.copy()
    if s["place"] in TIES:
        _tie_adv(params)
    if s["place"] == "adv_tie":
        _tie_adv(nets["dtarget"])
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
    weights = None
    if s["wkind"] == "one":
        weights = np.ones(mb, f32)
    elif s["wkind"] == "span":
        weights = (10.0 ** rng.uniform(-3, 0, mb)).astype(f32)
        weights[0], weights[1] = 1.0, 0.0
        rng.shuffle(weights)
    if s["place"] == "online_tie":                         # the target head that prefers action 1 on at least half the live rows
        qt = X.forward(nets["dtarget"], obs[nx])
        live = terminated[nx] == 0
        if (qt[live, 1] > qt[live, 0]).sum() * 2 < live.sum():
            nets["dtarget"] = _swap_adv(nets["dtarget"])
    c = dict(s, params=nets["dparams"], target=nets["dtarget"], idx=idx, weights=weights, observations=obs.reshape(S, N, 4), rewards=rewards.reshape(S, N),
             terminated=terminated.reshape(S, N), actions=actions.reshape(S, N), units=units)
    return finish(c)


def finish(c):
    N, S = c["ring"]
    idx, mb = c["idx"], c["mb"]
    e = c["exp"] = X.evaluate(c)
    live = e["live"] > 0
    differ = e["q_next"].argmax(axis=1) != e["q_target"].argmax(axis=1)
    c["cond"] = dict(rows=int(len(idx)), wraps=int((idx // N == S - 1).sum()), repeats=int(mb - len(np.unique(idx))),
                     poisoned=float(np.isnan(c["rewards"].reshape(-1)[idx]).mean()), zero_gap=float(D._zero_gap(e["z1"], e["z2"], c["units"]).min()),
                     loss=e["loss"], terminated=int((~live).sum()), live_differ=int((differ & live).sum()),
                     q_gap=float(np.abs(e["q_next"][:, 0] - e["q_next"][:, 1]).min()), q_gap_max=float(np.abs(e["q_next"][:, 0] - e["q_next"][:, 1]).max()),
                     target_prefers_1=int((e["q_target"][live, 1] > e["q_target"][live, 0]).sum()), live=int(live.sum()), live_a1=int(e["next_actions"][live].sum()))
    return c


def conditions_met(c):
    k, fam, name = c["cond"], c["family"], c["name"]
    ok = k["rows"] == c["mb"] and k["zero_gap"] > NEAR_ZERO and abs(k["loss"]) >= LOSS_FLOOR
    if c["mb"] >= 5:
        ok = ok and k["wraps"] >= 2 and k["repeats"] >= 1
        if fam != "terminal":
            ok = ok and k["terminated"] >= 1
        if fam not in ("synced", "adv_tie") and name != "terminal_all_9":
            ok = ok and k["live_differ"] >= 1
        if fam not in TIES and name != "terminal_all_9":
            ok = ok and 1 <= k["live_a1"] < k["live"]
    if fam == "terminal":
        ok = ok and k["terminated"] == (c["mb"] if c["p_term"] == 1.0 else 0)
    if fam in TIES:
        ok = ok and k["q_gap_max"] == 0.0 and (c["exp"]["next_actions"] == 0).all() and k["live"] >= 1
        if fam == "online_tie":
            ok = ok and 2 * k["target_prefers_1"] >= k["live"]
    else:
        ok = ok and k["q_gap"] >= X.CLOSE_Q[fam]
    return bool(ok)


def find_seed(i, start=0, tries=200):
    for seed in range(start, start + tries):
        if conditions_met(build(i, seed)):
            return seed
    raise RuntimeError("no seed for case %d" % i)


@functools.lru_cache(maxsize=None)
def make_case(i):
    """parameters, ring, indices, weights and float64 expectations of case i (cached: treat as read-only)"""
    return build(i, SEEDS[i])
