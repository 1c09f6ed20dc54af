"""Synthetic replay rings for the n-step kernels (deep_rl_amd/csrc/mi_nstep.hip, mi_nwalk.h) and their float64 expectations — TEST INFRASTRUCTURE
(tests/test_nstep_cases_cpu.py validates it, tests/test_gpu_nstep_cases.py uses it).  The reference is tests/_nstep_ref.py.

Every row kind is PLACED, not left to the seed.  A case has one head slot H (drawn from 1 .. slots - 3, so that slots - 1 is not the head).  Its rows are laid
into the ring one after the other; laying a row fixes the terminated flags its walk looks at (steps 1 .. m) and nothing else, and a row is only laid where the
flags already fixed agree with it.  With n = n_step, S = slots:
  full           starts behind the head (s_0 = H + 1 + j): n steps, no flag set
  term_1         terminated[s_1] = 1, s_1 != H
  term_mid       terminated[s_k] = 1 for one 1 < k < n, s_k != H                                          (n >= 3)
  term_n         terminated[s_n] = 1 and no flag before it, s_n != H                                      (n >= 2)
  head_cut       s_0 = H - k for one 1 <= k < n, no flag set: the head ends the walk at step k            (n >= 2)
  head_at_n      s_0 = H - n, no flag set: the walk ends ON the head by itself, the head has no effect
  on_head        s_0 = H (the stale row of a wrapped ring): step 1 is taken and terminated[s_1] = 0, so the walk runs on    (n >= 2)
  term_and_head  s_0 = H - k for one 1 <= k <= n and terminated[H] = 1: both stops on one slot
  wrap           s_0 = S - 2, terminated[S - 1] = 0: the walk crosses slot S - 1 -> 0 at its second step  (n >= 2)
  repeat         the index of another row, again
  lone_term / lone_head   a term_1 (term_mid where n >= 3) row and a head_cut row (n >= 2) laid FIRST into an env of their own that no later row may enter: the
                 cells beyond their stop are read by no other row and keep their NaN
and the rest of the batch are rows at random places whose flags are drawn with p_term as their walk meets cells that are still free.  The batch is then shuffled.
One-row case: the row sits in the last slot of the (1, 2) ring with n_step 1 and H = 0.

Poisoning.  Observations are finite at the sampled rows s_0 and at the bootstrap cells s_m and NaN everywhere else — the intermediate observations s_k, 0 < k < m,
included.  Rewards are distinct draws from N(0, r_std) at the cells some walk USES (steps 1 .. m of some row) and NaN everywhere else: beyond each stop, and at a
sampled row's own cell unless another row's walk uses it.  Actions are 0 / 1 at the sampled rows and 2 elsewhere.  Flags: what the walks fixed; a cell that is inside
some row's n-step window but beyond every stop holds `beyond` (1, and 0 in the case beyond_0_17: the loaded-but-unused flags take both values); every other cell 1.

Parameters, weights and the carried-over families are tests/_pdd_cases.py's: independent dueling draws for the two networks; weights None / "one" / "span" (one
exact 0, the maximum exactly 1); synced (target == online bit for bit); gamma 0 (the target is r_1 exactly) and 1; both heads x 30 with rewards N(0, 10); placed
exact-zero pre-activations (four units per layer).

Shapes (SPECS): batch 1 with n_step 1 on (n_envs, slots) = (1, 2); 12 rows with n_step 2 and 13 with n_step 3 on (5, 7); 17 with n_step 5 on (4, 12); 129 rows —
one more than there are workgroups — with n_step 3 on (4, 30); 300 rows, where workgroups walk three, with n_step 16 on (129, 40).  The families use 17 rows,
n_step 3, on (4, 12).

Conditions (asserted by the CPU test on the float64 reference; SEEDS holds the first seed from 0 that meets them, find_seed).  No row is excluded from any
comparison.  Every multi-row case holds at least one row of each kind its n_step allows, counted from the REFERENCE's walk, not from the placement; one terminated
and (n >= 2) one head-cut row whose cells beyond the stop all hold NaN rewards; at least one NaN reward inside some row's window.  No online pre-activation of a
sampled row lies within NEAR_ZERO of 0, placed units aside.  At EVERY bootstrap observation (terminated ones included: a* is written for them too) the online
net's |q0 - q1| is >= CLOSE_Q of the family.  |loss| >= LOSS_FLOOR.  Spanning weights: exactly one 0, at least one 1, the rest in [1e-3, 1].
"""
import functools

import numpy as np

import _dqn_cases as D
import _nstep_ref as X

f32 = np.float32
NEAR_ZERO, LOSS_FLOOR = D.NEAR_ZERO, D.LOSS_FLOOR
MAX_SLABS = 128
KINDS = ("full", "term_1", "term_mid", "term_n", "head_cut", "head_at_n", "on_head", "term_and_head", "wrap", "repeat")
MIN_N = dict(full=1, term_1=1, term_mid=3, term_n=2, head_cut=2, head_at_n=1, on_head=2, term_and_head=1, wrap=2, repeat=1)


def _spec(name, family, mb, n_step, ring, **opt):
    return dict(dict(name=name, family=family, mb=mb, n_step=n_step, ring=ring, gamma=0.99, p_term=0.25, head_scale=1.0, r_std=1.0, place=None, wkind=None, beyond=1), **opt)


SPECS = (
    _spec("plain_1_n1", "plain", 1, 1, (1, 2)),
    _spec("plain_12_n2", "plain", 12, 2, (5, 7)),
    _spec("plain_13_n3", "plain", 13, 3, (5, 7)),
    _spec("plain_17_n5", "plain", 17, 5, (4, 12)),
    _spec("plain_129_n3", "plain", MAX_SLABS + 1, 3, (4, 30)),
    _spec("plain_300_n16", "plain", 300, 16, (129, 40)),
    _spec("beyond_0_17", "plain", 17, 3, (4, 12), beyond=0),
    _spec("weights_one_17", "weights", 17, 3, (4, 12), wkind="one"),
    _spec("weights_span_17", "weights", 17, 3, (4, 12), wkind="span"),
    _spec("synced_17", "synced", 17, 3, (4, 12), place="synced"),
    _spec("gamma_0_17", "gamma", 17, 3, (4, 12), gamma=0.0),
    _spec("gamma_1_17", "gamma", 17, 3, (4, 12), gamma=1.0),
    _spec("scale_30_17", "scale", 17, 3, (4, 12), head_scale=30.0, r_std=10.0),
    _spec("kink_placed_17", "kink_placed", 17, 3, (4, 12), place="kink"),
)
NAMES = tuple(s["name"] for s in SPECS)
# found by find_seed(i): the first seed from 0 whose case meets the conditions of the module docstring
SEEDS = (0, 3, 1, 2, 0, 0, 5, 3, 0, 1, 0, 0, 0, 1)


class _Ring:
    """the flags while the rows are laid: -1 free, 0 / 1 fixed"""

    def __init__(self, N, S, head, n, rng, p_term):
        self.N, self.S, self.head, self.n, self.rng, self.p_term = N, S, head, n, rng, p_term
        self.flag = np.full((S, N), -1, np.int64)
        self.closed = set()   # envs no further row may enter

    def lay(self, s0, e, want, draw=False):
        """lay a row at (s0, e).  want: {step: flag} for the steps whose flags the kind fixes; every other step the walk reaches up to its stop is 0, or with `draw`
        keeps the flag it has and draws a free one -> the flat index, or None when a fixed flag disagrees or the env is closed"""
        if e in self.closed:
            return None
        S, n, head = self.S, self.n, self.head
        new, s = {}, s0 % S
        for k in range(1, n + 1):
            s = (s + 1) % S
            have = int(self.flag[s, e])
            f = want[k] if k in want else have if draw and have >= 0 else int(self.rng.random() < self.p_term) if draw else 0
            if have >= 0 and have != f:
                return None
            new[s] = f
            if f or s == head:
                break
        for s, f in new.items():
            self.flag[s, e] = f
        return (s0 % S) * self.N + e


def _lay_kinds(L, n, rng):
    """one row of every kind n allows, the two lone rows first -> {kind: flat index} (None where a kind found no place)"""
    N, S, H = L.N, L.S, L.head
    envs = lambda: rng.permutation(N).tolist()   # noqa: E731
    out = {}

    def first(name, tries):
        for s0, e, want, *draw in tries:
            i = L.lay(s0, e, want, *draw)
            if i is not None:
                out[name] = i
                return
        out[name] = None

    # the lone rows, each in an env of its own
    lone = envs()
    if N >= 3:
        k = 2 if n >= 3 else 1
        out["lone_term"] = L.lay(H + 1, lone[0], {k: 1}); L.closed.add(lone[0])
        if n >= 2:
            out["lone_head"] = L.lay(H - 1, lone[1], {}); L.closed.add(lone[1])
    free = lambda j: (H + 1 + j) % S   # noqa: E731  (slots behind the head)
    span = max(S - 1 - n, 1)
    starts = lambda: [int(x) for x in rng.permutation(span)]   # noqa: E731
    first("full", [(free(j), e, {}) for j in starts() for e in envs()])
    first("term_1", [(free(j), e, {1: 1}) for j in starts() for e in envs()])
    if n >= 3:
        first("term_mid", [(free(j), e, {int(k): 1}) for j in starts() for e in envs() for k in rng.permutation(np.arange(2, n))])
    if n >= 2:
        first("term_n", [(free(j), e, {n: 1}) for j in starts() for e in envs()])
        first("head_cut", [(H - int(k), e, {}) for k in rng.permutation(np.arange(1, n)) for e in envs()])
        first("on_head", [(H, e, {1: 0}, True) for e in envs()])
        first("wrap", [(S - 2, e, {1: 0}, True) for e in envs()])
    first("head_at_n", [(H - n, e, {}) for e in envs()])
    first("term_and_head", [(H - int(k), e, {int(k): 1}) for k in rng.permutation(np.arange(1, n + 1)) for e in envs()])
    return out


def build(i, seed):
    """case i from `seed`, with its float64 expectation under "exp" and the quantities the conditions are about under "cond"; None when a kind found no place"""
    s = SPECS[i]
    rng = np.random.default_rng([i, seed, 2018, 7])
    (N, S), mb, n = s["ring"], s["mb"], s["n_step"]
    cap = N * S
    if mb == 1:
        head, idx = 0, np.array([(S - 1) * N + int(rng.integers(0, N))], np.int64)
        L = _Ring(N, S, head, n, rng, s["p_term"])
        L.lay(S - 1, int(idx[0]) % N, {}, True)
    else:
        head = int(rng.integers(1, S - 2))
        L = _Ring(N, S, head, n, rng, s["p_term"])
        placed = _lay_kinds(L, n, rng)
        if any(v is None for v in placed.values()):
            return None
        idx = list(placed.values())
        while len(idx) < mb - 1:
            j = L.lay(int(rng.integers(0, S)), int(rng.integers(0, N)), {}, True)
            if j is not None:
                idx.append(j)
        idx.append(idx[int(rng.integers(0, len(idx)))])          # the repeat
        idx = np.array(idx, np.int64)
        rng.shuffle(idx)
    flags = L.flag
    ring0 = dict(actions=np.zeros((S, N), np.int64), rewards=np.zeros((S, N), f32), terminated=np.where(flags < 0, 1, flags).astype(np.uint8))
    at, _, _, m = X.walk(ring0, idx, n, head, s["gamma"])                                 # the flags the walks look at are all fixed: free cells do not matter
    used, window = np.zeros(cap, bool), np.zeros(cap, bool)
    for i0, mm in zip(idx.tolist(), m.tolist()):
        for k in range(1, n + 1):
            j = ((i0 // N + k) % S) * N + i0 % N
            window[j] = True
            used[j] = used[j] or k <= mm
    terminated = np.where(flags.reshape(-1) >= 0, flags.reshape(-1), np.where(window, s["beyond"], 1)).astype(np.uint8)
    rows, boot = np.unique(idx), np.unique(at)
    qparams, params = D.init_params(rng)
    qtarget, target = D.init_params(rng)                                                          # an independent draw
    nets = dict(params=qparams, dparams=params, target=qtarget, dtarget=target)
    units = D._place_params(dict(place=s["place"] if s["place"] == "kink" else None, head_scale=s["head_scale"]), rng, nets)
    if s["place"] == "synced":
        nets["dtarget"] = params.copy()
    obs = np.full((cap, 4), np.nan, f32)
    ref = np.union1d(rows, boot)
    obs[ref] = D._draw_obs(rng, len(ref))
    for _ in range(100):                                   # a sampled row's observation is redrawn until its online pre-activations are clear of 0
        bad = rows[D._zero_gap(*D._preacts64(params, obs[rows]), units) <= NEAR_ZERO]
        if not len(bad):
            break
        obs[bad] = D._draw_obs(rng, len(bad))
    rewards = np.full(cap, np.nan, f32)
    while True:
        rewards[used] = rng.normal(0, s["r_std"], int(used.sum())).astype(f32)
        if len(np.unique(rewards[used])) == used.sum():
            break
    actions = np.full(cap, 2, np.int64)
    actions[rows] = rng.integers(0, 2, len(rows))
    weights = None
    if s["wkind"] == "one":
        weights = np.ones(mb, f32)
    elif s["wkind"] == "span":
        weights = (10.0 ** rng.uniform(-3, 0, mb)).astype(f32)
        weights[0], weights[1] = 1.0, 0.0
        rng.shuffle(weights)
    c = dict(s, params=nets["dparams"], target=nets["dtarget"], idx=idx, head=head, weights=weights, observations=obs.reshape(S, N, 4), rewards=rewards.reshape(S, N),
             terminated=terminated.reshape(S, N), actions=actions.reshape(S, N), units=units, used=used, window=window)
    return finish(c)


def kinds_of(c, e=None):
    """the kinds of every row, read off the reference's walk -> {kind: bool [rows]} (and lone_term / lone_head: the cells beyond the stop all hold NaN rewards)"""
    e = c["exp"] if e is None else e
    (N, S), n, H, idx = c["ring"], c["n_step"], c["head"], c["idx"]
    m, at = e["horizon"], e["at"]
    term = c["terminated"].reshape(-1)[at] != 0
    on_h = at // N == H
    s0 = idx // N
    rew = c["rewards"].reshape(-1)
    crossed = np.array([any((s + k) % S == 0 for k in range(2, mm + 1)) for s, mm in zip(s0.tolist(), m.tolist())])
    beyond_nan = np.array([mm < n and all(np.isnan(rew[((s + k) % S) * N + i0 % N]) for k in range(mm + 1, n + 1)) for i0, s, mm in zip(idx.tolist(), s0.tolist(), m.tolist())])
    _, inv, cnt = np.unique(idx, return_inverse=True, return_counts=True)
    return dict(full=(m == n) & ~term & ~on_h & (s0 != H), term_1=(m == 1) & term & ~on_h, term_mid=(m > 1) & (m < n) & term & ~on_h, term_n=(m == n) & term & ~on_h & (n > 1),
                head_cut=(m < n) & on_h & ~term, head_at_n=(m == n) & on_h & ~term & (s0 != H), on_head=(s0 == H) & (m >= 2), term_and_head=on_h & term,
                wrap=crossed, repeat=cnt[inv] > 1, lone_term=beyond_nan & term, lone_head=beyond_nan & on_h & ~term)


def finish(c):
    e = c["exp"] = X.evaluate(c)
    kinds = kinds_of(c)
    rew = c["rewards"].reshape(-1)
    c["cond"] = dict(rows=int(len(c["idx"])), kinds={k: int(v.sum()) for k, v in kinds.items()}, zero_gap=float(D._zero_gap(e["z1"], e["z2"], c["units"]).min()),
                     loss=e["loss"], q_gap=float(np.abs(e["q_next"][:, 0] - e["q_next"][:, 1]).min()), nan_in_window=int(np.isnan(rew[c["window"]]).sum()),
                     live=int((e["live"] > 0).sum()), live_a1=int(e["next_actions"][e["live"] > 0].sum()))
    return c


def conditions_met(c):
    if c is None:
        return False
    k, n = c["cond"], c["n_step"]
    ok = k["rows"] == c["mb"] and k["zero_gap"] > NEAR_ZERO and abs(k["loss"]) >= LOSS_FLOOR and k["q_gap"] >= X.CLOSE_Q[c["family"]]
    if c["mb"] > 1:
        ok = ok and all(k["kinds"][kind] >= 1 for kind in KINDS if n >= MIN_N[kind]) and k["kinds"]["lone_term"] >= 1 and k["nan_in_window"] >= 1
        ok = ok and (n < 2 or k["kinds"]["lone_head"] >= 1) and 1 <= k["live_a1"] < k["live"]
    return bool(ok)


def find_seed(i, start=0, tries=200):
    for seed in range(start, start + tries):
        if conditions_met(build(i, seed)):
            return seed
    raise RuntimeError("no seed for case %d" % i)


@functools.lru_cache(maxsize=None)
def make_case(i):
    """parameters, ring, head, indices, weights and float64 expectations of case i (cached: treat as read-only)"""
    return build(i, SEEDS[i])
