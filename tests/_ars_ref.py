"""Augmented Random Search restated on the CPU — TEST INFRASTRUCTURE for libmirl_ars.so (include/mi_ars.h).

Every expression of the header is restated here in float64 with one rounding per operation (Python floats: IEEE double, nothing contracted), on the oracle's
`philox`, `reset_noise` and `cartpole_step` in its device-matched sin/cos mode ("fdlibm": bit for bit the device's env), as tests/_eval_ref.py uses them.  All sums
are sequential loops in the header's order.  Given the same `deltas` and `norm` the device must reproduce every output of this file BIT FOR BIT; the draw itself
(`normal64`: the header's float32 u1 / u2, then float64 logarithm, root and cosine) is the one float64 restatement that the device is held to within a bound.

VARIANTS are the ways an implementation can misread the header; each is a switch here, and tests/test_ars_ref_cpu.py shows that each changes M on the inputs the
GPU tests use:
  stats_before_episodes   the iteration's observations reach the normaliser BEFORE its episodes are played (they are folded, norm recomputed, the episodes played
                          under that norm) instead of serving the next iteration
  top_by_plus_only        the directions are ranked by r+ alone, not by max(r+, r-)
  sigma_all_returns       sigma_R over all 2 N returns, not over the 2 b selected ones
  sample_deviation        the sample deviation (2 b - 1 in the denominator) instead of the population's
  signs_share_start       both signs of a direction start from one state (env id base + 2 i for both)
  tie_to_higher_index     equal keys are ranked towards the higher index

The constants below are what the GPU tests run.
"""
import functools
import math

import numpy as np

import _timelimit_cases as T

f32 = np.float32
LIMIT = T.LIMIT
STREAM = 15
VARIANTS = ("stats_before_episodes", "top_by_plus_only", "sigma_all_returns", "sample_deviation", "signs_share_start", "tie_to_higher_index")
SEED = 1
TRAIN_BASE = (1 << 33) + 5        # training env ids: past 2^32, so that the high word of the id reaches the counter
EVAL_BASE = 1 << 40
SHAPES = (1, 3, 8, 33, 200)       # N: a partial wave, several waves, more than one 256-lane block (400 episodes)
CONTROLLER_MAX_N = 8              # a 500-step replay on the Python oracle is what costs time
EVAL_EPISODES = (1, 5, 37)
STEP_SIZE, NOISE = f32(0.02), f32(0.03)
CHAIN_ITERATIONS = (1, 2, 5)
CHAIN_SHAPES = ((3, 2), (8, 4))   # (N, b): b < N
MIXED_FACTORS = (1.0, 2.0, 4.0, 8.0)


def fresh_state():
    """-> dict M f32 [8], stats f64 [9], norm f64 [8], k"""
    return dict(M=np.zeros(8, f32), stats=np.zeros(9), norm=np.array([0.0] * 4 + [1.0] * 4), k=0)


@functools.lru_cache(maxsize=None)
def controller():
    """M with rows -K w, +K w (w = _timelimit_cases.RULE_W): s_1 - s_0 = 2 K (w . x), the balancing rule under norm = 0 / 1"""
    w = (T.CONTROLLER_K * T.RULE_W).astype(f32)
    M = np.concatenate([-w, w]).astype(f32)
    M.setflags(write=False)
    return M


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------------
def normal64(R, seed, n, k):
    """z f64 [n][8] of iteration k: the header's float32 u1 and u2, then everything in float64"""
    z = np.empty((n, 8))
    for i in range(n):
        for c in range(8):
            r = R.philox(int(seed), i, 8 * int(k) + c, STREAM)
            u1 = f32(f32(f32(r[0] >> np.uint32(8)) + f32(0.5)) * f32(1.0 / 16777216.0))
            u2 = f32(f32(r[1] >> np.uint32(8)) * f32(1.0 / 16777216.0))
            z[i, c] = math.sqrt(-2.0 * math.log(float(u1))) * math.cos(float(f32(6.28318530717958647692)) * float(u2))
    return z


def draw(R, seed, n, k):
    """the reference's own deltas f32 [n][8]: the float64 draw rounded once"""
    return normal64(R, seed, n, k).astype(f32)


# ---- episodes --------------------------------------------------------------------------------------------------------------------------------------
def run_episode(R, w, norm, seed, env, k):
    """one episode of the fp64 weights w [8] under norm [8] from mi_reset_noise(seed, env, k).  The caller holds the oracle in "fdlibm" mode.
    -> dict length, ret, truncated, actions u8 [length], partial f64 [9]"""
    w = [float(v) for v in w]
    mu, sc = [float(v) for v in norm[:4]], [float(v) for v in norm[4:]]
    y = R.reset_noise(int(seed), int(env), int(k))
    n, so, soo, acts = 0.0, [0.0] * 4, [0.0] * 4, []
    trunc = 0
    for _t in range(LIMIT):
        o = y.astype(f32).astype(np.float64).tolist()
        n = n + 1.0
        x = [0.0] * 4
        for j in range(4):
            so[j] = so[j] + o[j]
            soo[j] = soo[j] + o[j] * o[j]
            x[j] = (o[j] - mu[j]) * sc[j]
        s0 = ((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]) + w[3] * x[3]
        s1 = ((w[4] * x[0] + w[5] * x[1]) + w[6] * x[2]) + w[7] * x[3]
        a = 1 if s1 > s0 else 0
        y, term = R.cartpole_step(y, a)
        acts.append(a)
        trunc = int(not term and len(acts) >= LIMIT)
        if term or trunc:
            break
    return dict(length=len(acts), ret=float(len(acts)), truncated=trunc, actions=np.asarray(acts, np.uint8), partial=np.array([n] + so + soo))


def perturbed(M, delta, noise, sign):
    """w f64 [8] = (double)M + sign * ((double)noise * (double)delta): the product of two float32 is exact, the sum rounds once"""
    return [float(M[c]) + sign * (float(f32(noise)) * float(delta[c])) for c in range(8)]


def episodes(R, state, deltas, noise, seed=SEED, base=TRAIN_BASE, variant=None, norm=None):
    """the 2 N training episodes of the state's iteration under deltas f32 [N][8] -> list of run_episode dicts, e = 2 i + s"""
    assert variant is None or variant in VARIANTS
    norm = state["norm"] if norm is None else norm
    out = []
    with T._Mode(R):
        for i in range(len(deltas)):
            for s in (0, 1):
                env = base + (2 * i if variant == "signs_share_start" else 2 * i + s)
                out.append(run_episode(R, perturbed(state["M"], deltas[i], noise, 1.0 if s == 0 else -1.0), norm, seed, env, state["k"]))
    return out


def evaluate(R, state, n, seed=SEED, base=EVAL_BASE):
    """n greedy episodes of M under the current norm, keyed (seed, base + e, 0)"""
    with T._Mode(R):
        return [run_episode(R, [float(v) for v in state["M"]], state["norm"], seed, base + e, 0) for e in range(n)]


# ---- the update ------------------------------------------------------------------------------------------------------------------------------------
def select(returns, b, variant=None):
    """-> bool [N]: the b selected directions"""
    r = np.asarray(returns, f32).reshape(-1, 2)
    key = r[:, 0] if variant == "top_by_plus_only" else np.where(r[:, 0] > r[:, 1], r[:, 0], r[:, 1])
    n = len(key)
    sel = np.zeros(n, bool)
    for i in range(n):
        before = (np.arange(n) > i) if variant == "tie_to_higher_index" else (np.arange(n) < i)
        sel[i] = int(((key > key[i]) | ((key == key[i]) & before)).sum()) < b
    return sel


def fold(stats, partials):
    s = [float(v) for v in stats]
    for p in partials:
        for c in range(9):
            s[c] = s[c] + float(p[c])
    return np.array(s)


def normaliser(stats):
    out = [0.0] * 8
    n = float(stats[0])
    for j in range(4):
        with np.errstate(all="ignore"):
            m = float(np.float64(stats[1 + j]) / np.float64(n))
            v = float(np.float64(stats[5 + j]) / np.float64(n)) - m * m
        sd = math.sqrt(v if v > 0.0 else 0.0)
        out[j], out[4 + j] = m, (0.0 if sd < 1e-7 else 1.0 / sd)
    return np.array(out)


def update(state, returns, deltas, partials, b, step_size=STEP_SIZE, normalize=True, variant=None, fold_stats=True):
    """-> the state after the update (a new dict); `returns` f32 [2 N] whole numbers"""
    assert variant is None or variant in VARIANTS
    r = np.asarray(returns, f32).reshape(-1, 2)
    sel = select(returns, b, variant)
    pool = np.ones(len(r), bool) if variant == "sigma_all_returns" else sel
    cnt = 2 * int(pool.sum())
    ints = [int(v) for v in r[pool].reshape(-1)]
    S1, S2 = sum(ints), sum(v * v for v in ints)
    num = cnt * S2 - S1 * S1
    M = np.array(state["M"], f32)
    if num != 0:
        den = cnt * (cnt - 1) if variant == "sample_deviation" else cnt * cnt
        sigma = math.sqrt(float(num) / float(den))
        coef = float(f32(step_size)) / (float(b) * sigma)
        for c in range(8):
            g = 0.0
            for i in np.flatnonzero(sel):
                g = g + (float(r[i, 0]) - float(r[i, 1])) * float(deltas[i][c])
            M[c] = f32(float(M[c]) + coef * g)
    stats = fold(state["stats"], partials) if fold_stats else np.array(state["stats"], np.float64)
    norm = normaliser(stats) if normalize else np.array(state["norm"], np.float64)
    return dict(M=M, stats=stats, norm=norm, k=state["k"] + 1)


def iterate(R, state, N, b, deltas=None, step_size=STEP_SIZE, noise=NOISE, normalize=True, seed=SEED, base=TRAIN_BASE, variant=None):
    """one iteration -> (the new state, returns f32 [2 N], the episodes); deltas f32 [N][8] (None: the reference's own draw)"""
    d = draw(R, seed, N, state["k"]) if deltas is None else np.asarray(deltas, f32)
    if variant == "stats_before_episodes":
        first = episodes(R, state, d, noise, seed, base)
        stats = fold(state["stats"], [e["partial"] for e in first])
        early = dict(state, stats=stats, norm=normaliser(stats) if normalize else state["norm"])
        eps = episodes(R, early, d, noise, seed, base)
        ret = np.array([e["ret"] for e in eps], f32)
        return update(early, ret, d, [], b, step_size, normalize, None, fold_stats=False), ret, eps
    eps = episodes(R, state, d, noise, seed, base, variant)
    ret = np.array([e["ret"] for e in eps], f32)
    return update(state, ret, d, [e["partial"] for e in eps], b, step_size, normalize, variant), ret, eps


def chain(R, N, b, iterations, deltas=None, normalize=True, variant=None, seed=SEED, base=TRAIN_BASE, state=None):
    """`iterations` iterations from a fresh state (or `state`); deltas [iterations][N][8] or None -> (the final state, returns f32 [iterations][2 N])"""
    st = fresh_state() if state is None else state
    rows = []
    for t in range(iterations):
        st, ret, _ = iterate(R, st, N, b, None if deltas is None else deltas[t], normalize=normalize, seed=seed, base=base, variant=variant)
        rows.append(ret)
    return st, np.stack(rows)


# ---- the mixed case: a wave whose lanes run very different lengths ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case():
    """N = 8, SEED, M = the controller, the reference's own deltas of iteration 0; noise = the first of MIXED_FACTORS x max|M| under which at least one of the 16
    episodes is truncated at 500 and at least one ends before 100 steps -> dict noise, deltas, episodes (None when no factor qualifies: the CPU test fails)"""
    from oracle import cpu_ref as R
    st = dict(fresh_state(), M=np.array(controller()))
    d = draw(R, SEED, 8, 0)
    for fct in MIXED_FACTORS:
        noise = f32(fct * float(np.abs(controller()).max()))
        eps = episodes(R, st, d, noise)
        if any(e["truncated"] for e in eps) and any(e["length"] < 100 for e in eps):
            return dict(noise=noise, factor=fct, deltas=d, episodes=eps)
    return None


# ---- placed update cases -----------------------------------------------------------------------------------------------------------------------------
def _placed(name, returns, b, rng, M0=None, step_size=STEP_SIZE):
    returns = np.asarray(returns, f32)
    N = len(returns) // 2
    deltas = rng.standard_normal((N, 8)).astype(f32)
    partials = np.empty((2 * N, 9))
    for e in range(2 * N):   # what an episode of that length could have summed: observations around 0.3 with unit spread
        o = 0.3 + rng.standard_normal((max(int(returns[e]), 1), 4)).astype(f32).astype(np.float64)
        partials[e] = np.concatenate([[len(o)], np.cumsum(o, 0)[-1], np.cumsum(o * o, 0)[-1]])
    M0 = (rng.standard_normal(8).astype(f32) if M0 is None else np.asarray(M0, f32))
    stats0 = np.concatenate([[64.0], 64 * 0.3 + rng.standard_normal(4), 64 * 1.1 + rng.random(4)])
    return dict(name=name, N=N, b=b, returns=returns, deltas=deltas, partials=partials, step_size=f32(step_size),
                state=dict(M=M0, stats=stats0, norm=np.array([0.0] * 4 + [1.0] * 4), k=7))


@functools.lru_cache(maxsize=None)
def placed_cases():
    """name -> case.  Every case is named for the property tests/test_ars_ref_cpu.py shows it to have."""
    rng = np.random.default_rng(20181)
    out = []
    for b in range(1, 9):
        out.append(_placed("all_equal_b%d" % b, np.full(16, 500.0), b, rng))
    # keys 90, 70, 70, 70, 50, ...: with b = 3 the cut falls inside the three 70s, of which the two LOWER indices (2 and 5) are taken
    r = np.array([[20, 10], [90, 30], [70, 15], [30, 50], [12, 40], [25, 70], [70, 70], [9, 33]], f32)
    out.append(_placed("ties_straddle_cut", r.reshape(-1), 3, rng))
    rnd = lambda n: rng.integers(9, 501, 2 * n).astype(f32)   # noqa: E731
    out.append(_placed("b_1", rnd(8), 1, rng))
    out.append(_placed("b_N", rnd(8), 8, rng))
    out.append(_placed("N_1", np.array([37, 212], f32), 1, rng))
    # r+ == r- on the selected (the four best) directions, whose returns differ from one another: sigma_R > 0 and g = 0
    r = np.array([[400, 400], [11, 30], [350, 350], [45, 12], [500, 500], [19, 23], [275, 275], [60, 14]], f32)
    out.append(_placed("equal_pairs_selected", r.reshape(-1), 4, rng))
    out.append(_placed("N_4096", rnd(4096), 1000, rng))
    return {c["name"]: c for c in out}


def conditioning(stats):
    """per dimension (So2 / n) / var: the cancellation factor of the variance (the norm comparison's 1e-9 rests on <= 1e3)"""
    n = stats[0]
    m = stats[1:5] / n
    return (stats[5:9] / n) / (stats[5:9] / n - m * m)
