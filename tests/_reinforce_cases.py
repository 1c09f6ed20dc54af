"""Synthetic inputs of tests/test_gpu_reinforce_kernels.py — TEST INFRASTRUCTURE.  Every input those GPU tests hand to libmirl_pg.so is made here, from
numpy generators keyed by (MIRL_FUZZ_SEED, family, case), so that tests/test_reinforce_cases_cpu.py can validate the same inputs without a GPU and measure the
tolerances on them.

Tolerances (the convention of tests/test_gpu_reinforce.py): the device bound of a quantity is 8 x the error of the f32 numpy restatement (tests/_reinforce_ref.py)
against float64 on the same inputs.  The *_REST constants below are those errors, the largest over each case list at the default seed; the CPU test asserts that
the restatement stays at or below them, the GPU tests assert `<= 8 x` them."""
import os

import numpy as np

import _reinforce_ref as P
from oracle import cpu_ref as R

SEED = int(os.environ.get("MIRL_FUZZ_SEED", "1"))
CASES = int(os.environ.get("MIRL_FUZZ_CASES", "4"))
DEVICE_FACTOR = 8
f32 = np.float32

# measured by tests/test_reinforce_cases_cpu.py at MIRL_FUZZ_SEED = 1 (the figure observed stands beside each constant)
GRAD_REST = 6.8e-7           # of max |g|; observed 6.75e-7 (case 3: 1,088 envs, sigma 3), 3.6e-7 ... 4.6e-7 on the other three
RETURNS_RAW_REST = 4.3e-7    # relative to the value; observed 4.29e-7
RETURNS_NORM_REST = 6.2e-6   # absolute; observed 6.11e-6 at gamma 0.9, length 500 (R saturates at 10: the variance is a cancelling sum)
PROBS_REST = 1.7e-6          # absolute; observed 1.51e-6 with masks, 1.66e-6 in eval mode (logits of order 1e3 at sigma 3)
LOG_PROBS_REST = 1.2e-6      # of max(1, |l0|, |l1|); observed 1.11e-6
ADAM_REST = 4.7e-7           # per element, of max(|p|, lr); observed 4.68e-7

NEAR_ZERO = 1e-5           # tests/test_gpu_fuzz.py: a pre-activation this close to 0 may land on either side of the ReLU kink
KINK_SHARE = 0.01          # at most this share of a case's rows may be switched off for it
OBS_RANGE = np.array([4.8, 10.0, 0.42, 10.0])      # CartPole's position / angle limits and velocities far beyond what an episode reaches
SIGMAS = (0.05, 0.3, 1.0, 3.0)
POISON_ACTION, POISON_WORD = -7, 0xFFFFFFFF


def _rng(*key):
    return np.random.default_rng([SEED, *key])


def draw_params(rng, sigma):
    return rng.normal(0.0, sigma, P.NPARAMS).astype(f32)


def draw_obs(rng, n):
    return (rng.uniform(-1.0, 1.0, (n, 4)) * OBS_RANGE).astype(f32)


def draw_masks(rng, n):
    return rng.random((n, 128)) < 0.4


def gap_params(rng, sign):
    """parameters whose two logits differ by more than 100 on every row and under every mask: b2 = +-(75, -75), and W2's rows pull the same way (H >= 0)"""
    p = draw_params(rng, 1.0)
    w = np.abs(p[640:768]) + f32(0.01)
    p[640:768], p[768:896] = sign * w, -sign * w
    p[896], p[897] = sign * 75.0, -sign * 75.0
    return p


def one_bit_masks():
    """the special mask rows of section 4: all-zero, all-one, exactly one unit kept at the edges of the four 32-bit words"""
    rows = [np.zeros(128, bool), np.ones(128, bool)]
    for u in (0, 31, 32, 63, 64, 95, 96, 127):
        m = np.zeros(128, bool); m[u] = True
        rows.append(m)
    return np.array(rows)


# ---- 1. slab sum and grid stride ------------------------------------------------------------------------
PROBE_NS = (17, 33, 49, 65, 81, 1023, 1025, 1100)
PROBE_LEN = 37


def probe_envs(n):
    ks = [0, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, n - 1] + ([1023, 1024, n - 1] if n > 1024 else [])
    return sorted({k for k in ks if 0 <= k < n})


def probe_episode():
    """one synthetic 37-row episode: parameters, X (37, 4), A, M (37, 128), mask words (37, 4), b_returns (37,)"""
    rng = _rng(10)
    M = draw_masks(rng, PROBE_LEN)
    return dict(params=draw_params(rng, 0.3), X=draw_obs(rng, PROBE_LEN), A=rng.integers(0, 2, PROBE_LEN).astype(np.int32), M=M, W=P.mask_words(M),
                Rn=rng.normal(0.0, 1.0, PROBE_LEN).astype(f32))


# ---- 2. gradient at any shape ---------------------------------------------------------------------------
N_BUCKETS = ((1, 9), (9, 71), (70, 261), (1025, 1101))


def grad_case(case):
    """-> dict: the full storage of an N-env engine (rows behind each episode's end poisoned) and the valid rows, concatenated in env order, for the references.
    The env-count bucket rotates with the case number, so any four consecutive cases visit all four."""
    rng = _rng(20, case)
    lo, hi = N_BUCKETS[case % 4]
    n = int(rng.integers(lo, hi))
    sigma = float(rng.choice(SIGMAS))
    params = draw_params(rng, sigma)
    lengths = np.where(rng.random(n) < 0.15, 0, rng.integers(1, 25, n)).astype(np.int32)
    for e in rng.choice(n, size=min(n, int(rng.integers(0, 3))), replace=False):
        lengths[e] = rng.integers(493, 501)
    if lengths.sum() == 0:
        lengths[int(rng.integers(0, n))] = rng.integers(1, 25)
    rows = int(lengths.sum())
    X, A, M, Rn = draw_obs(rng, rows), rng.integers(0, 2, rows).astype(np.int32), draw_masks(rng, rows), rng.normal(0.0, 1.0, rows).astype(f32)
    if rows >= 2:
        z, o = rng.choice(rows, size=2, replace=False)
        M[z], M[o] = False, True
    Z = P.forward64(params, X, M)[3]
    kink = (np.where(M, np.abs(Z), np.inf) <= NEAR_ZERO).any(axis=1)          # a KEPT unit within NEAR_ZERO of the kink: the row contributes nothing on either side
    Rn[kink] = 0.0
    obs = np.full((n, P.ROWS, 4), np.nan, f32)
    act = np.full((n, P.ROWS), POISON_ACTION, np.int32)
    words = np.full((n, P.ROWS, 4), POISON_WORD, np.uint32)
    brn = np.full((n, P.ROWS), np.nan, f32)
    off = np.concatenate([[0], np.cumsum(lengths)])
    W = P.mask_words(M)
    for e in range(n):
        a, b, L = off[e], off[e + 1], lengths[e]
        obs[e, :L], act[e, :L], words[e, :L], brn[e, :L] = X[a:b], A[a:b], W[a:b], Rn[a:b]
    shape = "pg grad case %d: envs %d, rows %d, lengths 0 x %d / 1-24 x %d / 493-500 %s, sigma %g, kink rows %d" % (
        case, n, rows, int((lengths == 0).sum()), int(((lengths > 0) & (lengths < 25)).sum()), lengths[lengths > 24].tolist(), sigma, int(kink.sum()))
    return dict(n=n, sigma=sigma, params=params, lengths=lengths, X=X, A=A, M=M, Rn=Rn, kink=kink, obs=obs, act=act, words=words, brn=brn, shape=shape)


# ---- 3. returns ---------------------------------------------------------------------------------------------
RETURNS_NS = (1, 3, 5, 7)
RETURNS_LENGTHS = (2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 448, 449, 499, 500)
GAMMAS = (0.0, 0.5, 0.9, 0.99, 1.0)
RETURNS_EDGE_LENGTHS = (1, 0, -3, 501, 10 ** 6, 500, 2)      # one launch at N = 7: NaN row, empty, negative, two above the cap, the cap itself, the shortest


def returns_launches(n):
    """the length vectors of the launches at n envs: RETURNS_LENGTHS dealt n at a time, the last launch filled up from the front"""
    ls = list(RETURNS_LENGTHS)
    return [np.array([ls[(i + j) % len(ls)] for j in range(n)], np.int32) for i in range(0, len(ls), n)]


# ---- 4. forward and log-probs -------------------------------------------------------------------------------
FORWARD_NS = (1, 2, 3, 5, 257)


def forward_param_sets():
    """-> [(name, params)]: the four sigmas and the two saturated vectors (logit gap > 100 either way)"""
    rng = _rng(40)
    return [("sigma%g" % s, draw_params(rng, s)) for s in SIGMAS] + [("gap+", gap_params(rng, 1.0)), ("gap-", gap_params(rng, -1.0))]


def forward_launches(n):
    """-> [(X (n, 4), M (n, 128))]: as many launches as it takes for the ten special mask rows to pass through n rows; the first rows of X sit on the corners of the
    observation range, rows past the special ones carry drawn masks"""
    rng = _rng(41, n)
    special = one_bit_masks()
    out = []
    for off in range(0, len(special), n):
        X = draw_obs(rng, n)
        corners = (np.array([[1, 1, 1, 1], [-1, -1, -1, -1], [1, -1, 1, -1], [-1, 1, -1, 1]]) * OBS_RANGE).astype(f32)
        X[:min(n, 4)] = corners[(np.arange(min(n, 4)) + off) % 4]
        M = draw_masks(rng, n)
        k = min(n, len(special))
        M[:k] = special[(off + np.arange(k)) % len(special)]
        out.append((X, M))
    return out


def _balancing_actions(reset, rule):
    """forced actions from a rule on the oracle's f64 state, until done (as in tests/test_gpu_reinforce.py)"""
    env = R.VecCartPole(1, seed=1)
    env.reset(np.asarray(reset, np.float64).reshape(1, 4))
    acts = []
    while True:
        a = rule(env.state[0].copy())
        acts.append(a)
        d = env.step(np.array([a]), forced_reset=np.zeros((1, 4)))[2]
        if d[0]:
            return np.array(acts, np.int32)


def log_prob_rollouts():
    """-> two teacher-forced rollouts at N = 3: dict(name, params, resets (3, 4) f64, actions (3, 500), words (3, 500, 4), lengths, and per env the rows the policy
    sees: X from the oracle stepper, A, M).  Rows 0 / 1 of every env carry the all-zero / all-one mask."""
    rng = _rng(42)
    full = lambda s: int(s[2] + 0.5 * s[3] + 0.05 * s[0] + 0.1 * s[1] > 0)
    sets = [("sigma3", draw_params(rng, 3.0), [lambda s: 0, lambda s: 1, full]),
            ("gap+", gap_params(rng, 1.0), [lambda s: 1, lambda s: int(s[2] < 0), lambda s: int(s[2] + 0.5 * s[3] > 0)])]
    resets = np.array([[0.01 * (i - 1), 0.0, 0.02 * (i - 1), 0.0] for i in range(3)], np.float64)
    out = []
    R.set_sincos_mode("fdlibm")
    try:
        for name, params, rules in sets:
            acts = np.zeros((3, P.MAX_STEPS), np.int32); words = np.zeros((3, P.MAX_STEPS, 4), np.uint32); lens = np.zeros(3, np.int32); rows = []
            for i in range(3):
                a = _balancing_actions(resets[i], rules[i])
                L = len(a)
                M = draw_masks(rng, L); M[0] = False
                if L > 1:
                    M[1] = True
                after = P.replay_episode(resets[i], a)[0]
                X = np.concatenate([resets[i].astype(f32)[None], after[:-1]]).astype(f32)
                acts[i, :L], words[i, :L], lens[i] = a, P.mask_words(M), L
                acts[i, L:] = 1 - a[-1]
                rows.append((X, a.astype(np.int64), M))
            out.append(dict(name=name, params=params, resets=resets, actions=acts, words=words, lengths=lens, rows=rows))
    finally:
        R.set_sincos_mode("libm")
    return out


# ---- 5. RNG continuation -------------------------------------------------------------------------------------
RNG_N, RNG_SEED, RNG_BASE, RNG_EPISODES = 5, 2 ** 33 + 11, 2 ** 32 + 7, 3


def rng_params():
    return draw_params(_rng(50), 0.3)


def predicted_rng_lengths():
    """(RNG_N, RNG_EPISODES) episode lengths of the production streams under rng_params(), from the f32 restatement and the oracle stepper — a prediction used to
    choose the seed (the GPU test asserts the residue condition on the lengths the device produced)"""
    params = rng_params()
    out = np.zeros((RNG_N, RNG_EPISODES), np.int64)
    R.set_sincos_mode("fdlibm")
    try:
        for e in range(RNG_N):
            E, ctr = RNG_BASE + e, 0
            for j in range(RNG_EPISODES):
                s = R.reset_noise(RNG_SEED, E, j)
                for t in range(P.MAX_STEPS):
                    p0 = P.forward(params, s.astype(f32), P.keyed_masks(RNG_SEED, E, [ctr]))[0][0, 0]
                    a = int(P.action_uniforms(RNG_SEED, E, [ctr])[0] >= p0)
                    s, term = R.cartpole_step(s, a)
                    ctr += 1
                    if term:
                        break
                out[e, j] = t + 1
    finally:
        R.set_sincos_mode("libm")
    return out


def start_counters(lengths):
    """(N, episodes) lengths -> (N, episodes) step counter at which each episode starts"""
    lengths = np.asarray(lengths, np.int64)
    return np.cumsum(lengths, axis=1) - lengths


# ---- 6. Adam ------------------------------------------------------------------------------------------------
ADAM_NS = (1, 255, 256, 257, 898, 1000)
ADAM_STEPS = (1, 2, 1000, 10 ** 6)
ADAM_HPS = ((1e-2, 0.9, 0.999, 1e-8), (3e-4, 0.8, 0.99, 1e-5))
ADAM_PAD = 64              # elements behind n in every buffer, which must stay untouched


def adam_cases():
    """-> [dict(n, step, hp, p, g, m, v, shape)]: all of ADAM_NS x ADAM_STEPS x ADAM_HPS x (zero moments, drawn moments); buffers are n + ADAM_PAD long"""
    out = []
    for i, n in enumerate(ADAM_NS):
        for j, step in enumerate(ADAM_STEPS):
            for k, hp in enumerate(ADAM_HPS):
                for warm in (0, 1):
                    rng = _rng(60, i, j, k, warm)
                    tot = n + ADAM_PAD
                    g = (10.0 ** rng.uniform(-12.0, 3.0, tot) * rng.choice([-1.0, 1.0], tot)).astype(f32)
                    g[rng.random(tot) < 0.1] = 0.0
                    g[0] = 0.0 if (i + j) % 2 else g[0]
                    p = rng.normal(0.0, 0.5, tot).astype(f32)
                    if warm:
                        v = (10.0 ** rng.uniform(-12.0, 3.0, tot)).astype(f32) ** 2
                        v[rng.random(tot) < 0.1] = 0.0
                        m = (rng.normal(0.0, 1.0, tot) * np.sqrt(v)).astype(f32)
                    else:
                        m, v = np.zeros(tot, f32), np.zeros(tot, f32)
                    out.append(dict(n=n, step=step, hp=hp, p=p, g=g, m=m, v=v,
                                    shape="adam n %d, step %d, (lr, b1, b2, eps) %s, %s moments" % (n, step, hp, "drawn" if warm else "zero")))
    return out
