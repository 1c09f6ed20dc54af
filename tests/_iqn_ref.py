"""numpy restatement of the IQN path (include/mi_iqn.h "Numerics contract") — TEST INFRASTRUCTURE.

Two modes.  ``f32``: the header's chains and summation orders for the forward, the targets and the loss (numpy has no fmaf: ``fma32`` forms the product and the sum
in f64 and rounds once more to f32, so comparisons with the device are to tolerance), the gradient in numpy's own f32 order.  ``float64``: everything in double on
the same f32 inputs.  Also the fixtures' loaders, the Philox draws of the RNG contract and the synthetic cases of the GPU tests.

Device bounds.  tests/test_iqn_ref_pinned_cpu.py measures the f32 restatement against the fixtures (the reference's own f32 evaluation by torch) and against
float64 at every checkpoint; each device bound is 8 x the measured figure: the project's margin for "another f32 evaluation in another summation order plus a
~1-ulp cosf".
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPARAMS, EMB, NCOS, HID = 44898, 64, 64, 512
OFF = dict(FW1=0, FB1=128, FW2=160, FB2=2208, FW3=2272, FB3=6368, CW=6432, CB=10528, QW1=10592, QB1=43360, QW2=43872, QB2=44896)
SHAPES = dict(FW1=(32, 4), FB1=(32,), FW2=(64, 32), FB2=(64,), FW3=(64, 64), FB3=(64,), CW=(64, 64), CB=(64,), QW1=(512, 64), QB1=(512,), QW2=(2, 512), QB2=(2,))
ORDER = ("FW1", "FB1", "FW2", "FB2", "FW3", "FB3", "CW", "CB", "QW1", "QB1", "QW2", "QB2")
f32 = np.float32
I_PI = (f32(np.pi) * np.arange(1, 65).astype(f32)).astype(f32)   # equal to the fixture's captured table and the header's constants (asserted on the CPU)
S_C = [np.array([u for u in range(HID) if (u >> 3) & 3 == c]) for c in range(4)]   # the header's split of the hidden units

# measured by tests/test_iqn_ref_pinned_cpu.py (f32 restatement against the reference's torch evaluation and against float64, maximum over the checkpoints and
# the acting forwards) -> device bound = 8 x
MEASURED_QUANT_ABS = 1.0e-4          # current / target quantiles, absolute (9.2e-5; max |quantile| is 215 at the checkpoints)
MEASURED_QUANT_REL = 5.0e-7          # the same, relative to max |quantile| (4.3e-7)
MEASURED_Q_ABS = 1.0e-5              # action values (mean over 32 taus), absolute, against float64 (8.8e-6)
MEASURED_LOSS_REL = 2.0e-7           # loss, relative (1.97e-7)
MEASURED_GRAD_REL = 2.6e-6           # gradient, relative to max |g| (2.5e-6)
MEASURED_GRAD_TENSOR_REL = 6.5e-6    # gradient of each of the twelve tensors, relative to that tensor's own max |g| (6.1e-6)
MEASURED_PARAM_ABS = 3.0e-8          # parameters at the checkpoints of the 21 chained updates, restatement's own gradients and Adam (2.98e-8)
MEASURED_PREACT_ABS = 4.5e-6         # max |pre-activation f32 - float64| over all ReLU inputs (3.4e-6 at the checkpoints, 1.6e-6 on the synthetic cases)
BOUND_QUANT_ABS, BOUND_QUANT_REL, BOUND_Q_ABS = 8 * MEASURED_QUANT_ABS, 8 * MEASURED_QUANT_REL, 8 * MEASURED_Q_ABS
BOUND_LOSS_REL, BOUND_GRAD_REL, BOUND_PARAM_ABS = 8 * MEASURED_LOSS_REL, 8 * MEASURED_GRAD_REL, 8 * MEASURED_PARAM_ABS
BOUND_GRAD_TENSOR_REL = 8 * MEASURED_GRAD_TENSOR_REL
NEAR_ZERO = 8 * MEASURED_PREACT_ABS  # no ReLU pre-activation of a synthetic case's float64 evaluation lies within this of 0
NEAR_KAPPA_REL = 8 * MEASURED_QUANT_REL   # no |td error| of a case lies within NEAR_KAPPA_REL * max(1, max |quantile|) of kappa (value and slope jump there)
# The fixtures are captured at a batch of 8 rows (trace["hparams"][5]): at the reference's 32 the 131,072 td errors of an update lie so densely around kappa (CartPole's
# reward) that no update of two whole runs kept NEAR_KAPPA_REL; at 8 rows the four checkpoints do (asserted by the capture tool and on the CPU).  For the other 17
# updates of the window the fixture names the td errors inside the margin and what they can move the loss by (flip_allowance), which the chained test adds to its bound.
CLOSE_Q = 2 * BOUND_Q_ABS            # rows whose two action values are closer than this are left out of action comparisons (at most one row per case)


def results_dir():
    """Where the GPU tests leave their observed figures: $MIRL_RESULTS_DIR, else results_out/ in the repository root (git-ignored)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.environ.get("MIRL_RESULTS_DIR") or os.path.join(root, "results_out")
    os.makedirs(d, exist_ok=True)
    return d


def load(name):
    z = np.load(os.path.join(GOLD, name))
    return {k: z[k] for k in z.files}


def load_trace():
    return load("iqn_ref_trace.npz")


def load_start():
    return load("iqn_ref_start.npz")


def load_ckpt(k):
    return load("iqn_ref_ckpt%d.npz" % k)


def ring(t):
    """the compact ring of the trace fixture as [slots][1] arrays: observations (S, 1, 4) f32, actions (S, 1) i64, rewards (S, 1) f32, terminated (S, 1) u8"""
    return (t["ring_observations"].astype(f32)[:, None, :], t["ring_actions"].astype(np.int64)[:, None], t["ring_rewards"].astype(f32)[:, None],
            t["ring_terminated"].astype(np.uint8)[:, None])


# ---- RNG contract --------------------------------------------------------------------------------------
def _philox(seed, env, idx, stream):
    from _reinforce_ref import philox
    return philox(seed, env, idx, stream)


def tau_draws(seed, key, rows, n, stream, base=16):
    """taus [rows][n] of streams 9 - 12: word w of philox(seed, key, row * base + m, stream) is tau 4 m + w"""
    rows = np.asarray(rows, np.uint64).reshape(-1)
    m = np.arange(n // 4, dtype=np.uint64)
    r = _philox(seed, np.uint64(key), rows[:, None] * np.uint64(base) + m[None, :], stream)   # (rows, n / 4, 4)
    return ((r >> np.uint32(8)).astype(f32) / f32(16777216.0)).reshape(len(rows), n)


def index_draws(seed, update, batch, upper):
    r = _philox(seed, np.uint64(update), np.arange(batch, dtype=np.uint64), 4)
    return ((r[:, 0].astype(np.uint64) | (r[:, 1].astype(np.uint64) << np.uint64(32))) % np.uint64(upper)).astype(np.int64)


# ---- arithmetic -------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def unpack(p, dtype=f32):
    p = np.asarray(p, f32).astype(dtype)
    return {k: p[OFF[k]:OFF[k] + int(np.prod(SHAPES[k]))].reshape(SHAPES[k]) for k in ORDER}


def pack_grads(g):
    return np.concatenate([np.asarray(g[k]).ravel() for k in ORDER])


def _chain(W, V, start):
    """acc = start; for ascending k: acc = fma32(W[..., k], V[..., k], acc) — W (out, K), V (rows, K) -> (rows, out)"""
    acc = np.broadcast_to(start, (V.shape[0], W.shape[0])).astype(f32)
    for k in range(W.shape[1]):
        acc = fma32(W[None, :, k], V[:, k, None], acc)
    return acc


def cosines(taus, dtype=f32):
    """c_k = cos(tau * i_pi[k]): the f32 product, then the cosine (f32: the correctly rounded value; the device library's cosf is within 1 ulp of it)"""
    arg = (np.asarray(taus, f32)[..., None] * I_PI).astype(f32)
    return np.cos(arg.astype(np.float64)).astype(dtype)


def forward(params, X, taus, dtype=f32):
    """obs X [n][4], taus [n][K] -> dict(quantiles [n][K][2], q [n][2], and the intermediates) in f32 (the header's chains) or float64"""
    w = unpack(params, dtype)
    X = np.asarray(X, f32).astype(dtype).reshape(-1, 4)
    taus = np.asarray(taus, f32).reshape(X.shape[0], -1)
    n, K = taus.shape
    cs = cosines(taus, dtype).reshape(n * K, NCOS)
    if dtype is f32:
        z1 = _chain(w["FW1"], X, w["FB1"]); h1 = np.maximum(z1, f32(0))
        z2 = _chain(w["FW2"], h1, w["FB2"]); h2 = np.maximum(z2, f32(0))
        z3 = _chain(w["FW3"], h2, w["FB3"]); emb = np.maximum(z3, f32(0))
        zc = _chain(w["CW"], cs, w["CB"]); te = np.maximum(zc, f32(0)).reshape(n, K, EMB)
        prod = (emb[:, None, :] * te).astype(f32).reshape(n * K, EMB)
        z = _chain(w["QW1"], prod, w["QB1"]); h = np.maximum(z, f32(0))
        quant = np.zeros((n * K, 2), f32)
        for a in range(2):
            parts = []
            for c in range(4):
                acc = np.full(n * K, w["QB2"][a] if c == 0 else f32(0), f32)
                for u in S_C[c]:
                    acc = fma32(w["QW2"][a, u], h[:, u], acc)
                parts.append(acc)
            quant[:, a] = (((parts[0] + parts[1]).astype(f32) + parts[2]).astype(f32) + parts[3]).astype(f32)
        quant = quant.reshape(n, K, 2)
        s = np.zeros((n, 2), f32)
        for i in range(K):
            s = (s + quant[:, i]).astype(f32)
        q = (s / f32(K)).astype(f32)
    else:
        z1 = X @ w["FW1"].T + w["FB1"]; h1 = np.maximum(z1, 0)
        z2 = h1 @ w["FW2"].T + w["FB2"]; h2 = np.maximum(z2, 0)
        z3 = h2 @ w["FW3"].T + w["FB3"]; emb = np.maximum(z3, 0)
        zc = cs @ w["CW"].T + w["CB"]; te = np.maximum(zc, 0).reshape(n, K, EMB)
        prod = (emb[:, None, :] * te).reshape(n * K, EMB)
        z = prod @ w["QW1"].T + w["QB1"]; h = np.maximum(z, 0)
        quant = (h @ w["QW2"].T + w["QB2"]).reshape(n, K, 2)
        q = quant.mean(axis=1)
    return dict(quantiles=quant, q=q, X=X, z1=z1, h1=h1, z2=z2, h2=h2, z3=z3, emb=emb, cs=cs.reshape(n, K, NCOS), zc=zc.reshape(n, K, EMB), te=te,
                prod=prod.reshape(n, K, EMB), z=z.reshape(n, K, HID), h=h.reshape(n, K, HID))


def target(target_params, X_next, rewards, terminated, next_taus, tau_dashes, gamma=0.99, dtype=f32):
    """-> (next_actions, target_action_quantiles [B][64], q [B][2]) of iqn.py:252-278"""
    q = forward(target_params, X_next, next_taus, dtype)["q"]
    a = (q[:, 1] > q[:, 0]).astype(np.int64)
    nq = forward(target_params, X_next, tau_dashes, dtype)["quantiles"][np.arange(len(a)), :, a]
    lg = np.where(np.asarray(terminated).astype(bool), 0, f32(gamma)).astype(dtype)[:, None]
    r = np.asarray(rewards, f32).astype(dtype)[:, None]
    return a, (r + (lg * nq).astype(dtype)).astype(dtype), q


def quantile_huber(current, tgt, taus, dtype=f32):
    """loss and dcurrent of iqn.py:281-289 (kappa = 1) from current [B][64], target [B][64], taus [B][64]; f32: the header's order (rows added ascending)"""
    inp = f32 if dtype is f32 else np.float64   # float64: current and target as the float64 forward formed them, not rounded to f32 on the way in (taus are f32 inputs)
    cur = np.asarray(current, inp).astype(dtype); tg = np.asarray(tgt, inp).astype(dtype); tau = np.asarray(taus, f32).astype(dtype)
    B = cur.shape[0]
    d = (tg[:, None, :] - cur[:, :, None]).astype(dtype)   # [b][i][j]
    ad = np.abs(d)
    quad = ad <= 1
    huber = np.where(quad, (d * d).astype(dtype), (ad - dtype(0.5)).astype(dtype))
    g = np.where(quad, (dtype(2) * d).astype(dtype), np.where(d > 0, dtype(1), dtype(-1)))
    w = np.abs((tau[:, :, None] - (d < 0).astype(dtype)).astype(dtype))
    lt, gt = (w * huber).astype(dtype), (w * g).astype(dtype)
    if dtype is f32:
        inv = f32(1.0) / f32(B * 64)

        def rows(v):   # [b][i][64] -> ((T0 + T1) + T2) + T3, T_c the ascending sum of 16
            parts = []
            for c in range(4):
                acc = np.zeros(v.shape[:2], f32)
                for j in range(16 * c, 16 * c + 16):
                    acc = (acc + v[:, :, j]).astype(f32)
                parts.append(acc)
            return (((parts[0] + parts[1]).astype(f32) + parts[2]).astype(f32) + parts[3]).astype(f32)

        L, G = rows(lt), rows(gt)
        rowloss = np.zeros(B, f32)
        for i in range(64):
            rowloss = (rowloss + L[:, i]).astype(f32)
        total = f32(0)
        for b in range(B):
            total = f32(total + rowloss[b])
        return f32(total * inv), (-(G * inv)).astype(f32), rowloss
    inv = 1.0 / (B * 64)
    rowloss = lt.sum(axis=(1, 2))
    return rowloss.sum() * inv, -(gt.sum(axis=2) * inv), rowloss


def loss_grad(params, X, A, tgt, taus, dtype=f32):
    """loss (iqn.py:289) and its gradient w.r.t. the flat parameters -> (loss, grad [44,898], current [B][64], forward dict).  f32: forward and loss in the header's
    order, the backward in numpy's own f32 order."""
    fw = forward(params, X, taus, dtype)
    w = unpack(params, dtype)
    A = np.asarray(A, np.int64).reshape(-1)
    B = len(A)
    rows = np.arange(B)
    cur = fw["quantiles"][rows, :, A]
    loss, dcur, _ = quantile_huber(cur, tgt, taus, dtype)
    dq = np.zeros((B, 64, 2), dtype); dq[rows, :, A] = dcur
    dq = dq.reshape(B * 64, 2)
    h, z, prod = fw["h"].reshape(B * 64, HID), fw["z"].reshape(B * 64, HID), fw["prod"].reshape(B * 64, EMB)
    g = {}
    g["QW2"] = dq.T @ h; g["QB2"] = dq.sum(0)
    dz = (dq @ w["QW2"]) * (z > 0)
    g["QW1"] = dz.T @ prod; g["QB1"] = dz.sum(0)
    dprod = (dz @ w["QW1"]).reshape(B, 64, EMB)
    dte = (dprod * fw["emb"][:, None, :]) * (fw["zc"] > 0)
    g["CW"] = dte.reshape(B * 64, EMB).T @ fw["cs"].reshape(B * 64, NCOS); g["CB"] = dte.reshape(B * 64, EMB).sum(0)
    dz3 = (dprod * fw["te"]).sum(1) * (fw["z3"] > 0)
    g["FW3"] = dz3.T @ fw["h2"]; g["FB3"] = dz3.sum(0)
    dz2 = (dz3 @ w["FW3"]) * (fw["z2"] > 0)
    g["FW2"] = dz2.T @ fw["h1"]; g["FB2"] = dz2.sum(0)
    dz1 = (dz2 @ w["FW2"]) * (fw["z1"] > 0)
    g["FW1"] = dz1.T @ fw["X"]; g["FB1"] = dz1.sum(0)
    return dtype(loss), pack_grads(g).astype(dtype), cur, fw


def adam_step(p, g, m, v, step, lr=5e-5, beta1=0.9, beta2=0.999, eps=0.01 / 32):   # eps: 1e-2 / batch_size (iqn.py:171)
    """torch's single-tensor Adam in f32 with the library's coefficients (in place on p, m, v)"""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    w1, b2_, w2, ss, rbc2, e = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(lr / bc1), f32(1.0 / np.sqrt(bc2)), f32(eps)
    g = np.asarray(g, f32)
    m[:] = m + w1 * (g - m)
    v[:] = v * b2_ + w2 * (g * g)
    denom = np.sqrt(v).astype(f32) * rbc2 + e
    p[:] = p - ss * (m / denom)


def batch_of(ringv, inds):
    """rows of one batch as iqn.py:228-232 gathers them from a [slots][N] ring (flat indices) -> (X, A, X_next, R, T)"""
    obs, actions, rewards, term = (np.asarray(a).reshape((-1,) + a.shape[2:]) for a in ringv)
    N = ringv[1].shape[1]
    inds = np.asarray(inds, np.int64)
    nx = (inds + N) % len(actions)
    return obs[inds], actions[inds], obs[nx], rewards[nx], term[nx]


def update(params, target_params, ringv, inds, taus, next_taus, tau_dashes, gamma=0.99, dtype=f32):
    """one update block -> dict(next_actions, target, current, loss, grads, q_next, fw)"""
    X, A, Xn, R, T = batch_of(ringv, inds)
    na, tg, qn = target(target_params, Xn, R, T, next_taus, tau_dashes, gamma, dtype)
    loss, grads, cur, fw = loss_grad(params, X, A, tg, taus, dtype)
    return dict(next_actions=na, target=tg, current=cur, loss=loss, grads=grads, q_next=qn, fw=fw, terminated=T, actions=A)


# ---- synthetic cases -----------------------------------------------------------------------------------
CASES = ((1, 1, 2), (5, 3, 7), (33, 2, 40), (32, 1, 300), (70, 2, 50))   # (batch, envs, slots); the last is larger than MI_IQN_MAX_SLABS = 64
CASE_SEEDS = {(1, 1, 2): 187, (5, 3, 7): 1, (33, 2, 40): 98, (32, 1, 300): 4, (70, 2, 50): 13}   # searched for by tests/test_iqn_cases_cpu.py's conditions


def init_realistic(rng):
    """reference-style initial parameters: kaiming-uniform weights and zero biases in the extractor, torch's default ranges elsewhere, the output layer scaled by 8 so
    that td errors straddle kappa.  Every ReLU input depends on the observation and the tau; used at the shapes small enough for a seed to keep all of them
    clear of 0 (32,768 head inputs per batch row: about one seed in three at one row, one in fifty at five)."""
    def uni(shape, bound):
        return rng.uniform(-bound, bound, size=shape).astype(f32)
    fan = dict(FW1=4, FW2=32, FW3=64, CW=64, CB=64, QW1=64, QB1=64, QW2=512, QB2=512)
    p = np.zeros(NPARAMS, f32)
    for k in ORDER:
        if k[0] == "F":
            v = uni(SHAPES[k], np.sqrt(6.0 / fan[k])) if k[1] == "W" else np.zeros(SHAPES[k], f32)
        else:
            v = uni(SHAPES[k], 1.0 / np.sqrt(fan[k])) * (f32(8) if k in ("QW2", "QB2") else f32(1))
        p[OFF[k]:OFF[k] + v.size] = v.astype(f32).ravel()
    return p


def init_params(rng):
    """Parameters of the larger synthetic cases.  A head of 512 units at 64 taus has 32,768 ReLU inputs per batch row: at reference-style values some of them lie
    within NEAR_ZERO of 0 for every seed once a batch has more than a few rows.  These cases use biases of either sign and magnitude in [1.5, 2.5] with weights small
    enough that no pre-activation crosses 0 (about half the units of every layer are off), yet large enough that the quantiles vary with tau by more than kappa,
    so that one row holds both Huber branches and both indicator values; the ReLU pattern near 0 is covered by the two small cases and the fixtures."""
    def uni(shape, bound):
        return rng.uniform(-bound, bound, size=shape).astype(f32)

    def bias(shape):
        return (rng.uniform(1.5, 2.5, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(f32)
    wscale = dict(FW1=0.1, FW2=0.05, FW3=0.03, CW=0.1, QW1=0.03, QW2=1.0)
    p = np.zeros(NPARAMS, f32)
    for k in ORDER:
        v = uni(SHAPES[k], wscale[k]) if k in wscale else (bias(SHAPES[k]) if k != "QB2" else uni(SHAPES[k], 0.5))
        p[OFF[k]:OFF[k] + v.size] = v.ravel()
    return p


REALISTIC = ((1, 1, 2),)   # the shape whose case uses reference-style parameters (at five rows no seed in 400 keeps every margin)


def make_case(batch, envs, slots, seed):
    """a synthetic ring + batch: random CartPole-range observations, ~20 % terminated rows, indices that include the wrap (the last slot), all taus.  The target
    network is the online one slightly perturbed, as between two syncs, so that td errors are of the order of kappa."""
    rng = np.random.default_rng(1000 * seed + 7 * batch + envs)
    obs = rng.uniform(-1, 1, size=(slots, envs, 4)).astype(f32) * np.array([2.4, 2.0, 0.21, 2.0], f32)
    actions = rng.integers(0, 2, size=(slots, envs)).astype(np.int64)
    rewards = np.ones((slots, envs), f32)
    term = (rng.uniform(size=(slots, envs)) < 0.2).astype(np.uint8)
    inds = rng.integers(0, slots * envs, size=batch).astype(np.int64)
    inds[0] = (slots - 1) * envs + (envs - 1)   # the successor wraps to slot 0
    if batch > 1:
        term.reshape(-1)[(inds[1] + envs) % (slots * envs)] = 1   # at least one terminated row
    params = init_realistic(rng) if (batch, envs, slots) in REALISTIC else init_params(rng)
    tparams = (params * (1 + 0.02 * rng.standard_normal(NPARAMS))).astype(f32)
    taus = rng.integers(0, 1 << 24, size=(batch, 64)).astype(f32) / f32(1 << 24)
    next_taus = rng.integers(0, 1 << 24, size=(batch, 32)).astype(f32) / f32(1 << 24)
    tau_dashes = rng.integers(0, 1 << 24, size=(batch, 64)).astype(f32) / f32(1 << 24)
    return dict(ring=(obs, actions, rewards, term), inds=inds, params=params, target_params=tparams, taus=taus, next_taus=next_taus, tau_dashes=tau_dashes)


def tensor_grad_errors(g, ref):
    """-> {tensor: max |g - ref| relative to that TENSOR's own max |ref|}: a small tensor's gradient is not hidden behind the output layer's"""
    a, b = unpack(np.asarray(g, np.float64), np.float64), unpack(np.asarray(ref, np.float64), np.float64)
    return {k: float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) for k in ORDER}


def case_conditions(case, r64):
    """-> dict of the margins a case must keep (float64 evaluation r64 = update(..., dtype=np.float64)) and what it reaches"""
    fw = r64["fw"]
    pre = np.concatenate([np.abs(fw[k]).ravel() for k in ("z1", "z2", "z3", "zc", "z")])
    d = r64["target"][:, None, :] - r64["current"][:, :, None]
    scale = max(1.0, float(np.abs(r64["target"]).max()), float(np.abs(r64["current"]).max()))
    qn = r64["q_next"]
    return dict(min_preact=float(pre.min()), min_kappa=float(np.abs(np.abs(d) - 1.0).min()), kappa_margin=NEAR_KAPPA_REL * scale,
                close_rows=int((np.abs(qn[:, 1] - qn[:, 0]) < CLOSE_Q).sum()), terminated_rows=int(np.asarray(r64["terminated"]).sum()),
                quad=int((np.abs(d) <= 1).sum()), lin=int((np.abs(d) > 1).sum()), neg=int((d < 0).sum()), pos=int((d >= 0).sum()),
                mixed_rows=int(((np.abs(d) <= 1).any(axis=(1, 2)) & (np.abs(d) > 1).any(axis=(1, 2)) & (d < 0).any(axis=(1, 2)) & (d >= 0).any(axis=(1, 2))).sum()),
                wraps=int(((case["inds"] + case["ring"][1].shape[1]) >= case["ring"][1].size).sum()))
