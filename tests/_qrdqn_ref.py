"""numpy restatement of the QR-DQN path (include/mi_qr.h "Numerics contract") — TEST INFRASTRUCTURE.

The reference has no qrdqn.py: the fixtures under tests/golden/qrdqn_* come from the same algorithm written as a plain torch script (tools/capture_qrdqn_ref.py:
autograd, optim.Adam, CPU), torch standing in for the reference.

Torso, quantiles, collapsed head, targets and the 64 x 64 loss stage in f32 in the header's expression and summation orders (the backward through the network in
numpy's own order), everything again in float64, the fixtures' loaders and the ring the torch script's run leaves behind.  numpy has no fmaf: ``fma32`` forms the
product and the sum in f64 and rounds once to f32 (a double rounding in rare cases), so comparisons of chains with the device are to tolerance; the loss stage has no
fma and is bit-exact.

Device bounds.  tests/test_qrdqn_ref_cpu.py measures this f32 restatement against the fixtures (torch's own f32 evaluation) at every checkpoint; each device
bound is 8 x the measured figure, the project's factor for "another f32 evaluation in another summation order".
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPARAMS, NQ, H1, H2 = 21644, 64, 120, 84
CHECKPOINTS = (0, 1, 50, 51, 2000, 4000)
T_STEPS, N_UPDATES = 50_000, 4001
f32 = np.float32
TAUS = ((2 * np.arange(NQ, dtype=f32) + 1) * f32(1 / 128)).astype(f32)   # (2 i + 1) / 128, exact

# measured by tests/test_qrdqn_ref_cpu.py (f32 restatement against torch's evaluation in the fixtures, maximum over the six checkpoints) -> device bound = 8 x
MEASURED_QUANT_ABS = 1.6e-5   # `current`, absolute (1.53e-5: two ulps of a quantile near 100)
MEASURED_Q_ABS = 1.7e-5     # action values through the collapsed head, absolute, against float64 (the fixtures hold no action values; 1.66e-5)
MEASURED_TARGET_ABS = 1.6e-5   # `target`, absolute
MEASURED_LOSS_REL = 1.2e-7    # loss, relative
MEASURED_GRAD_REL = 4.2e-7    # gradient, relative to max |g|
MEASURED_PARAMS_ABS = 6.0e-8   # parameters behind the first 51 updates chained (across both target syncs), absolute
MEASURED_CHAIN_LOSS_REL = 2.0e-7 # loss along those 51 updates, relative
BOUND_QUANT_ABS, BOUND_Q_ABS, BOUND_TARGET_ABS = 8 * MEASURED_QUANT_ABS, 8 * MEASURED_Q_ABS, 8 * MEASURED_TARGET_ABS
BOUND_LOSS_REL, BOUND_GRAD_REL, BOUND_PARAMS_ABS = 8 * MEASURED_LOSS_REL, 8 * MEASURED_GRAD_REL, 8 * MEASURED_PARAMS_ABS
BOUND_CHAIN_LOSS_REL = 8 * MEASURED_CHAIN_LOSS_REL
CLOSE_Q = 2 * BOUND_Q_ABS            # rows whose two action values are closer than this are left out of action comparisons ...
MAX_EXCLUDED = 0.01                  # ... and may be at most this share of a case's rows


def load_trace():
    out = {}
    for name in ("qrdqn_ref_trace.npz", "qrdqn_ref_trace_obs.npz", "qrdqn_ref_trace_inds.npz"):   # one run, three files: each stays below 1 MiB
        z = np.load(os.path.join(GOLD, name))
        out.update({k: z[k] for k in z.files})
    out["batch_inds"] = out["batch_inds"].astype(np.int32)
    return out


def load_ckpt(k):
    z = np.load(os.path.join(GOLD, "qrdqn_ref_ckpt%d.npz" % k))
    return {n: z[n] for n in z.files}


def ring(t):
    """The torch script's storage after its run: observations (50001, 4) f32, actions (50001,) i64, rewards (50001,) f32, terminated (50001,) u8.  Row g + 1 holds
    the RESET observation where step g ended an episode."""
    T = len(t["actions"])
    obs = np.zeros((T + 1, 4), f32); obs[1:] = t["obs"]
    for r, at in enumerate(t["reset_at"]):
        obs[at] = t["reset_states"][r].astype(f32)
    actions = np.zeros(T + 1, np.int64); actions[:T] = t["actions"]
    rewards = np.zeros(T + 1, f32); rewards[1:] = 1
    term = np.zeros(T + 1, np.uint8); term[1:] = t["terminated"]
    return obs, actions, rewards, term


def forced_resets(t):
    """(T, 4) f64: the state the env is reset to behind step g (zeros where step g ends no episode)"""
    fr = np.zeros((len(t["actions"]), 4), np.float64)
    for r, at in enumerate(t["reset_at"]):
        if at > 0:
            fr[at - 1] = t["reset_states"][r]
    return fr


def explore_draws(seed, env_id, ctrs):
    """the exploration stream of include/mi_qr.h (stream 3, idx = the env step counter): -> (u, random_action)"""
    from _reinforce_ref import philox
    r = philox(seed, np.uint64(env_id), np.asarray(ctrs, np.uint64), 3)
    return (r[..., 0] >> np.uint32(8)).astype(np.float64) / 16777216.0, (r[..., 1] & np.uint32(1)).astype(np.int64)


# ---- arithmetic -------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def unpack(p, dtype=f32):
    p = np.asarray(p, dtype)
    return (p[0:480].reshape(120, 4), p[480:600], p[600:10680].reshape(84, 120), p[10680:10764], p[10764:21516].reshape(128, 84), p[21516:21644])


def torso(params, X):
    """f32, the header's chains -> h1 (rows, 120), h2 (rows, 84)"""
    W1, b1, W2, b2, _W3, _b3 = unpack(params)
    X = np.asarray(X, f32).reshape(-1, 4)
    n = X.shape[0]
    z = np.broadcast_to(b1, (n, H1)).astype(f32)
    for k in range(4):
        z = fma32(W1[:, k][None, :], X[:, k][:, None], z)
    h1 = np.maximum(z, f32(0))
    parts = []
    for c in range(3):
        acc = np.broadcast_to(b2, (n, H2)).astype(f32) if c == 0 else np.zeros((n, H2), f32)
        for k in range(40 * c, 40 * c + 40):
            acc = fma32(W2[:, k][None, :], h1[:, k][:, None], acc)
        parts.append(acc)
    h2 = np.maximum(((parts[0] + parts[1]).astype(f32) + parts[2]).astype(f32), f32(0))
    return h1, h2


def collapse(params):
    """wbar (2, 84), bbar (2,) in f32: the serial sums over ascending i, scaled by 1 / 64"""
    _W1, _b1, _W2, _b2, W3, b3 = unpack(params)
    W3 = W3.reshape(2, NQ, H2); b3 = b3.reshape(2, NQ)
    s, sb = np.zeros((2, H2), f32), np.zeros(2, f32)
    for i in range(NQ):
        s = (s + W3[:, i]).astype(f32); sb = (sb + b3[:, i]).astype(f32)
    return (s * f32(1 / 64)).astype(f32), (sb * f32(1 / 64)).astype(f32)


def forward(params, X):
    """f32 -> quantiles (rows, 2, 64), q (rows, 2) through the collapsed head, h1, h2"""
    W3, b3 = unpack(params)[4:]
    h1, h2 = torso(params, X)
    n = h2.shape[0]
    acc = np.broadcast_to(b3, (n, 2 * NQ)).astype(f32)
    for k in range(H2):
        acc = fma32(W3[:, k][None, :], h2[:, k][:, None], acc)
    wbar, bbar = collapse(params)
    q = np.broadcast_to(bbar, (n, 2)).astype(f32)
    for k in range(H2):
        q = fma32(wbar[:, k][None, :], h2[:, k][:, None], q)
    return acc.reshape(n, 2, NQ), q, h1, h2


def forward64(params, X):
    """float64 on the same f32 inputs -> quantiles (rows, 2, 64), q (rows, 2) = their mean, z1 (rows, 120), z2 (rows, 84) (the pre-activations)"""
    W1, b1, W2, b2, W3, b3 = unpack(np.asarray(params, f32).astype(np.float64), np.float64)
    X = np.asarray(X, f32).astype(np.float64).reshape(-1, 4)
    z1 = X @ W1.T + b1
    z2 = np.maximum(z1, 0) @ W2.T + b2
    th = (np.maximum(z2, 0) @ W3.T + b3).reshape(-1, 2, NQ)
    return th, th.mean(-1), z1, z2


def target(target_params, obs_next, rewards, terminated, gamma=0.99, dtype=f32):
    """-> (next_actions, target (rows, 64), q); gamma is the f32 value the kernel is handed"""
    if dtype is f32:
        th, q = forward(target_params, obs_next)[:2]
    else:
        th, q = forward64(target_params, obs_next)[:2]
    a = (q[:, 1] > q[:, 0]).astype(np.int64)
    nq = th[np.arange(len(a)), a]
    lg = np.where(np.asarray(terminated) != 0, dtype(0), dtype(f32(gamma)))[:, None].astype(dtype)
    r = np.asarray(rewards, f32).astype(dtype)[:, None]
    return a, (r + (lg * nq).astype(dtype)).astype(dtype), q


def huber_rows(current, tgt, n_rows_total=None):
    """the loss stage of the header in f32, bit for bit (no fma in it) -> (rowloss (rows,), dcurrent (rows, 64)); inv = 1 / (n_rows_total * 64)"""
    cur, tgt = np.asarray(current, f32), np.asarray(tgt, f32)
    B = cur.shape[0]
    inv = f32(1.0) / f32((n_rows_total or B) * NQ)
    u = (tgt[:, None, :] - cur[:, :, None]).astype(f32)                      # [b][i][j]
    au = np.abs(u)
    L = np.where(au <= 1, ((f32(0.5) * u).astype(f32) * u).astype(f32), (au - f32(0.5)).astype(f32)).astype(f32)
    c = np.minimum(np.maximum(u, f32(-1)), f32(1))
    w = np.abs((TAUS[None, :, None] - (u < 0).astype(f32)).astype(f32))
    wl, wc = (w * L).astype(f32), (w * c).astype(f32)
    T, S = np.zeros((4, B, NQ), f32), np.zeros((4, B, NQ), f32)
    for cc in range(4):
        for j in range(16 * cc, 16 * cc + 16):
            T[cc] = (T[cc] + wl[:, :, j]).astype(f32); S[cc] = (S[cc] + wc[:, :, j]).astype(f32)
    Li = (((T[0] + T[1]).astype(f32) + T[2]).astype(f32) + T[3]).astype(f32)
    G = (((S[0] + S[1]).astype(f32) + S[2]).astype(f32) + S[3]).astype(f32)
    rowloss = np.zeros(B, f32)
    for i in range(NQ):
        rowloss = (rowloss + Li[:, i]).astype(f32)
    return rowloss, (-(G * inv).astype(f32)).astype(f32)


def sum_rows_ascending(rowloss):
    s = f32(0)
    for v in np.asarray(rowloss, f32):
        s = f32(s + v)
    return s


def sum_rows_slabs(rowloss):
    """SUMROWS of mi_qr_grad: G = min(B, 128) slabs own rows g, g + G, ...; 16 groups (g mod 16) on four interleaved accumulators; groups ascending"""
    v = np.asarray(rowloss, f32)
    B = len(v); G = min(B, 128)
    slabs = np.zeros(G, f32)
    for b in range(B):
        slabs[b % G] = f32(slabs[b % G] + v[b])
    total = None
    for k in range(16):
        s = [f32(0)] * 4
        for n, g in enumerate(range(k, G, 16)):
            s[n % 4] = f32(s[n % 4] + slabs[g])
        part = f32(f32(s[0] + s[1]) + f32(s[2] + s[3]))
        total = part if total is None else f32(total + part)
    return total


def huber64(current, tgt):
    """float64 -> (loss, dcurrent (rows, 64))"""
    cur, tgt = np.asarray(current, np.float64), np.asarray(tgt, np.float64)
    B = cur.shape[0]
    u = tgt[:, None, :] - cur[:, :, None]
    au = np.abs(u)
    L = np.where(au <= 1, 0.5 * u * u, au - 0.5)
    w = np.abs(TAUS.astype(np.float64)[None, :, None] - (u < 0))
    return (w * L).sum() / (B * NQ), -(w * np.clip(u, -1, 1)).sum(-1) / (B * NQ)


def loss_grad(params, X, A, tgt, dtype=f32):
    """loss and its hand-derived gradient w.r.t. the flat parameters -> (loss, grad, current (rows, 64)).  f32: forward and loss stage in the header's orders
    (rows summed in the slab order), the backward through the network in numpy's own order; float64: everything in float64."""
    A = np.asarray(A, np.int64)
    W1, b1, W2, b2, W3, b3 = unpack(np.asarray(params, f32).astype(dtype), dtype)
    Xd = np.asarray(X, f32).astype(dtype).reshape(-1, 4)
    B = Xd.shape[0]
    rows = np.arange(B)
    if dtype is f32:
        th, _q, h1, h2 = forward(params, X)
        cur = th[rows, A]
        rowloss, d = huber_rows(cur, tgt)
        loss = f32(sum_rows_slabs(rowloss) * (f32(1.0) / f32(B * NQ)))
        m1, m2 = h1 > 0, h2 > 0
    else:
        th, _q, z1, z2 = forward64(params, X)
        h1, h2 = np.maximum(z1, 0), np.maximum(z2, 0)
        cur = th[rows, A]
        loss, d = huber64(cur, tgt)
        m1, m2 = z1 > 0, z2 > 0
    dth = np.zeros((B, 2, NQ), dtype); dth[rows, A] = d
    dth = dth.reshape(B, 2 * NQ)
    gW3 = dth.T @ h2; gb3 = dth.sum(0)
    dz2 = (dth @ W3) * m2
    gW2 = dz2.T @ h1; gb2 = dz2.sum(0)
    dz1 = (dz2 @ W2) * m1
    gW1 = dz1.T @ Xd; gb1 = dz1.sum(0)
    return dtype(loss), np.concatenate([gW1.ravel(), gb1, gW2.ravel(), gb2, gW3.ravel(), gb3]).astype(dtype), cur


def adam_step(p, g, m, v, step, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=0.01 / 128):
    """torch's single-tensor Adam in f32 with the library's coefficients (in place on p, m, v)"""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    w1, b2_, w2, ss, rbc2, e = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(lr / bc1), f32(1.0 / np.sqrt(bc2)), f32(eps)
    g = np.asarray(g, f32)
    m[:] = m + w1 * (g - m)
    v[:] = v * b2_ + w2 * (g * g)
    denom = np.sqrt(v).astype(f32) * rbc2 + e
    p[:] = p - ss * (m / denom)


def batch_of(ringv, inds):
    """rows of one batch as the script gathers them -> (X, A, X_next, R, T)"""
    obs, actions, rewards, term = ringv
    inds = np.asarray(inds, np.int64)
    return obs[inds], actions[inds], obs[inds + 1], rewards[inds + 1], term[inds + 1]


def results_dir():
    from _c51_ref import results_dir as rd
    return rd()
