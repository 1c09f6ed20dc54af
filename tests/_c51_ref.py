"""numpy restatement of the C51 path (include/mi_c51.h "Numerics contract") — TEST INFRASTRUCTURE.

Forward, action values, categorical projection, loss and gradient in f32 (the header's expression and summation orders for the forward and the projection; the
gradient in numpy's own order) and in float64, the fixtures' loaders and the ring the reference's run leaves behind.  numpy has no fmaf: ``fma32`` forms the
product and the sum in f64 and rounds once more to f32, so comparisons with the device are to tolerance; the projection has no fma and is bit-exact.

Device bounds.  tests/test_c51_ref_pinned_cpu.py measures this f32 restatement against the fixtures (the reference's own f32 evaluation by torch) at every
checkpoint; each device bound is 8 x the measured figure: the project's margin for "another f32 evaluation in another summation order plus ~1-ulp exp / log".
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPARAMS, N_ATOMS, H1, H2 = 27934, 101, 120, 84
OFF = dict(W1=0, b1=480, W2=600, b2=10680, W3=10764, b3=27732)
CHECKPOINTS = (0, 1, 50, 51, 500, 1000)
f32 = np.float32
ATOMS = (f32(-100) + f32(2) * np.arange(N_ATOMS, dtype=f32)).astype(f32)   # z_j; equal to torch.linspace(-100, 100, 101) bit for bit (asserted on the CPU)

# measured by tests/test_c51_ref_pinned_cpu.py (f32 restatement against the reference's torch evaluation, maximum over the six checkpoints) -> device bound = 8 x
MEASURED_PROBS_ABS = 3.0e-7          # probs of c51.py:156, absolute
MEASURED_TARGET_PROBS_ABS = 1.5e-7   # target_probs of :151-154 (through the target network's forward), absolute (1.49e-7)
MEASURED_Q_ABS = 2.2e-6              # action values of :143, absolute, against float64: the fixture holds no action values (2.18e-6; max |q| is 13.3)
MEASURED_LOSS_REL = 1.1e-7           # loss of :158, relative (1.03e-7)
MEASURED_GRAD_REL = 1.1e-6           # gradient, relative to max |g| (1.06e-6)
BOUND_PROBS_ABS, BOUND_TARGET_PROBS_ABS, BOUND_Q_ABS = 8 * MEASURED_PROBS_ABS, 8 * MEASURED_TARGET_PROBS_ABS, 8 * MEASURED_Q_ABS
BOUND_LOSS_REL, BOUND_GRAD_REL = 8 * MEASURED_LOSS_REL, 8 * MEASURED_GRAD_REL
CLOSE_Q = 2 * BOUND_Q_ABS            # rows whose two action values are closer than this are left out of action comparisons ...
MAX_EXCLUDED = 0.01                  # ... and may be at most this share of a case's rows


def results_dir():
    """Where the GPU tests leave their observed figures: $MIRL_RESULTS_DIR, else results_out/ in the repository root (git-ignored)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.environ.get("MIRL_RESULTS_DIR") or os.path.join(root, "results_out")
    os.makedirs(d, exist_ok=True)
    return d


def load_trace():
    z = np.load(os.path.join(GOLD, "c51_ref_trace.npz"))
    return {k: z[k] for k in z.files}


def load_ckpt(k):
    z = np.load(os.path.join(GOLD, "c51_ref_ckpt%d.npz" % k))
    return {n: z[n] for n in z.files}


def ring(t):
    """The reference's storage after its run (c51.py:80-83,88,103,114-116): observations (20001, 4) f32, actions (20001,) i64, rewards (20001,) f32,
    terminated (20001,) u8.  Row g + 1 holds the RESET observation where step g ended an episode."""
    T = len(t["actions"])
    obs = np.zeros((T + 1, 4), f32); obs[1:] = t["obs"]
    for r, at in enumerate(t["reset_at"]):
        obs[at] = t["reset_states"][r].astype(f32)
    actions = np.zeros(T + 1, np.int64); actions[:T] = t["actions"]
    rewards = np.zeros(T + 1, f32); rewards[1:] = 1
    term = np.zeros(T + 1, np.uint8); term[1:] = t["terminated"]
    return obs, actions, rewards, term


def forced_resets(t):
    """(20000, 4) f64: the state the env is reset to behind step g (zeros where step g ends no episode)"""
    fr = np.zeros((len(t["actions"]), 4), np.float64)
    for r, at in enumerate(t["reset_at"]):
        if at > 0:
            fr[at - 1] = t["reset_states"][r]
    return fr


def explore_draws(seed, env_id, ctrs):
    """the exploration stream of include/mi_c51.h (stream 3, idx = the env step counter): -> (u, random_action) with u = (w0 >> 8) / 2^24 and action = w1 & 1"""
    from _reinforce_ref import philox
    r = philox(seed, np.uint64(env_id), np.asarray(ctrs, np.uint64), 3)
    return (r[..., 0] >> np.uint32(8)).astype(np.float64) / 16777216.0, (r[..., 1] & np.uint32(1)).astype(np.int64)


# ---- arithmetic -------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def tree64(q):
    """balanced pairwise f32 sum over the last axis (64 lanes in natural order)"""
    q = np.asarray(q, f32)
    while q.shape[-1] > 1:
        q = (q[..., 0::2] + q[..., 1::2]).astype(f32)
    return q[..., 0]


def tree2(v):
    """TREE2 of the header over the last axis (101 values): lane i holds v_i + v_{i + 64} (v_i alone past atom 100), then the pairwise tree"""
    v = np.asarray(v, f32)
    lanes = v[..., :64].copy()
    lanes[..., :N_ATOMS - 64] = (v[..., :N_ATOMS - 64] + v[..., 64:]).astype(f32)
    return tree64(lanes)


def unpack(p, dtype=f32):
    p = np.asarray(p, dtype)
    return (p[0:480].reshape(120, 4), p[480:600], p[600:10680].reshape(84, 120), p[10680:10764], p[10764:27732].reshape(202, 84), p[27732:27934])


def forward(params, X):
    """f32, the header's chains -> logits (rows, 2, 101), h1 (rows, 120), h2 (rows, 84)"""
    W1, b1, W2, b2, W3, b3 = unpack(params)
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
    acc = np.broadcast_to(b3, (n, 202)).astype(f32)
    for k in range(H2):
        acc = fma32(W3[:, k][None, :], h2[:, k][:, None], acc)
    return acc.reshape(n, 2, N_ATOMS), h1, h2


def softmax_q(logits):
    """f32 -> probs (rows, 2, 101), q (rows, 2) in the header's order"""
    L = np.asarray(logits, f32)
    m = L.max(axis=-1, keepdims=True)
    e = np.exp((L - m).astype(f32)).astype(f32)
    s = tree2(e)[..., None]
    p = (e / s).astype(f32)
    lanes = (p[..., :64] * ATOMS[:64]).astype(f32)
    lanes[..., :N_ATOMS - 64] = fma32(p[..., 64:], ATOMS[64:], lanes[..., :N_ATOMS - 64])
    return p, tree64(lanes)


def probs_q(params, X):
    return softmax_q(forward(params, X)[0])


def forward64(params, X):
    """float64 on the same f32 inputs -> probs (rows, 2, 101), q (rows, 2), z1 (rows, 120), z2 (rows, 84) (the pre-activations)"""
    W1, b1, W2, b2, W3, b3 = unpack(np.asarray(params, f32).astype(np.float64), np.float64)
    X = np.asarray(X, f32).astype(np.float64).reshape(-1, 4)
    z1 = X @ W1.T + b1
    z2 = np.maximum(z1, 0) @ W2.T + b2
    L = (np.maximum(z2, 0) @ W3.T + b3).reshape(-1, 2, N_ATOMS)
    e = np.exp(L - L.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    return p, (p * ATOMS.astype(np.float64)).sum(-1), z1, z2


def project(next_probs, rewards, terminated, gamma=0.99):
    """c51.py:132-154 in f32, the reference's operations in the reference's order; accumulation per target atom: lower contributions in ascending j, then the upper
    ones (index_add_ on the CPU).  -> (m (rows, 101), l, u, b)"""
    p = np.asarray(next_probs, f32)
    r = np.asarray(rewards, f32).reshape(-1, 1)
    live = (1 - np.asarray(terminated).astype(f32)).astype(f32).reshape(-1, 1)
    tz = (r + ((f32(gamma) * ATOMS).astype(f32)[None, :] * live).astype(f32)).astype(f32)
    tz = np.minimum(np.maximum(tz, f32(-100)), f32(100))
    b = ((tz + f32(100)).astype(f32) / f32(2)).astype(f32)
    l, u = np.floor(b), np.ceil(b)
    wl = (((u + (l == u).astype(f32)).astype(f32) - b).astype(f32) * p).astype(f32)
    wu = ((b - l).astype(f32) * p).astype(f32)
    li, ui = l.astype(np.int64), u.astype(np.int64)
    m = np.zeros_like(p)
    rows = np.arange(p.shape[0])
    for j in range(N_ATOMS):
        m[rows, li[:, j]] = (m[rows, li[:, j]] + wl[:, j]).astype(f32)
    for j in range(N_ATOMS):
        m[rows, ui[:, j]] = (m[rows, ui[:, j]] + wu[:, j]).astype(f32)
    return m, li, ui, b


def project64(next_probs, rewards, terminated, gamma=0.99):
    """float64 form on the same inputs (gamma is the f32 value the kernel is handed)"""
    p = np.asarray(next_probs, np.float64)
    r = np.asarray(rewards, np.float64).reshape(-1, 1)
    live = 1.0 - np.asarray(terminated).astype(np.float64).reshape(-1, 1)
    b = (np.clip(r + float(f32(gamma)) * ATOMS.astype(np.float64)[None, :] * live, -100, 100) + 100) / 2
    l, u = np.floor(b), np.ceil(b)
    m = np.zeros_like(p)
    rows = np.arange(p.shape[0])
    for j in range(N_ATOMS):
        np.add.at(m, (rows, l[:, j].astype(np.int64)), (u[:, j] + (l[:, j] == u[:, j]) - b[:, j]) * p[:, j])
        np.add.at(m, (rows, u[:, j].astype(np.int64)), (b[:, j] - l[:, j]) * p[:, j])
    return m


def target(target_params, obs_next, rewards, terminated, gamma=0.99, dtype=f32):
    """-> (next_actions, target_probs, q) of c51.py:132-154"""
    if dtype is f32:
        p, q = probs_q(target_params, obs_next)
    else:
        p, q = forward64(target_params, obs_next)[:2]
    a = (q[:, 1] > q[:, 0]).astype(np.int64)
    nxt = p[np.arange(len(a)), a]
    m = project(nxt, rewards, terminated, gamma)[0] if dtype is f32 else project64(nxt, rewards, terminated, gamma)
    return a, m, q


def loss_grad(params, X, A, M, dtype=f32):
    """loss of c51.py:158 and its gradient w.r.t. the flat parameters, dtype f32 (numpy's own summation order) or float64 -> (loss, grad, probs (rows, 101))"""
    W1, b1, W2, b2, W3, b3 = unpack(np.asarray(params, f32).astype(dtype), dtype)
    X = np.asarray(X, f32).astype(dtype).reshape(-1, 4); M = np.asarray(M).astype(dtype); A = np.asarray(A, np.int64)
    B = X.shape[0]
    rows = np.arange(B)
    z1 = X @ W1.T + b1; h1 = np.maximum(z1, 0)
    z2 = h1 @ W2.T + b2; h2 = np.maximum(z2, 0)
    L = (h2 @ W3.T + b3).reshape(B, 2, N_ATOMS)[rows, A]
    e = np.exp(L - L.max(axis=-1, keepdims=True))
    p = (e / e.sum(axis=-1, keepdims=True)).astype(dtype)
    eps = dtype(1e-8)
    loss = (-(M * np.log(p + eps)).sum(-1)).sum() / dtype(B)
    g = -M / (p + eps)
    dl = (p * (g - (p * g).sum(-1, keepdims=True))) / dtype(B)
    dL = np.zeros((B, 2, N_ATOMS), dtype); dL[rows, A] = dl
    dL = dL.reshape(B, 202)
    gW3 = dL.T @ h2; gb3 = dL.sum(0)
    dz2 = (dL @ W3) * (z2 > 0)
    gW2 = dz2.T @ h1; gb2 = dz2.sum(0)
    dz1 = (dz2 @ W2) * (z1 > 0)
    gW1 = dz1.T @ X; gb1 = dz1.sum(0)
    return dtype(loss), np.concatenate([gW1.ravel(), gb1, gW2.ravel(), gb2, gW3.ravel(), gb3]).astype(dtype), p


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
    """rows of one batch as c51.py:126-130 gathers them -> (X, A, X_next, R, T)"""
    obs, actions, rewards, term = ringv
    inds = np.asarray(inds, np.int64)
    return obs[inds], actions[inds], obs[inds + 1], rewards[inds + 1], term[inds + 1]
