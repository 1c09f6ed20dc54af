"""numpy restatement of the REINFORCE path (include/mi_reinforce.h "Numerics contract" / "RNG contract") — TEST INFRASTRUCTURE.

Forward with a given mask, returns + per-episode normalisation, gradient, Adam, the keyed dropout mask and the action uniforms (Philox checked against
``oracle.cpu_ref.philox``), env stepping through ``oracle.cpu_ref``.  Accumulation orders are the header's: bias-first k-ascending fma chains for the hidden
layer, lane pairs (units i, i + 64) and a balanced pairwise tree over the 64 lanes for the logits and the return statistics.  numpy has no fmaf:
``fma32`` forms the product and the sum in f64 and rounds once more to f32 (the product of two f32 is exact in f64; the double rounding of the sum differs
from a true fma in rare last-bit cases, so comparisons with the device are to tolerance, bitwise only for integers: masks, actions, lengths, done).
"""
import os

import numpy as np

from oracle import cpu_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPARAMS, HID, MAX_STEPS, ROWS = 898, 128, 500, 501
STREAM_ACTION, STREAM_DROPOUT, KEEP_BELOW = 1, 8, 0x66666666
EXP_M5 = np.float32(0.006737947)
f32 = np.float32


def results_dir():
    """Where the GPU tests leave their observed figures: $MIRL_RESULTS_DIR, else the directory in which this run's other learning tests (tests/test_gpu_learning.py)
    have written learning_stats_gpu.json — the REINFORCE record joins it under its own key —, else results_out/ in the repository root (git-ignored)."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.environ.get("MIRL_RESULTS_DIR")
    if not d:
        found = [f for f in glob.glob(os.path.join(root, "*", "learning_stats_gpu.json")) if os.path.basename(os.path.dirname(f)) not in ("profiles", "tests")]
        d = os.path.dirname(sorted(found, key=os.path.getmtime)[-1]) if found else os.path.join(root, "results_out")
    os.makedirs(d, exist_ok=True)
    return d


def load_trace():
    z = np.load(os.path.join(GOLD, "reinforce_ref_trace.npz"))
    t = {k: z[k] for k in z.files}
    t["offsets"] = np.concatenate([[0], np.cumsum(t["lengths"])]).astype(np.int64)
    t["masks"] = np.unpackbits(t["masks_packed"], axis=1, bitorder="little").astype(bool)      # (rows, 128)
    t["mask_words"] = np.ascontiguousarray(t["masks_packed"]).view("<u4").reshape(-1, 4)        # (rows, 4): unit u = bit (u & 31) of word u >> 5
    return t


def episode(t, e):
    """-> dict of update e: X (len, 4) the observations the policy saw, A, M, mask words, params before the update, reference outputs"""
    a, b = int(t["offsets"][e]), int(t["offsets"][e + 1])
    X = np.concatenate([t["reset_states"][e].astype(f32)[None], t["obs"][a:b - 1]]).astype(f32)
    return dict(X=X, A=t["actions"][a:b].astype(np.int64), M=t["masks"][a:b], W=t["mask_words"][a:b], obs_after=t["obs"][a:b], terminated=t["terminated"][a:b],
                params=(t["init_params"] if e == 0 else t["params_after"][e - 1]), grads=t["grads"][e], b_returns=t["b_returns"][a:b],
                b_log_probs=t["b_log_probs"][a:b], policy_loss=t["policy_loss"][e], reset=t["reset_states"][e], length=b - a)


# ---- arithmetic -------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def tree64(q):
    """balanced pairwise f32 sum over the last axis (64 lanes in natural order)"""
    q = np.asarray(q, f32)
    while q.shape[-1] > 1:
        q = (q[..., 0::2] + q[..., 1::2]).astype(f32)
    return q[..., 0]


def unpack(p):
    p = np.asarray(p, f32)
    return p[:512].reshape(128, 4), p[512:640], p[640:896].reshape(2, 128), p[896:898]


def forward(params, X, M=None):
    """-> probs (rows, 2), log_probs (rows, 2), H (rows, 128).  M (rows, 128) bool: the dropout masks; None: eval mode."""
    W1, b1, W2, b2 = unpack(params)
    X = np.asarray(X, f32).reshape(-1, 4)
    z = np.broadcast_to(b1, (X.shape[0], 128)).astype(f32)
    for k in range(4):
        z = fma32(W1[:, k][None, :], X[:, k][:, None], z)
    if M is None:
        H = np.maximum(z, f32(0))
    else:
        H = np.where(M, np.maximum((z * f32(2.5)).astype(f32), f32(0)), f32(0)).astype(f32)
    L = np.empty((X.shape[0], 2), f32)
    for a in range(2):
        q = fma32(W2[a, 64:][None, :], H[:, 64:], (W2[a, :64][None, :] * H[:, :64]).astype(f32))
        L[:, a] = (b2[a] + tree64(q)).astype(f32)
    m = L.max(axis=1, keepdims=True)
    d = (L - m).astype(f32)
    e = np.exp(d).astype(f32)
    s = (e[:, 0] + e[:, 1]).astype(f32)[:, None]
    return (e / s).astype(f32), (d - np.log(s).astype(f32)).astype(f32), H


def returns_normalised(length, gamma=0.99):
    """-> (R, Rn) of an episode of `length` unit rewards, in the returns kernel's order"""
    g = f32(gamma)
    Rr = np.zeros(length, f32)
    acc = f32(0)
    for t in range(length - 1, -1, -1):
        acc = fma32(g, acc, f32(1)); Rr[t] = acc
    pad = np.zeros(512, f32); pad[:length] = Rr
    lanes = pad.reshape(8, 64)                       # row j, lane i = element i + 64 j
    part = np.zeros(64, f32)
    for j in range(8):
        part = (part + lanes[j]).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = f32(tree64(part)) / f32(length)
        valid = (np.arange(512) < length).reshape(8, 64)
        sq = np.zeros(64, f32)
        for j in range(8):
            dj = (lanes[j] - mean).astype(f32)
            sq = np.where(valid[j], fma32(dj, dj, sq), sq)
        var = f32(tree64(sq)) / f32(length - 1)
        denom = f32(np.sqrt(var)) + EXP_M5
        return Rr, ((Rr - mean) / denom).astype(f32)


def forward64(params, X, M=None):
    """float64 form of `forward` on the same f32 inputs: -> probs (rows, 2), log_probs (rows, 2), logits (rows, 2), Z (rows, 128) the hidden pre-activations"""
    W1, b1, W2, b2 = [w.astype(np.float64) for w in unpack(params)]
    X = np.asarray(X, np.float64).reshape(-1, 4)
    Z = X @ W1.T + b1
    H = np.maximum(Z, 0.0) if M is None else np.where(M, np.maximum(Z * 2.5, 0.0), 0.0)
    L = H @ W2.T + b2
    d = L - L.max(axis=1, keepdims=True)
    lp = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    return np.exp(lp), lp, L, Z


def returns_normalised64(length, gamma=0.99):
    """float64 form of `returns_normalised` (gamma is the f32 value the kernel is handed): -> (R, Rn); a one-row episode gives NaN in Rn"""
    g = float(f32(gamma))
    Rr = np.zeros(length, np.float64)
    acc = 0.0
    for t in range(length - 1, -1, -1):
        acc = g * acc + 1.0; Rr[t] = acc
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = Rr.sum() / np.float64(length)
        var = ((Rr - mean) ** 2).sum() / np.float64(length - 1)
        return Rr, (Rr - mean) / (np.sqrt(var) + np.exp(-5.0))


def adam_step64(p, g, m, v, step, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8):
    """float64 form of `adam_step` (in place on float64 p, m, v)"""
    g = np.asarray(g, np.float64)
    m[:] = m + (1.0 - beta1) * (g - m)
    v[:] = v * beta2 + (1.0 - beta2) * (g * g)
    p[:] = p - (lr / (1.0 - beta1 ** step)) * (m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** step) + eps))


def grad(params, X, A, M, Rn, dtype=f32):
    """gradient of sum(-log_prob * Rn) w.r.t. the flat parameters; dtype f32 (vectorised, numpy's own summation order) or f64"""
    W1, b1, W2, b2 = [w.astype(dtype) for w in unpack(params)]
    X = np.asarray(X, dtype); Rn = np.asarray(Rn, dtype); A = np.asarray(A, np.int64)
    Z = X @ W1.T + b1
    H = np.where(M, np.maximum(Z * dtype(2.5), 0), 0).astype(dtype)
    L = H @ W2.T + b2
    L = L - L.max(1, keepdims=True)
    P = np.exp(L); P = P / P.sum(1, keepdims=True)
    dL = P.copy(); dL[np.arange(len(A)), A] -= 1; dL = dL * Rn[:, None]
    gW2 = dL.T @ H; gb2 = dL.sum(0)
    dZ = (dL @ W2) * (H > 0) * dtype(2.5)
    gW1 = dZ.T @ X; gb1 = dZ.sum(0)
    return np.concatenate([gW1.ravel(), gb1, gW2.ravel(), gb2]).astype(dtype)


def adam_step(p, g, m, v, step, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch's single-tensor Adam in f32 with the library's coefficients (in place on p, m, v)"""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    w1, b2_, w2, ss, rbc2, e = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(lr / bc1), f32(1.0 / np.sqrt(bc2)), f32(eps)
    g = np.asarray(g, f32)
    m[:] = m + w1 * (g - m)
    v[:] = v * b2_ + w2 * (g * g)
    denom = np.sqrt(v).astype(f32) * rbc2 + e
    p[:] = p - ss * (m / denom)


# ---- RNG --------------------------------------------------------------------------------------------
def philox(seed, env, idx, stream):
    """vectorised Philox4x32-10 with the library's counter layout; env / idx broadcast -> (..., 4) uint32"""
    env = np.asarray(env, np.uint64); idx = np.asarray(idx, np.uint64)
    env, idx = np.broadcast_arrays(env, idx)
    M32 = np.uint64(0xFFFFFFFF)
    c = [env & M32, env >> np.uint64(32), idx & M32, (((idx >> np.uint64(32)) << np.uint64(4)) | np.uint64(stream)) & M32]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32; k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def keyed_masks(seed, env_id, ctrs):
    """-> (len(ctrs), 128) bool: unit u of env-step c keeps iff philox(seed, E, 32 c + ((u & 63) >> 1), 8)[2 (u & 1) + (u >> 6)] < 0x66666666"""
    ctrs = np.asarray(ctrs, np.uint64).reshape(-1)
    r = philox(seed, np.uint64(env_id), ctrs[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64)[None, :], STREAM_DROPOUT)   # (steps, 32, 4)
    u = np.arange(128)
    return r[:, (u & 63) >> 1, 2 * (u & 1) + (u >> 6)] < np.uint32(KEEP_BELOW)


def mask_words(M):
    """(rows, 128) bool -> (rows, 4) uint32, the storage layout"""
    return np.ascontiguousarray(np.packbits(np.asarray(M, bool), axis=1, bitorder="little")).view("<u4").reshape(-1, 4)


def words_to_masks(W):
    W = np.ascontiguousarray(np.asarray(W).astype("<u4"))
    return np.unpackbits(W.view(np.uint8).reshape(-1, 16), axis=1, bitorder="little").astype(bool)


def action_uniforms(seed, env_id, ctrs):
    ctrs = np.asarray(ctrs, np.uint64).reshape(-1)
    r = philox(seed, np.uint64(env_id), ctrs >> np.uint64(2), STREAM_ACTION)
    w = r[np.arange(len(ctrs)), (ctrs & np.uint64(3)).astype(np.int64)]
    return ((w >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


# ---- env --------------------------------------------------------------------------------------------
def replay_episode(reset_state, actions, next_reset=None):
    """Teacher-forced oracle episode: -> (obs after each step (k, 4) f32, terminated (k,), done (k,), truncated (k,)) up to and including the first done.
    Steps `oracle.cpu_ref.VecCartPole` (TimeLimit, done) and, from its f64 state, `cpu_ref.cartpole_step` for the observation gym returns on the LAST step
    (VecCartPole hands back the reset observation there, as ppo.py's loop wants it); on all other steps the two must agree bit for bit."""
    env = R.VecCartPole(1, seed=1)
    env.reset(np.asarray(reset_state, np.float64).reshape(1, 4))
    nr = np.zeros((1, 4)) if next_reset is None else np.asarray(next_reset, np.float64).reshape(1, 4)
    obs, term, done, trunc = [], [], [], []
    for a in actions:
        ns, tm = R.cartpole_step(env.state[0].copy(), int(a))
        o, _r, d, tr, _fr, _fl = env.step(np.array([int(a)]), forced_reset=nr)
        if not d[0]:
            assert np.array_equal(o[0], ns.astype(f32))
        obs.append(ns.astype(f32)); term.append(bool(tm)); done.append(bool(d[0])); trunc.append(bool(tr[0]))
        if d[0]:
            break
    return np.array(obs, f32), np.array(term), np.array(done), np.array(trunc)
