"""Synthetic C51 cases — TEST INFRASTRUCTURE: rings, batches and parameters that reach what the reference's run never does (include/mi_c51.h).

The reference's run keeps b inside [1, 100], has one env and a batch of 128.  These cases add: rewards that drive the clamp of c51.py:135 at both ends, fractional and
integral b, terminated rows, rows whose successor wraps around the ring, several envs, batches of 1 row, of no multiple of anything, of 40 rows (40 slabs: the slab sum's
second and third interleaved accumulators end on a partial pass) and of more rows than the gradient launch has workgroups (128: a workgroup then walks several rows).  Parameters are drawn at torch's default-init scale and observations inside CartPole's
range, so the figures the device bounds come from (tests/_c51_ref.py) describe these cases too; the expected values are float64 (tests/_c51_ref.py).
A ReLU pre-activation within NEAR_ZERO of 0 may land on either side of the kink in another evaluation order: the cases are chosen (by their seeds) so that at most
KINK_SHARE of a case's rows have one — no row is excluded from a gradient comparison.
"""
import numpy as np

import _c51_ref as X

f32 = np.float32
NEAR_ZERO = 1e-5
KINK_SHARE = 0.01
#        (batch, n_envs, slots, seed)
SHAPES = ((1, 1, 2, 76), (5, 3, 7, 62), (129, 2, 80, 68), (300, 4, 100, 59), (128, 1, 300, 55), (40, 2, 30, 93))
REWARDS = np.array([1.0, -300.0, 250.0, 0.5, -7.25, 0.0, 100.0], f32)   # 1: the reference's; -300 / 250: the clamp at both ends; 0.5, -7.25: fractional b everywhere


def default_init(rng):
    """a flat parameter vector at torch's default nn.Linear scale: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))"""
    parts = []
    for fan_in, n in ((4, 480), (4, 120), (120, 10080), (120, 84), (84, 16968), (84, 202)):
        k = 1.0 / np.sqrt(fan_in)
        parts.append(rng.uniform(-k, k, n))
    # a trained head is far from uniform: spread the last layer so that the distributions have structure and the two action values differ
    parts[4] = parts[4] * 3.0
    return np.concatenate(parts).astype(f32)


def make_case(i):
    batch, n_envs, slots, seed = SHAPES[i]
    rng = np.random.default_rng(seed)
    params, target_params = default_init(rng), default_init(rng)
    total = slots * n_envs
    obs = (rng.uniform(-1, 1, (slots, n_envs, 4)) * np.array([2.4, 3.0, 0.21, 3.0])).astype(f32)
    actions = rng.integers(0, 2, (slots, n_envs)).astype(np.int64)
    rewards = REWARDS[rng.integers(0, len(REWARDS), (slots, n_envs))]
    term = (rng.random((slots, n_envs)) < 0.15).astype(np.uint8)
    idx = rng.integers(0, total, batch).astype(np.int64)
    if batch >= 5:
        idx[0] = total - 1                      # last slot, last env: the successor wraps to slot 0
        idx[1] = (slots - 1) * n_envs           # last slot, env 0
        idx[2] = 0
    nxt = (idx + n_envs) % total
    fo, fa, fr, ft = obs.reshape(total, 4), actions.reshape(total), rewards.reshape(total), term.reshape(total)
    Xb, A, Xn, Rw, Tm = fo[idx], fa[idx], fo[nxt], fr[nxt], ft[nxt]
    na, m, q = X.target(target_params, Xn, Rw, Tm, dtype=np.float64)
    loss, grad, probs = X.loss_grad(params, Xb, A, m, dtype=np.float64)
    _p, _q, z1, z2 = X.forward64(params, Xb)
    _p, _q, t1, t2 = X.forward64(target_params, Xn)
    kink = (np.abs(z1) <= NEAR_ZERO).any(1) | (np.abs(z2) <= NEAR_ZERO).any(1) | (np.abs(t1) <= NEAR_ZERO).any(1) | (np.abs(t2) <= NEAR_ZERO).any(1)
    _m32, li, ui, b = X.project(np.full((batch, 101), f32(1 / 101)), Rw, Tm)
    tz_raw = Rw.astype(np.float64)[:, None] + float(f32(0.99)) * X.ATOMS.astype(np.float64)[None, :] * (1 - Tm[:, None])
    return dict(batch=batch, n_envs=n_envs, slots=slots, params=params, target_params=target_params, obs=obs, actions=actions, rewards=rewards, term=term, idx=idx,
                wraps=int((idx + n_envs >= total).sum()), next_actions=na, target_probs=m, q=q, close=np.abs(q[:, 0] - q[:, 1]) < X.CLOSE_Q, loss=float(loss), grad=grad,
                probs=probs, kink=kink, clamped_low=int((tz_raw < -100).sum()), clamped_high=int((tz_raw > 100).sum()), integral=int((li == ui).sum()),
                fractional=int((li != ui).sum()), terminated_rows=int(Tm.sum()), b=b)
