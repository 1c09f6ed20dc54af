"""Synthetic QR-DQN cases — TEST INFRASTRUCTURE: rings, batches and parameters that reach what the torch script's run never does (include/mi_qr.h).

The run has one env, rewards of 1 and a batch of 128.  These cases add: terminated rows, rows whose successor wraps around the ring's end (down to slots = 2), 1 and 3
envs, batches of 1 row, of 5, of 129 (more rows than the gradient launch has workgroups, 128: a workgroup then walks two rows) and of 300, and rewards that put the
pairwise differences u on both sides of kappa and of 0 in every case.  Parameters are drawn at torch's default-init scale and observations inside CartPole's range,
so the figures the device bounds come from (tests/_qrdqn_ref.py) describe these cases too; the expected values are float64.
A ReLU pre-activation within NEAR_ZERO of 0 may land on either side of the kink in another evaluation order: the cases are chosen (by their seeds) so that at most
KINK_SHARE of a case's rows have one, and at most MAX_EXCLUDED have action values closer than CLOSE_Q — in float64 alone.  No row is excluded from a gradient comparison.
"""
import numpy as np

import _qrdqn_ref as X
from _c51_cases import KINK_SHARE, NEAR_ZERO

f32 = np.float32
#        (batch, n_envs, slots, seed)
SHAPES = ((1, 1, 2, 1), (5, 3, 7, 3), (129, 1, 80, 3), (300, 3, 100, 3), (128, 1, 300, 3))
REWARDS = np.array([1.0, -3.0, 5.0, 0.5, 0.0], f32)


def default_init(rng):
    """a flat parameter vector at torch's default nn.Linear scale: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))"""
    parts = []
    for fan_in, n in ((4, 480), (4, 120), (120, 10080), (120, 84), (84, 10752), (84, 128)):
        k = 1.0 / np.sqrt(fan_in)
        parts.append(rng.uniform(-k, k, n))
    parts[4] = parts[4] * 3.0   # a trained head is far from uniform: spread the last layer so that the quantiles differ by more than kappa and the action values differ
    return np.concatenate(parts).astype(f32)


def make_case(i, seed=None):
    batch, n_envs, slots, seed0 = SHAPES[i]
    rng = np.random.default_rng(seed0 if seed is None else seed)
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
    elif slots == 2:
        idx[0] = total - 1
    nxt = (idx + n_envs) % total
    fo, fa, fr, ft = obs.reshape(total, 4), actions.reshape(total), rewards.reshape(total), term.reshape(total)
    if batch >= 5 and not ft[nxt].any():
        ft[nxt[3]] = 1                          # every batch of several rows holds a terminated one
    Xb, A, Xn, Rw, Tm = fo[idx], fa[idx], fo[nxt], fr[nxt], ft[nxt]
    na, tgt, q = X.target(target_params, Xn, Rw, Tm, dtype=np.float64)
    loss, grad, cur = X.loss_grad(params, Xb, A, tgt, dtype=np.float64)
    _th, q_on, z1, z2 = X.forward64(params, Xb)
    _th, _q, t1, t2 = X.forward64(target_params, Xn)
    kink = (np.abs(z1) <= NEAR_ZERO).any(1) | (np.abs(z2) <= NEAR_ZERO).any(1) | (np.abs(t1) <= NEAR_ZERO).any(1) | (np.abs(t2) <= NEAR_ZERO).any(1)
    u = tgt[:, None, :] - cur[:, :, None]
    return dict(batch=batch, n_envs=n_envs, slots=slots, params=params, target_params=target_params, obs=obs, actions=actions, rewards=rewards, term=term, idx=idx,
                wraps=int((idx + n_envs >= total).sum()), next_actions=na, target=tgt, q=q, close=np.abs(q[:, 0] - q[:, 1]) < X.CLOSE_Q, loss=float(loss), grad=grad,
                current=cur, kink=kink, terminated_rows=int(Tm.sum()), quadratic=int((np.abs(u) <= 1).sum()), linear=int((np.abs(u) > 1).sum()),
                negative=int((u < 0).sum()), non_negative=int((u >= 0).sum()), u_min_abs=float(np.abs(u).min()))


def holds(c):
    """what tests/test_qrdqn_cases_cpu.py asks of a case (used to choose the seeds)"""
    ok = min(c["quadratic"], c["linear"], c["negative"], c["non_negative"]) > 0
    ok &= int(c["kink"].sum()) <= KINK_SHARE * c["batch"] and int(c["close"].sum()) <= X.MAX_EXCLUDED * c["batch"]
    ok &= c["batch"] < 5 or (len(set(c["next_actions"].tolist())) == 2 and c["terminated_rows"] > 0 and c["wraps"] >= 2)
    return bool(ok)
