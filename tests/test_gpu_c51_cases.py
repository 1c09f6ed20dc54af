"""The C51 kernels on the synthetic cases of tests/_c51_cases.py (validated on the CPU by tests/test_c51_cases_cpu.py) against float64: the clamp at both ends,
fractional and integral b, terminated rows, successors across the ring's end, several envs, and batches of 1, 5, 129 and 300 rows — the last two walk several
rows per workgroup.  Bounds: those of tests/_c51_ref.py (8 x the f32 restatement's measured distance from the reference); nothing is excluded from a gradient
comparison, action comparisons leave out the rows with close action values (none in these cases, by their seeds)."""
import numpy as np
import pytest

import _c51_cases as K
import _c51_ref as X
from test_gpu_c51 import _make, _np, _record

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(K.SHAPES)))
def test_update_on_a_synthetic_case_against_float64(i):
    import torch
    c = K.make_case(i)
    eng = _make(n=c["n_envs"], slots=c["slots"], batch_size=c["batch"], params=c["params"], target=c["target_params"])
    eng.observations.copy_(torch.from_numpy(c["obs"])); eng.actions.copy_(torch.from_numpy(c["actions"]))
    eng.rewards.copy_(torch.from_numpy(c["rewards"])); eng.terminated.copy_(torch.from_numpy(c["term"]))
    eng.global_step = c["slots"]
    eng.sample(c["idx"])
    eng.grad()
    na, tp, pr, g, loss = _np(eng.next_actions), _np(eng.target_probs), _np(eng.probs), _np(eng.grads), float(eng.loss.item())
    far = ~c["close"]
    assert np.array_equal(na[far], c["next_actions"][far])
    same = na == c["next_actions"]
    fig = {"batch": c["batch"], "target_probs": float(np.abs(tp - c["target_probs"])[same].max()), "probs": float(np.abs(pr - c["probs"]).max()),
           "loss": abs(loss - c["loss"]) / abs(c["loss"]), "grad": float(np.abs(g - c["grad"]).max() / np.abs(c["grad"]).max()), "actions_differ": int((~same).sum())}
    _record("case_%d" % i, fig)
    assert fig["target_probs"] <= X.BOUND_TARGET_PROBS_ABS and fig["probs"] <= X.BOUND_PROBS_ABS
    assert fig["loss"] <= X.BOUND_LOSS_REL and fig["grad"] <= X.BOUND_GRAD_REL
    # the fused call on the same batch steps the parameters by Adam on exactly this gradient
    p0 = c["params"].copy(); m = np.zeros_like(p0); v = np.zeros_like(p0)
    X.adam_step(p0, g, m, v, 1)
    eng.train_step(c["idx"])
    assert np.array_equal(_np(eng.grads), g) and np.abs(_np(eng.q.flat) - p0).max() <= 1e-6


def _episode_figures(term):
    """(steps,) terminated flags of one env that started a fresh episode at step 0 -> (finished episodes, sum of their lengths, longest)"""
    ends = np.flatnonzero(term)
    lens = np.diff(np.concatenate([[-1], ends]))
    return len(ends), int(lens.sum()), int(lens.max()) if len(ends) else 0


def test_acting_at_4096_envs_matches_single_env_engines():
    """the scaled acting size: 4,096 envs share 1,024 workgroups (each walks four envs); spot-checked envs act exactly as N = 1 engines keyed with their ids, and the
    launch's episode statistics (accumulated by integer atomics from 1,024 workgroups) are the sums over the envs of what the ring itself shows — which, for the
    spot-checked envs, is what their single-env engines report.  32 steps from fresh episodes: no TimeLimit truncation, so every finished episode is a terminated one"""
    p = X.load_ckpt(1000)["params_before"]
    S, T, g0 = 34, 32, 5_260
    kw = dict(slots=S, params=p, total_timesteps=20_000)
    big = _make(n=4096, **kw)
    big.global_step = g0
    big.reset()
    big.act(T)
    A, O, Tm = _np(big.actions), _np(big.observations), _np(big.terminated)
    term = Tm[(g0 + 1 + np.arange(T)) % S]                  # step s's flag lies in slot (g0 + s + 1) % slots
    per_env = np.array([_episode_figures(term[:, E]) for E in range(4096)])
    for E in (0, 1023, 1024, 4095):
        one = _make(n=1, env_id_base=E, **kw)
        one.global_step = g0
        one.reset()
        one.act(T)
        assert np.array_equal(_np(one.actions)[:, 0], A[:, E]) and np.array_equal(_np(one.observations)[:, 0], O[:, E])
        assert _np(one.episode_stats)[:3].tolist() == per_env[E].tolist()
    st = _np(big.episode_stats).tolist()
    assert per_env[:, 0].sum() >= 400                      # the case has episodes to count: at least a tenth of the envs finish one within 32 steps
    assert st[:3] == [int(per_env[:, 0].sum()), int(per_env[:, 1].sum()), int(per_env[:, 2].max())] and st[3] == 0   # (no episode log at this size: no slots handed out)
    assert big.global_step == g0 + T
