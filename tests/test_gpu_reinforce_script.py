"""The drop-in script ``python -m deep_rl_amd.reinforce``: the reference's lines, names and shapes at one env, a finite run at 4,096 envs — and whether the
PRODUCTION random path (keyed reset noise, action draws and dropout masks) learns like the unmodified reference: 50 seeds against
tests/golden/reinforce_learning_stats.npz under the criterion of tests/test_gpu_learning.py (its ``last_tenth``, ``tost_welch`` and ``MARGIN = 0.75``, the same
three asserts as its ``_compare``).  Statistic: mean return of the last tenth = the last 10 of the 100 episodes of a run.

The criterion against itself: 100 runs of the unmodified reference (seeds 1..100) split 51..100 vs 1..50 differ by -0.25 sd (-1.32 se), Mann-Whitney p 0.25, TOST
p 0.0044, and 93.5 % of 2,000 random 50 / 50 splits pass all three asserts; the seeds are fixed and the run deterministic, so a pass stays a pass."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _reinforce_ref import results_dir
from test_gpu_learning import MARGIN, last_tenth, tost_welch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SEED", "NUM_ENVS", "NUM_EPISODES", "PRINT_EPISODES", "MIRL_PG_SO")


def _env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in KNOBS:
        env.pop(k, None)
    env.update({k: str(v) for k, v in kw.items()})
    return env


_GLOBALS = r"""
import contextlib, io, json, runpy, sys, torch
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    g = runpy.run_module('deep_rl_amd.reinforce', run_name='__main__')
out = {k: (list(g[k].shape) if torch.is_tensor(g[k]) else g[k]) for k in ('log_probs', 'returns', 'b_returns', 'b_log_probs', 'policy_loss', 'global_step', 'gamma', 'env_id', 'seed',
                                                                          'episode_idx', 'LOG_STD_MIN')}
out['step'] = g['step'] if isinstance(g['step'], int) else list(g['step'].shape)
out['finite'] = bool(torch.isfinite(g['agent'].flat).all()) and bool(torch.isfinite(g['policy_loss']))
out['names'] = sorted(k for k in ('env', 'agent', 'optimizer', 'observation', 'done') if k in g)
out['lines'] = buf.getvalue().splitlines()
print('SCRIPT_JSON ' + json.dumps(out))
"""


def _run_globals(**kw):
    p = subprocess.run([sys.executable, "-c", _GLOBALS], env=_env(**kw), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SCRIPT_JSON ")][0][len("SCRIPT_JSON "):])


def test_script_at_one_env_prints_the_references_lines():
    p = subprocess.run([sys.executable, "-m", "deep_rl_amd.reinforce"], env=_env(NUM_ENVS=1), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 100 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in lines), lines[:3]
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    rets = [float(ln.split("episodic_return=")[1]) for ln in lines]
    assert steps == np.cumsum(rets).astype(int).tolist()      # reinforce.py:66,69: global_step counts every env step, the return of CartPole is the length


def test_script_globals_have_the_references_names_and_shapes():
    g = _run_globals(NUM_ENVS=1)
    assert g["log_probs"] == [501] and g["returns"] == [501]                       # reinforce.py:53-54
    assert isinstance(g["step"], int) and g["b_returns"] == [g["step"]] == g["b_log_probs"] and g["policy_loss"] == []
    assert g["gamma"] == 0.99 and g["env_id"] == "CartPole-v1" and g["seed"] == 1 and g["episode_idx"] == 99 and g["LOG_STD_MIN"] == -5
    assert {"agent", "done", "env", "optimizer"} <= set(g["names"])
    assert g["finite"] and len(g["lines"]) == 100


def test_script_at_4096_envs_stays_finite():
    g = _run_globals(NUM_ENVS=4096, NUM_EPISODES=3)
    assert g["finite"] and g["log_probs"] == [4096, 501]
    assert len(g["lines"]) == 3 and all(re.fullmatch(r"update=\d+, global_step=\d+, episodes=4096, mean_episodic_return=\d+\.\d\d", ln) for ln in g["lines"]), g["lines"]


_CODE = r"""
import contextlib, io, json, os, runpy, sys
seeds = [int(s) for s in sys.argv[1].split(',')]
out = {}
for s in seeds:
    os.environ.update(SEED=str(s), NUM_ENVS='1')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_module('deep_rl_amd.reinforce', run_name='__main__')
    out[s] = [float(ln.split('episodic_return=')[1]) for ln in buf.getvalue().splitlines() if ln.startswith('global_step=')]
print('LEARNING_JSON ' + json.dumps(out))
"""
WORKERS = 5


def test_production_rng_path_learns_like_the_reference():
    from scipy.stats import mannwhitneyu, t as student

    g = np.load(os.path.join(ROOT, "tests", "golden", "reinforce_learning_stats.npz"))
    SEEDS = g["reinforce_seeds"].tolist()
    assert SEEDS == list(range(1, 51))
    ref = g["reinforce_last_tenth_mean"].astype(np.float64)
    off, rets = g["reinforce_offsets"], g["reinforce_episode_return"]
    assert np.all(np.diff(off) == 100) and np.allclose([last_tenth(rets[off[i]:off[i + 1]]) for i in range(50)], ref)
    procs = [subprocess.Popen([sys.executable, "-c", _CODE, ",".join(map(str, SEEDS[w::WORKERS]))], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for w in range(WORKERS)]
    runs = {}
    for pr in procs:
        try:
            so, se = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert pr.returncode == 0, se[-3000:]
        line = [ln for ln in so.splitlines() if ln.startswith("LEARNING_JSON ")][0]
        runs.update({int(k): v for k, v in json.loads(line[len("LEARNING_JSON "):]).items()})
    assert sorted(runs) == SEEDS and all(len(runs[s]) == 100 and np.isfinite(runs[s]).all() for s in SEEDS)
    ours = np.array([last_tenth(runs[s]) for s in SEEDS])
    p = float(mannwhitneyu(ours, ref, alternative="two-sided").pvalue)
    se = float(np.sqrt(ours.var(ddof=1) / len(ours) + ref.var(ddof=1) / len(ref)))
    s_ref = float(ref.std(ddof=1))
    p_tost, dof = tost_welch(ours, ref, MARGIN * s_ref)
    half = float(student.ppf(0.95, dof)) * se
    rec = {"script": "reinforce", "seeds": SEEDS, "statistic": "mean episodic return of the last tenth (10) of the 100 episodes of a run",
           "ours_gpu": [round(x, 2) for x in ours.tolist()], "reference_cpu": [round(x, 2) for x in ref.tolist()],
           "ours_mean": round(float(ours.mean()), 2), "reference_mean": round(float(ref.mean()), 2), "pooled_se": round(se, 2),
           "mean_difference_in_se": round(float(ours.mean() - ref.mean()) / se, 3), "mannwhitney_p": round(p, 4),
           "reference_seed_sd": round(s_ref, 2), "ours_seed_sd": round(float(ours.std(ddof=1)), 2), "mean_difference_in_reference_sd": round(float(ours.mean() - ref.mean()) / s_ref, 3),
           "shortest_episode_ours": int(min(min(runs[s]) for s in SEEDS)),
           "equivalence": {"test": "TOST, two one-sided Welch t-tests", "margin_in_reference_sd": MARGIN, "margin": round(MARGIN * s_ref, 2), "p": float("%.3g" % p_tost), "dof": round(dof, 1),
                           "alpha": 0.05, "ci90_of_difference": [round(float(ours.mean() - ref.mean()) + sgn * half, 2) for sgn in (-1, 1)]}}
    path = os.path.join(results_dir(), "learning_stats_gpu.json")      # under the key "reinforce", beside the other scripts' records
    allrec = json.load(open(path)) if os.path.exists(path) else {}
    allrec["reinforce"] = rec
    json.dump(allrec, open(path, "w"), indent=1)
    print(json.dumps(rec))
    assert p > 0.01, rec
    assert abs(ours.mean() - ref.mean()) <= 2.0 * se, rec
    assert p_tost < 0.05, rec
