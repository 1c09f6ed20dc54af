"""The drop-in script ``python -m deep_rl_amd.qrdqn``: its lines, names, shapes, dtypes and constants at one env, the default run's shape, a finite run on a
4,096-env ring — and whether the PRODUCTION random path (keyed reset noise, exploration and minibatch draws) learns like the plain torch script that stands in for
the missing reference (tools/capture_qrdqn_ref.py): seeds 1..32 against tests/golden/qrdqn_learning_stats.npz under the criterion of tests/test_gpu_learning.py
(its ``last_tenth``, ``tost_welch`` and ``MARGIN``, the same three asserts as its ``_compare``).  Statistic: mean return of the last tenth of a run's episodes
(torch script: mean 109.9 over the 32 seeds, seed-to-seed sd 26.0)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _c51_ref import results_dir
from test_gpu_learning import MARGIN, last_tenth, tost_welch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SEED", "NUM_ENVS", "TOTAL_TIMESTEPS", "MEMORY_SIZE", "BATCH_SIZE", "LEARNING_STARTS", "PRINT_EPISODES", "MIRL_QR_SO")


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
    g = runpy.run_module('deep_rl_amd.qrdqn', run_name='__main__')
out = {k: (list(g[k].shape) if torch.is_tensor(g[k]) else g[k]) for k in ('observations', 'actions', 'rewards', 'terminated', 'observation', 'batch_inds', 'target_quantiles', 'current',
       'next_actions', 'taus', 'global_step', 'total_timesteps', 'learning_starts', 'train_frequency', 'target_network_frequency', 'batch_size', 'gamma', 'learning_rate',
       'n_quantiles', 'kappa', 'env_id', 'seed', 'start_e', 'end_e', 'exploration_fraction', 'slope', 'memory_size', 'loss')}
out['dtypes'] = [str(g[k].dtype) for k in ('observations', 'actions', 'rewards', 'terminated')]
out['adam_eps'] = g['optimizer'].param_groups[0]['eps']
out['updates'] = g['engine'].update_index
out['finite'] = bool(torch.isfinite(g['q_network'].flat).all())
out['synced'] = bool((g['q_network'].flat == g['target_network'].flat).all())
out['taus_ok'] = bool((g['taus'] == (2 * torch.arange(64, dtype=torch.float32) + 1) / 128).all()) and g['taus'].dtype == torch.float32
out['next_actions_dtype'] = str(g['next_actions'].dtype)
out['names'] = sorted(k for k in ('env', 'q_network', 'target_network', 'optimizer', 'epsilon') if k in g)
out['lines'] = buf.getvalue().splitlines()
print('SCRIPT_JSON ' + json.dumps(out))
"""


def _run_globals(**kw):
    p = subprocess.run([sys.executable, "-c", _GLOBALS], env=_env(**kw), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SCRIPT_JSON ")][0][len("SCRIPT_JSON "):])


def test_script_at_one_env_has_its_lines_names_shapes_and_constants():
    g = _run_globals(NUM_ENVS=1, TOTAL_TIMESTEPS=4000)
    assert g["observations"] == [4001, 4] and g["actions"] == [4001] and g["rewards"] == [4001] and g["terminated"] == [4001] and g["observation"] == [4]
    assert g["dtypes"] == ["torch.float32", "torch.int64", "torch.float32", "torch.bool"]
    assert g["batch_inds"] == [128] and g["target_quantiles"] == [128, 64] and g["current"] == [128, 64] and g["next_actions"] == [128] and g["next_actions_dtype"] == "torch.int32"
    assert g["taus"] == [64] and g["taus_ok"] and (g["n_quantiles"], g["kappa"]) == (64, 1.0)
    assert g["global_step"] == g["total_timesteps"] == 4000 and g["learning_starts"] == 2000 and g["memory_size"] == 4001
    assert (g["train_frequency"], g["target_network_frequency"], g["batch_size"], g["gamma"], g["learning_rate"]) == (10, 500, 128, 0.99, 2.5e-4)
    assert (g["env_id"], g["seed"]) == ("CartPole-v1", 1)
    assert (g["start_e"], g["end_e"], g["exploration_fraction"]) == (1, 0.05, 0.5) and g["slope"] == (0.05 - 1) / (0.5 * 4000) and g["adam_eps"] == 0.01 / 128
    assert g["updates"] == 201 and g["finite"] and g["synced"] and np.isfinite(g["loss"]) and g["loss"] > 0       # updates at 2,000, 2,010 ... 4,000; the sync at 4,000
    assert {"env", "optimizer", "q_network", "target_network"} <= set(g["names"])
    lines = g["lines"]
    assert len(lines) > 50 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.0", ln) for ln in lines), lines[:3]     # no format spec: 22.0
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    rets = [float(ln.split("episodic_return=")[1]) for ln in lines]
    assert steps == np.cumsum(rets).astype(int).tolist()      # every env step belongs to one episode; CartPole's return is its length


def test_script_default_run_has_the_torch_scripts_shape():
    p = subprocess.run([sys.executable, "-m", "deep_rl_amd.qrdqn"], env=_env(), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    assert 500 < len(lines) < 3000 and 49_000 < steps[-1] <= 50_000      # 50,000 steps; the torch script's 32 runs print 1,251 .. 1,949 episodes


def test_script_on_a_4096_env_ring_stays_finite():
    g = _run_globals(NUM_ENVS=4096, TOTAL_TIMESTEPS=600, MEMORY_SIZE=256, LEARNING_STARTS=100)
    assert g["observations"] == [256, 4096, 4] and g["actions"] == [256, 4096] and g["global_step"] == 600
    assert g["updates"] == 51 and g["finite"] and np.isfinite(g["loss"]) and g["lines"] == []


_CODE = r"""
import contextlib, io, json, os, runpy, sys
seeds = [int(s) for s in sys.argv[1].split(',')]
out = {}
for s in seeds:
    os.environ.update(SEED=str(s), NUM_ENVS='1')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_module('deep_rl_amd.qrdqn', run_name='__main__')
    out[s] = [float(ln.split('episodic_return=')[1]) for ln in buf.getvalue().splitlines() if ln.startswith('global_step=')]
print('LEARNING_JSON ' + json.dumps(out))
"""
WORKERS = 8


def test_production_rng_path_learns_like_the_torch_script():
    from scipy.stats import mannwhitneyu, t as student

    g = np.load(os.path.join(ROOT, "tests", "golden", "qrdqn_learning_stats.npz"))
    SEEDS = g["qrdqn_seeds"].tolist()
    assert SEEDS == list(range(1, 33))
    ref = g["qrdqn_last_tenth_mean"].astype(np.float64)
    off, rets = g["qrdqn_offsets"], g["qrdqn_episode_return"]
    assert np.allclose([last_tenth(rets[off[i]:off[i + 1]]) for i in range(32)], ref)
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
    assert sorted(runs) == SEEDS and all(len(runs[s]) > 100 and np.isfinite(runs[s]).all() for s in SEEDS)
    ours = np.array([last_tenth(runs[s]) for s in SEEDS])
    p = float(mannwhitneyu(ours, ref, alternative="two-sided").pvalue)
    se = float(np.sqrt(ours.var(ddof=1) / len(ours) + ref.var(ddof=1) / len(ref)))
    s_ref = float(ref.std(ddof=1))
    p_tost, dof = tost_welch(ours, ref, MARGIN * s_ref)
    half = float(student.ppf(0.95, dof)) * se
    rec = {"script": "qrdqn", "seeds": [SEEDS[0], SEEDS[-1]], "statistic": "mean episodic return of the last tenth of the episodes of a run",
           "ours_gpu": [round(x, 2) for x in ours.tolist()], "ours_mean": round(float(ours.mean()), 2), "reference_mean": round(float(ref.mean()), 2), "pooled_se": round(se, 2),
           "mean_difference_in_se": round(float(ours.mean() - ref.mean()) / se, 3), "mannwhitney_p": round(p, 4),
           "reference_seed_sd": round(s_ref, 2), "ours_seed_sd": round(float(ours.std(ddof=1)), 2), "mean_difference_in_reference_sd": round(float(ours.mean() - ref.mean()) / s_ref, 3),
           "equivalence": {"test": "TOST, two one-sided Welch t-tests", "margin_in_reference_sd": MARGIN, "margin": round(MARGIN * s_ref, 2), "p": float("%.3g" % p_tost), "dof": round(dof, 1),
                           "alpha": 0.05, "ci90_of_difference": [round(float(ours.mean() - ref.mean()) + sgn * half, 2) for sgn in (-1, 1)]}}
    path = os.path.join(results_dir(), "learning_stats_gpu.json")      # under the key "qrdqn", beside the other scripts' records
    allrec = json.load(open(path)) if os.path.exists(path) else {}
    allrec["qrdqn"] = rec
    json.dump(allrec, open(path, "w"), indent=1)
    print(json.dumps(rec))
    assert p > 0.01, rec
    assert abs(ours.mean() - ref.mean()) <= 2.0 * se, rec
    assert p_tost < 0.05, rec
