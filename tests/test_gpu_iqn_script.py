"""The drop-in script ``python -m deep_rl_amd.iqn``: the reference's lines, names and shapes at one env, a finite run on a 4,096-env ring — and whether the
PRODUCTION random path (keyed reset noise, exploration, minibatch and tau draws) learns like the reference's statements on the CPU: seeds 1..50 against
tests/golden/iqn_learning_stats.npz (tools/capture_iqn_ref.py --learning) under the criterion of tests/test_gpu_learning.py (its ``last_tenth``, ``tost_welch``
and ``MARGIN``, the three asserts of tests/test_gpu_c51_script.py).  Statistic: mean return of the last tenth of a run's episodes."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _iqn_ref import results_dir
from test_gpu_learning import MARGIN, last_tenth, tost_welch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SEED", "NUM_ENVS", "TOTAL_TIMESTEPS", "MEMORY_SIZE", "BATCH_SIZE", "LEARNING_STARTS", "PRINT_EPISODES", "MIRL_IQN_SO")


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
    g = runpy.run_module('deep_rl_amd.iqn', run_name='__main__')
out = {k: (list(g[k].shape) if torch.is_tensor(g[k]) else g[k]) for k in ('observations', 'actions', 'rewards', 'terminated', 'observation', 'batch_inds', 'taus',
       'current_action_quantiles', 'target_action_quantiles', 'next_actions', 'global_step', 'total_timesteps', 'learning_starts', 'train_frequency',
       'target_network_frequency', 'batch_size', 'gamma', 'learning_rate', 'final_epsilon', 'epsilon_decay_steps', 'slope', 'num_tau_samples', 'num_tau_prime_samples',
       'num_quantile_samples', 'num_cosines', 'embedding_dim', 'kappa', 'env_id', 'seed', 'memory_size', 'quantile_loss', 'epsilon')}
out['dtypes'] = [str(g[k].dtype) for k in ('observations', 'actions', 'rewards', 'terminated')]
out['adam_eps'] = g['optimizer'].param_groups[0]['eps']
out['updates'] = g['engine'].update_index
out['finite'] = bool(torch.isfinite(g['online_params']).all())
out['synced'] = bool((g['online_params'] == g['target_params']).all())
out['views'] = all(p.data_ptr() >= g['online_params'].data_ptr() and p.data_ptr() < g['online_params'].data_ptr() + 4 * 44898 for p in g['parameters'])
out['nparams'] = sum(p.numel() for p in g['parameters'])
out['names'] = sorted(k for k in ('env', 'online_features_extractor', 'online_cosine_net', 'online_quantile_net', 'target_features_extractor', 'target_cosine_net',
                                  'target_quantile_net', 'optimizer', 'parameters') if k in g)
out['lines'] = buf.getvalue().splitlines()
print('SCRIPT_JSON ' + json.dumps(out))
"""


def _run_globals(**kw):
    p = subprocess.run([sys.executable, "-c", _GLOBALS], env=_env(**kw), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SCRIPT_JSON ")][0][len("SCRIPT_JSON "):])


def test_script_at_one_env_has_the_references_lines_names_and_shapes():
    g = _run_globals(NUM_ENVS=1, TOTAL_TIMESTEPS=3000)
    assert g["observations"] == [3001, 4] and g["actions"] == [3001] and g["rewards"] == [3001] and g["terminated"] == [3001] and g["observation"] == [4]   # iqn.py:174-177
    assert g["dtypes"] == ["torch.float32", "torch.int64", "torch.float32", "torch.bool"]
    assert g["batch_inds"] == [32] and g["taus"] == [32, 64] and g["current_action_quantiles"] == [32, 64] and g["target_action_quantiles"] == [32, 64] and g["next_actions"] == [32]
    assert g["global_step"] == g["total_timesteps"] == 3000 and g["learning_starts"] == 1000 and g["memory_size"] == 3001
    assert (g["train_frequency"], g["target_network_frequency"], g["batch_size"], g["gamma"], g["learning_rate"]) == (4, 500, 32, 0.99, 5e-5)
    assert (g["num_tau_samples"], g["num_tau_prime_samples"], g["num_quantile_samples"], g["num_cosines"], g["embedding_dim"], g["kappa"]) == (64, 64, 32, 64, 64, 1.0)
    assert (g["final_epsilon"], g["epsilon_decay_steps"], g["env_id"], g["seed"]) == (0.01, 10_000, "CartPole-v1", 0) and g["slope"] == -(1.0 - 0.01) / 10_000
    assert g["adam_eps"] == 1e-2 / 32 and g["epsilon"] == max(1.0 + g["slope"] * 2999, 0.01)
    assert g["updates"] == 501 and g["finite"] and g["synced"] and np.isfinite(g["quantile_loss"]) and g["quantile_loss"] > 0   # updates at 1,000, 1,004 ... 3,000; the sync at 3,000
    assert len(g["names"]) == 9 and g["views"] and g["nparams"] == 44_898
    lines = g["lines"]
    assert len(lines) > 50 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in lines), lines[:3]     # :220 prints with :.2f
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    rets = [float(ln.split("episodic_return=")[1]) for ln in lines]
    assert steps == np.cumsum(rets).astype(int).tolist()      # every env step belongs to one episode; CartPole's return is its length


def test_script_on_a_4096_env_ring_stays_finite():
    g = _run_globals(NUM_ENVS=4096, TOTAL_TIMESTEPS=400, MEMORY_SIZE=128, LEARNING_STARTS=100)
    assert g["observations"] == [128, 4096, 4] and g["actions"] == [128, 4096] and g["global_step"] == 400
    assert g["updates"] == 76 and g["finite"] and np.isfinite(g["quantile_loss"]) and g["lines"] == []


_CODE = r"""
import contextlib, io, json, os, runpy, sys
seeds = [int(s) for s in sys.argv[1].split(',')]
out = {}
for s in seeds:
    os.environ.update(SEED=str(s), NUM_ENVS='1')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_module('deep_rl_amd.iqn', run_name='__main__')
    out[s] = [float(ln.split('episodic_return=')[1]) for ln in buf.getvalue().splitlines() if ln.startswith('global_step=')]
print('LEARNING_JSON ' + json.dumps(out))
"""
WORKERS = 10


def test_production_rng_path_learns_like_the_reference():
    from scipy.stats import mannwhitneyu, t as student

    g = np.load(os.path.join(ROOT, "tests", "golden", "iqn_learning_stats.npz"))
    SEEDS = g["iqn_seeds"].tolist()
    assert SEEDS == list(range(1, 51))
    ref = g["iqn_last_tenth_mean"].astype(np.float64)
    off, rets = g["iqn_offsets"], g["iqn_episode_return"]
    assert np.allclose([last_tenth(rets[off[i]:off[i + 1]]) for i in range(50)], ref)
    procs = [subprocess.Popen([sys.executable, "-c", _CODE, ",".join(map(str, SEEDS[w::WORKERS]))], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for w in range(WORKERS)]
    runs = {}
    for pr in procs:
        try:
            so, se = pr.communicate(timeout=900)
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
    rec = {"script": "iqn", "seeds": [SEEDS[0], SEEDS[-1]], "statistic": "mean episodic return of the last tenth of the episodes of a run",
           "ours_gpu": [round(x, 2) for x in ours.tolist()], "ours_mean": round(float(ours.mean()), 2), "reference_mean": round(float(ref.mean()), 2), "pooled_se": round(se, 2),
           "mean_difference_in_se": round(float(ours.mean() - ref.mean()) / se, 3), "mannwhitney_p": round(p, 4),
           "reference_seed_sd": round(s_ref, 2), "ours_seed_sd": round(float(ours.std(ddof=1)), 2), "mean_difference_in_reference_sd": round(float(ours.mean() - ref.mean()) / s_ref, 3),
           "equivalence": {"test": "TOST, two one-sided Welch t-tests", "margin_in_reference_sd": MARGIN, "margin": round(MARGIN * s_ref, 2), "p": float("%.3g" % p_tost), "dof": round(dof, 1),
                           "alpha": 0.05, "ci90_of_difference": [round(float(ours.mean() - ref.mean()) + sgn * half, 2) for sgn in (-1, 1)]}}
    path = os.path.join(results_dir(), "learning_stats_gpu.json")      # under the key "iqn", beside the other scripts' records
    allrec = json.load(open(path)) if os.path.exists(path) else {}
    allrec["iqn"] = rec
    json.dump(allrec, open(path, "w"), indent=1)
    print(json.dumps(rec))
    assert p > 0.01, rec
    assert abs(ours.mean() - ref.mean()) <= 2.0 * se, rec
    assert p_tost < 0.05, rec
