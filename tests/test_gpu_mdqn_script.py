"""The drop-in script ``python -m deep_rl_amd.munchausen_dqn``: its lines, names, shapes, dtypes, constants and knobs at one env, a finite run on a 64-env ring that
wraps — and whether the PRODUCTION random path (keyed reset noise, exploration and minibatch draws) learns like the plain torch script that stands in for the missing
reference (tools/capture_mdqn_ref.py): seeds 1 .. 6 at the full 100,000 steps against tests/golden/mdqn_learning_stats.npz (the last-tenth mean return of the torch
script's seeds 1 .. 24).  One-sided: the mean of the six must be >= the fixture's mean - 3 x the fixture's seed-to-seed sd / sqrt(6).  At most six child
processes at once, each under its own timeout."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _c51_ref import results_dir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SEED", "NUM_ENVS", "TOTAL_TIMESTEPS", "MEMORY_SIZE", "BATCH_SIZE", "LEARNING_STARTS", "PRINT_EPISODES", "MIRL_DDQN_SO", "MIRL_MDQN_SO", "ALPHA", "TAU", "CLIP_LO")


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
    g = runpy.run_module('deep_rl_amd.munchausen_dqn', run_name='__main__')
out = {k: (list(g[k].shape) if torch.is_tensor(g[k]) else g[k]) for k in ('observations', 'actions', 'rewards', 'terminated', 'observation', 'batch_inds', 'target_values', 'current',
       'next_actions', 'global_step', 'total_timesteps', 'learning_starts', 'train_frequency', 'target_network_frequency', 'batch_size', 'gamma', 'learning_rate',
       'env_id', 'seed', 'start_e', 'end_e', 'exploration_fraction', 'slope', 'memory_size', 'loss', 'bonus', 'soft_value', 'alpha', 'tau', 'clip_lo')}
out['engine_knobs'] = [g['engine'].alpha, g['engine'].tau, g['engine'].clip_lo]
out['bonus_range'] = [float(g['bonus'].min()), float(g['bonus'].max())]
out['soft_finite'] = bool(torch.isfinite(g['soft_value']).all())
out['dtypes'] = [str(g[k].dtype) for k in ('observations', 'actions', 'rewards', 'terminated')]
out['adam_eps'] = g['optimizer'].param_groups[0]['eps']
out['updates'] = g['engine'].update_index
out['engine'] = type(g['engine']).__name__
out['nets'] = [type(g['q_network']).__name__, type(g['target_network']).__name__]
out['finite'] = bool(torch.isfinite(g['q_network'].flat).all()) and bool(torch.isfinite(g['engine'].observations).all())
out['synced'] = bool((g['q_network'].flat == g['target_network'].flat).all())
out['next_actions_dtype'] = str(g['next_actions'].dtype)
out['both_actions'] = sorted(set(g['next_actions'].tolist()))
out['names'] = sorted(k for k in ('env', 'q_network', 'target_network', 'optimizer') if k in g)
out['lines'] = buf.getvalue().splitlines()
print('SCRIPT_JSON ' + json.dumps(out))
"""


def _run_globals(**kw):
    p = subprocess.run([sys.executable, "-c", _GLOBALS], env=_env(**kw), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SCRIPT_JSON ")][0][len("SCRIPT_JSON "):])


def test_script_at_one_env_has_its_lines_names_shapes_and_constants():
    g = _run_globals(NUM_ENVS=1, TOTAL_TIMESTEPS=3000)
    assert g["observations"] == [3001, 4] and g["actions"] == [3001] and g["rewards"] == [3001] and g["terminated"] == [3001] and g["observation"] == [4]
    assert g["dtypes"] == ["torch.float32", "torch.int64", "torch.float32", "torch.bool"]
    assert g["batch_inds"] == [128] and g["target_values"] == [128] and g["current"] == [128] and g["next_actions"] == [128] and g["next_actions_dtype"] == "torch.int32"
    assert g["bonus"] == [128] and g["soft_value"] == [128] and (g["alpha"], g["tau"], g["clip_lo"]) == (0.9, 0.03, -1.0) == tuple(g["engine_knobs"])
    assert -1.0 <= g["bonus_range"][0] < 0 and g["bonus_range"][1] <= 0 and g["soft_finite"]
    assert g["global_step"] == g["total_timesteps"] == 3000 and g["learning_starts"] == 300 and g["memory_size"] == 3001
    assert (g["train_frequency"], g["target_network_frequency"], g["batch_size"], g["gamma"], g["learning_rate"]) == (10, 500, 128, 0.99, 2.5e-4)
    assert (g["env_id"], g["seed"], g["engine"], g["nets"]) == ("CartPole-v1", 1, "MunchausenDQNEngine", ["QNetwork", "QNetwork"])
    assert (g["start_e"], g["end_e"], g["exploration_fraction"]) == (1, 0.05, 0.5) and g["slope"] == (0.05 - 1) / (0.5 * 3000) and g["adam_eps"] == 1e-8
    assert g["updates"] == 271 and g["finite"] and g["synced"] and np.isfinite(g["loss"]) and g["loss"] > 0       # updates at 300, 310 ... 3,000; the sync at 3,000
    assert {"env", "optimizer", "q_network", "target_network"} <= set(g["names"]) and set(g["both_actions"]) <= {0, 1}
    lines = g["lines"]
    assert len(lines) > 30 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in lines), lines[:3]     # dqn.py's line: 22.00
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    rets = [float(ln.split("episodic_return=")[1]) for ln in lines]
    assert steps == np.cumsum(rets).astype(int).tolist()      # every env step belongs to one episode; CartPole's return is its length


def test_script_module_runs_as_main():
    p = subprocess.run([sys.executable, "-m", "deep_rl_amd.munchausen_dqn"], env=_env(TOTAL_TIMESTEPS=1000), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) > 10 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in lines)


def test_script_on_a_64_env_ring_that_wraps_stays_finite():
    """with the three knobs set from the environment: they reach the engine, and the bonus respects the CLIP_LO given"""
    g = _run_globals(NUM_ENVS=64, TOTAL_TIMESTEPS=600, MEMORY_SIZE=32, LEARNING_STARTS=100, ALPHA=0.5, TAU=0.1, CLIP_LO=-0.25)
    assert g["engine_knobs"] == [0.5, 0.1, -0.25] and -0.25 <= g["bonus_range"][0] <= g["bonus_range"][1] <= 0 and g["soft_finite"]
    assert g["observations"] == [32, 64, 4] and g["actions"] == [32, 64] and g["global_step"] == 600 and g["memory_size"] == 32 < 600
    assert g["updates"] == 51 and g["finite"] and np.isfinite(g["loss"]) and g["lines"] == []


_CODE = r"""
import contextlib, io, json, os, runpy, sys
seeds = [int(s) for s in sys.argv[1].split(',')]
out = {}
for s in seeds:
    os.environ.update(SEED=str(s), NUM_ENVS='1')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_module('deep_rl_amd.munchausen_dqn', run_name='__main__')
    out[s] = [float(ln.split('episodic_return=')[1]) for ln in buf.getvalue().splitlines() if ln.startswith('global_step=')]
print('LEARNING_JSON ' + json.dumps(out))
"""
SEEDS = (1, 2, 3, 4, 5, 6)


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def test_production_rng_path_learns_like_the_torch_script():
    ref = np.load(os.path.join(ROOT, "tests", "golden", "mdqn_learning_stats.npz"))["mdqn_last_tenth_mean"].astype(np.float64)
    assert ref.shape == (24,) and np.isfinite(ref).all()
    assert len(SEEDS) <= 6                                              # at most six child processes at once, each under its own timeout below
    procs = [subprocess.Popen([sys.executable, "-c", _CODE, str(s)], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for s in SEEDS]
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
    assert sorted(runs) == list(SEEDS) and all(len(runs[s]) > 100 and np.isfinite(runs[s]).all() for s in SEEDS)
    ours = np.array([last_tenth(runs[s]) for s in SEEDS])
    floor = float(ref.mean() - 3.0 * ref.std(ddof=1) / np.sqrt(len(SEEDS)))
    rec = {"script": "munchausen_dqn", "seeds": list(SEEDS), "statistic": "mean episodic return of the last tenth of the episodes of a run",
           "ours_gpu": [round(x, 2) for x in ours.tolist()], "ours_mean": round(float(ours.mean()), 2), "reference_mean": round(float(ref.mean()), 2),
           "reference_seed_sd": round(float(ref.std(ddof=1)), 2), "floor": round(floor, 2)}
    path = os.path.join(results_dir(), "learning_stats_gpu.json")      # under the key "munchausen_dqn", beside the other scripts' records
    allrec = json.load(open(path)) if os.path.exists(path) else {}
    allrec["munchausen_dqn"] = rec
    json.dump(allrec, open(path, "w"), indent=1)
    print(json.dumps(rec))
    assert ours.mean() >= floor, rec
