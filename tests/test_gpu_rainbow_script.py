"""The drop-in script ``python -m deep_rl_amd.rainbow``: its lines, names, shapes, dtypes and constants at one env, a finite run on a 64-env ring that wraps (both
replay modes, noisy and NOISY=0) — and whether the PRODUCTION random path (keyed reset noise, the keyed noisy heads of acting and learning, libmirl's prioritized
sampler fed the row losses) learns like the plain torch script that stands in for the missing reference (tools/capture_rainbow_ref.py): seeds 1 .. 6 at the full
100,000 steps, one test per seed, against tests/golden/rainbow_learning_stats.npz (the last-tenth mean return of the torch script's seeds 1 .. 24).  Statistical,
not draw for draw.  One-sided: the mean of the six must be >= the fixture's mean - 3 x the fixture's seed-to-seed sd / sqrt(6) (the rule of
tests/test_gpu_noisy_script.py).  The record goes to rainbow_learning.json in the tests' results directory."""
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
KNOBS = ("SEED", "NUM_ENVS", "TOTAL_TIMESTEPS", "MEMORY_SIZE", "BATCH_SIZE", "LEARNING_STARTS", "PRINT_EPISODES", "PRIORITIZED", "N_STEP", "NOISY", "SIGMA_0", "V_MIN", "V_MAX", "MIRL_RB_SO")


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
    g = runpy.run_module('deep_rl_amd.rainbow', run_name='__main__')
out = {k: (list(g[k].shape) if torch.is_tensor(g[k]) else g[k]) for k in ('observations', 'actions', 'rewards', 'terminated', 'priorities', 'observation', 'batch_inds', 'target_probs',
       'probs', 'next_actions', 'prio', 'horizon', 'n_atoms', 'v_min', 'v_max', 'n_step', 'global_step', 'total_timesteps', 'learning_starts', 'train_frequency', 'target_network_frequency', 'batch_size', 'gamma',
       'learning_rate', 'env_id', 'seed', 'start_e', 'end_e', 'exploration_fraction', 'slope', 'memory_size', 'loss', 'alpha', 'beta_0', 'prioritized', 'max_priority', 'noisy', 'sigma_0')}
out['dtypes'] = [str(g[k].dtype) for k in ('observations', 'actions', 'rewards', 'terminated')]
out['adam_eps'] = g['optimizer'].param_groups[0]['eps']
out['updates'] = g['engine'].update_index
out['engine'] = type(g['engine']).__name__
out['nets'] = [type(g['q_network']).__name__, type(g['target_network']).__name__]
out['finite'] = bool(torch.isfinite(g['q_network'].flat).all()) and bool(torch.isfinite(g['engine'].observations).all())
out['synced'] = bool((g['q_network'].flat == g['target_network'].flat).all())
out['next_actions_dtype'] = str(g['next_actions'].dtype)
out['both_actions'] = sorted(set(g['next_actions'].tolist()))
out['horizon_dtype'] = str(g['horizon'].dtype)
out['horizons'] = sorted(set(g['horizon'].tolist()))
out['engine_n_step'] = g['engine'].n_step
out['engine_noisy'] = g['engine'].noisy
out['nparams'] = g['q_network'].flat.numel()
f, f0 = g['q_network'].flat, torch.tensor(0.5 / 84 ** 0.5, dtype=torch.float32)
out['sigma_moved'] = float((f[23769:] - f0).abs().max())
out['sigma_grad'] = bool(g['engine'].grads[23769:].any())
out['names'] = sorted(k for k in ('env', 'q_network', 'target_network', 'optimizer') if k in g)
if g['prioritized']:
    e = g['engine']
    p = e.priorities.reshape(-1)
    out['prio_ring'] = dict(finite=bool(torch.isfinite(p).all()), nonneg=bool((p >= 0).all()), head=float(p.reshape(e.slots, e.N)[e.global_step % e.slots].max()),
                       top=float(p.max()), distinct=int(torch.unique(p).numel()), beta=e.beta(), weights_max=float(e.weights.max()), weights_min=float(e.weights.min()))
out['lines'] = buf.getvalue().splitlines()
print('SCRIPT_JSON ' + json.dumps(out))
"""


def _run_globals(**kw):
    p = subprocess.run([sys.executable, "-c", _GLOBALS], env=_env(**kw), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SCRIPT_JSON ")][0][len("SCRIPT_JSON "):])


def test_script_at_one_env_has_its_lines_names_shapes_and_constants():
    g = _run_globals(NUM_ENVS=1, TOTAL_TIMESTEPS=3000)
    assert g["observations"] == [3001, 4] and g["actions"] == [3001] and g["rewards"] == [3001] and g["terminated"] == [3001] and g["priorities"] == [3001] and g["observation"] == [4]
    assert g["dtypes"] == ["torch.float32", "torch.int64", "torch.float32", "torch.bool"]
    assert g["batch_inds"] == [128] and g["target_probs"] == [128, 51] and g["probs"] == [128, 51] and g["prio"] == [128] and g["next_actions"] == [128]
    assert (g["n_atoms"], g["v_min"], g["v_max"]) == (51, 0.0, 100.0)
    assert g["horizon"] == [128] and g["horizon_dtype"] == "torch.int32" and g["n_step"] == g["engine_n_step"] == 3 and g["horizons"] == [1, 2, 3]
    assert g["next_actions_dtype"] == "torch.int32"
    assert g["global_step"] == g["total_timesteps"] == 3000 and g["learning_starts"] == 300 and g["memory_size"] == 3001
    assert (g["train_frequency"], g["target_network_frequency"], g["batch_size"], g["gamma"], g["learning_rate"]) == (10, 500, 128, 0.99, 2.5e-4)
    assert (g["alpha"], g["beta_0"], g["prioritized"]) == (0.6, 0.4, True)
    assert (g["env_id"], g["seed"], g["engine"], g["nets"]) == ("CartPole-v1", 1, "RainbowEngine", ["RainbowQNetwork", "RainbowQNetwork"])
    assert (g["start_e"], g["end_e"], g["exploration_fraction"]) == (0.0, 0.0, 0.5) and g["slope"] == 0.0 and g["adam_eps"] == 1e-8       # the noise is the exploration
    assert g["noisy"] is True and g["engine_noisy"] is True and g["sigma_0"] == 0.5 and g["nparams"] == 36774 and g["sigma_grad"] and g["sigma_moved"] > 20 * 2.5e-4
    assert g["updates"] == 271 and g["finite"] and g["synced"] and np.isfinite(g["loss"]) and g["loss"] > 0       # updates at 300, 310 ... 3,000; the sync at 3,000
    assert {"env", "optimizer", "q_network", "target_network"} <= set(g["names"]) and set(g["both_actions"]) <= {0, 1}
    p = g["prio_ring"]
    assert p["finite"] and p["nonneg"] and p["head"] == 0.0 and p["top"] <= g["max_priority"] and g["max_priority"] > 1e-2 and p["distinct"] > 500
    assert p["beta"] == 1.0 and p["weights_max"] == 1.0 and 0 < p["weights_min"] < 1
    lines = g["lines"]
    assert len(lines) > 30 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in lines), lines[:3]     # dqn.py's line: 22.00
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    rets = [float(ln.split("episodic_return=")[1]) for ln in lines]
    assert steps == np.cumsum(rets).astype(int).tolist()      # every env step belongs to one episode; CartPole's return is its length


def test_script_module_runs_as_main():
    p = subprocess.run([sys.executable, "-m", "deep_rl_amd.rainbow"], env=_env(TOTAL_TIMESTEPS=1000), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) > 10 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in lines)


@pytest.mark.parametrize("noisy", [1, 0], ids=["noisy", "mean"])
@pytest.mark.parametrize("prioritized", [1, 0], ids=["prioritized", "uniform"])
def test_script_on_a_64_env_ring_that_wraps_stays_finite(prioritized, noisy):
    g = _run_globals(NUM_ENVS=64, TOTAL_TIMESTEPS=600, MEMORY_SIZE=32, LEARNING_STARTS=100, PRIORITIZED=prioritized, NOISY=noisy)
    assert g["n_step"] == g["engine_n_step"] == 3 and g["horizons"] == [1, 2, 3] and g["noisy"] == g["engine_noisy"] == bool(noisy)
    assert g["observations"] == [32, 64, 4] and g["actions"] == [32, 64] and g["global_step"] == 600 and g["memory_size"] == 32 < 600
    assert g["updates"] == 51 and g["finite"] and np.isfinite(g["loss"]) and g["lines"] == [] and g["prioritized"] == bool(prioritized)
    assert (g["start_e"], g["end_e"]) == ((0.0, 0.0) if noisy else (1, 0.05)) and g["sigma_grad"] == bool(noisy) and (g["sigma_moved"] > 0) == bool(noisy)
    if prioritized:
        assert g["priorities"] == [32, 64] and g["prio_ring"]["finite"] and g["prio_ring"]["nonneg"] and g["prio_ring"]["head"] == 0.0 and g["prio_ring"]["top"] <= g["max_priority"]
    else:
        assert g["priorities"] is None and g["max_priority"] is None


_CODE = r"""
import contextlib, io, json, os, runpy, sys
s = int(sys.argv[1])
os.environ.update(SEED=str(s), NUM_ENVS='1')
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    runpy.run_module('deep_rl_amd.rainbow', run_name='__main__')
print('LEARNING_JSON ' + json.dumps([float(ln.split('episodic_return=')[1]) for ln in buf.getvalue().splitlines() if ln.startswith('global_step=')]))
"""
SEEDS = (1, 2, 3, 4, 5, 6)
_RUNS = {}


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def _run_seed(s):
    """the script at seed s, 100,000 steps, in a process of its own (once: the judging test reuses what the per-seed tests ran)"""
    if s not in _RUNS:
        p = subprocess.run([sys.executable, "-c", _CODE, str(s)], env=_env(), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEARNING_JSON ")][0]
        _RUNS[s] = json.loads(line[len("LEARNING_JSON "):])
    return _RUNS[s]


@pytest.mark.parametrize("seed", SEEDS)
def test_production_rng_path_runs_a_seed(seed):
    rets = _run_seed(seed)
    assert len(rets) > 100 and np.isfinite(rets).all() and sum(rets) <= 100_000 and min(rets) >= 8 and max(rets) <= 500
    print("seed %d: %d episodes, last-tenth mean %.2f" % (seed, len(rets), last_tenth(rets)))


def test_production_rng_path_learns_like_the_torch_script():
    ref = np.load(os.path.join(ROOT, "tests", "golden", "rainbow_learning_stats.npz"))["rainbow_last_tenth_mean"].astype(np.float64)
    assert ref.shape == (24,) and np.isfinite(ref).all()
    ours = np.array([last_tenth(_run_seed(s)) for s in SEEDS])
    floor = float(ref.mean() - 3.0 * ref.std(ddof=1) / np.sqrt(len(SEEDS)))
    rec = {"script": "rainbow", "n_step": 3, "sigma_0": 0.5, "support": [0.0, 100.0], "seeds": list(SEEDS), "statistic": "mean episodic return of the last tenth of the episodes of a run",
           "ours_gpu": [round(x, 2) for x in ours.tolist()], "ours_mean": round(float(ours.mean()), 2), "reference_mean": round(float(ref.mean()), 2),
           "reference_seed_sd": round(float(ref.std(ddof=1)), 2), "floor": round(floor, 2)}
    from deep_rl_amd import _native_rb
    rec["rainbow_source_id"] = _native_rb.source_id()
    json.dump(rec, open(os.path.join(results_dir(), "rainbow_learning.json"), "w"), indent=1)
    print(json.dumps(rec))
    assert ours.mean() >= floor, rec
