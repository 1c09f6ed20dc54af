"""``python -m deep_rl_amd.ars``: its lines and knobs, and whether the production path — the device's own float32 draw, the keyed starts, the chained launches —
learns like the CPU restatement with its own float64 draw (tools/capture_ars_ref.py -> tests/golden/ars_ref_learning.json: 24 seeds, 40 iterations at the script's
defaults).  Seeds 1 .. 6 run in one fresh child process each, all six side by side, each under its own timeout.  One-sided: the six-seed mean of the last-10
training mean must reach the fixture's floor (mean - 3 sd), and each seed's greedy evaluate(100) mean the reference's smallest greedy mean."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SEED", "N_DIRECTIONS", "N_TOP", "STEP_SIZE", "NOISE", "NORMALIZE", "NUM_ITERATIONS", "EVAL_EPISODES", "MIRL_ARS_SO")
SEEDS = (1, 2, 3, 4, 5, 6)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in KNOBS:
        env.pop(k, None)
    env.update({k: str(v) for k, v in kw.items()})
    return env


def _start(**kw):
    return subprocess.Popen([sys.executable, "-m", "deep_rl_amd.ars"], env=_env(**kw), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)


def _finish(p):
    out, err = p.communicate(timeout=240)
    assert p.returncode == 0, err[-3000:]
    return out.splitlines()


@pytest.fixture(scope="module")
def runs():
    """the six default runs, started together"""
    procs = [_start(SEED=s) for s in SEEDS]
    try:
        return {s: _finish(p) for s, p in zip(SEEDS, procs)}
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()


def test_script_lines_at_the_defaults(runs):
    lines = runs[1]
    eps = [ln for ln in lines if ln.startswith("global_step=")]
    assert len(eps) == 40 * 16 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.00", ln) for ln in eps), eps[:3]
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in eps]
    rets = [float(ln.split("episodic_return=")[1]) for ln in eps]
    assert steps == [int(sum(rets[:i + 1])) for i in range(len(rets))] and max(rets) == 500.0      # every env step belongs to one episode; CartPole's return is its length
    assert re.fullmatch(r"train_mean_return_last_10=\d+\.\d{4}", lines[-2]) and lines[-1].startswith("eval episodes=100 mean_return=")
    assert abs(float(lines[-2].split("=")[1]) - sum(rets[-160:]) / 160) < 1e-3


def test_script_knobs_and_the_summary_line_above_eight_directions():
    lines = _finish(_start(SEED=2, N_DIRECTIONS=16, N_TOP=4, NUM_ITERATIONS=3, STEP_SIZE=0.05, NOISE=0.1, NORMALIZE=0, EVAL_EPISODES=0))
    assert len(lines) == 4 and all(re.fullmatch(r"iteration=%d, global_step=\d+, episodes=32, mean_episodic_return=\d+\.\d\d" % i, lines[i]) for i in range(3)), lines
    assert lines[-1].startswith("train_mean_return_last_3=")


def test_six_seeds_learn_like_the_reference(runs):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ars_ref_learning.json")))
    train = {s: float(runs[s][-2].split("=")[1]) for s in SEEDS}
    greedy = {s: float(re.search(r"mean_return=([0-9.]+)", runs[s][-1]).group(1)) for s in SEEDS}
    mean = sum(train.values()) / len(train)
    print("last-10 training means %s -> %.3f (floor %.3f); greedy means %s (reference minimum %.3f)" % (train, mean, fx["floor"], greedy, fx["greedy_min"]))
    from _c51_ref import results_dir
    with open(os.path.join(results_dir(), "ars_learning.json"), "w") as f:
        json.dump(dict(train_last_mean=train, greedy_mean=greedy, mean=mean, floor=fx["floor"], greedy_min=fx["greedy_min"]), f, indent=1, sort_keys=True)
    assert mean >= fx["floor"]
    assert all(g >= fx["greedy_min"] for g in greedy.values()), greedy
