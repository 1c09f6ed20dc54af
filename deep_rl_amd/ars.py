"""Augmented Random Search on CartPole-v1 (Mania, Guy, Recht 2018: ARS V2-t with discrete actions; NORMALIZE=0 gives V1).  The reference project lists ARS in
its README and has no script for it; this one follows the shape of the project's other single-file scripts.  Run:  ``python -m deep_rl_amd.ars``.

Per iteration N directions are drawn, 2 N perturbed linear policies play one episode each, and the policy moves along the best N_TOP directions.  The arithmetic
runs in hand-written HIP kernels (deep_rl_amd/csrc/mi_ars.hip) on an MI355X; this file only sequences launches.

Knobs, read from the environment: N_DIRECTIONS (default 8), N_TOP (default: N_DIRECTIONS), STEP_SIZE (0.02), NOISE (0.03), NORMALIZE (1), NUM_ITERATIONS (40),
SEED (1), EVAL_EPISODES (100; 0: no final evaluation).
"""
import os

import torch

from deep_rl_amd import ARSEngine

env_id = "CartPole-v1"

n_directions = int(os.environ.get("N_DIRECTIONS", "8"))
n_top = int(os.environ.get("N_TOP", str(n_directions)))
step_size = float(os.environ.get("STEP_SIZE", "0.02"))
noise = float(os.environ.get("NOISE", "0.03"))
normalize = int(os.environ.get("NORMALIZE", "1")) != 0
num_iterations = int(os.environ.get("NUM_ITERATIONS", "40"))
seed = int(os.environ.get("SEED", "1"))
eval_episodes = int(os.environ.get("EVAL_EPISODES", "100"))
device = torch.device("cuda", 0)

engine = ARSEngine(n_directions=n_directions, n_top=n_top, step_size=step_size, noise=noise, normalize=normalize, seed=seed, device=device)

global_step = 0
mean_returns = []   # per iteration, over its 2 N episodes

for iteration in range(num_iterations):
    engine.train(1)
    n_finished, finished = engine.drain_episodes()
    steps = sum(length for _e, length, _r in finished)
    mean_returns.append(steps / n_finished)
    if n_directions <= 8:
        for _e, length, ret in finished:
            global_step += length
            print(f"global_step={global_step}, episodic_return={ret:.2f}")
    else:
        global_step += steps
        print(f"iteration={iteration}, global_step={global_step}, episodes={n_finished}, mean_episodic_return={steps / n_finished:.2f}")

last = mean_returns[-10:]
print(f"train_mean_return_last_{len(last)}={sum(last) / len(last):.4f}")
if eval_episodes > 0:
    result = engine.evaluate(eval_episodes)
    print("eval " + result.line())
policy = engine.policy
