"""REINFORCE on CartPole-v1 — the drop-in counterpart of the reference single-file script ``deep_rl/reinforce.py``.

Same top-level names, constants, seeding order, printed lines and final module globals as the reference (file:line comments point into it), with an env
axis ``num_envs`` that reduces to the reference at 1: per update every env plays one episode, then one Adam step on the summed loss.  The arithmetic runs
in hand-written HIP kernels (deep_rl_amd/csrc/mi_reinforce.hip) on an MI355X; this file only sequences launches.  Run:  ``python -m deep_rl_amd.reinforce``.

Knobs the reference does not have are read from the environment so the constants below stay the reference's:
NUM_ENVS (default 1), SEED (default 1), NUM_EPISODES (updates, default 100), PRINT_EPISODES (default: 1 if NUM_ENVS <= 8).
"""
import os

import numpy as np
import torch

from deep_rl_amd import Adam, DropoutPolicy, ReinforceEngine, make

LOG_STD_MIN = -5  # reinforce.py:9 (np.exp(LOG_STD_MIN) is the epsilon of the return normalisation, :73 — a constant of the returns kernel)

env_id = "CartPole-v1"  # :27

gamma = 0.99  # :29

num_envs = int(os.environ.get("NUM_ENVS", "1"))  # the reference is implicitly 1
num_episodes = int(os.environ.get("NUM_EPISODES", "100"))  # :51
device = torch.device("cuda", 0)

# Env setup (:32-33)
env = make(env_id, num_envs=num_envs, device=device)

# Seeding (:36-38), same order: env, torch — before the agent is built so the init matches
seed = int(os.environ.get("SEED", "1"))
env.seed(seed)
torch.manual_seed(seed)

agent = DropoutPolicy(env)  # :40-46
optimizer = Adam(agent, lr=1e-2)  # :47

print_episodes = int(os.environ.get("PRINT_EPISODES", "1" if num_envs <= 8 else "0"))
engine = ReinforceEngine(env, agent, optimizer, gamma=gamma)
# At num_envs == 1 the storage globals are views WITHOUT the env axis, i.e. exactly the reference's shapes (:53-54); the engine keeps writing the same memory.
_ref = (lambda t: t.squeeze(0)) if num_envs == 1 else (lambda t: t)
log_probs, returns = _ref(engine.log_probs), _ref(engine.returns)  # (501,) each at one env

global_step = 0  # :49

for episode_idx in range(num_episodes):  # :51
    # episode (:53-67), normalised returns (:71-73), loss gradient (:74-76) and the Adam step (:77): one enqueue
    engine.update()

    n_finished, finished = engine.drain_episodes()
    if print_episodes:
        for _e, length, ret in finished:
            global_step += length
            print(f"global_step={global_step}, episodic_return={ret:.2f}")  # :69
    else:
        steps = sum(length for _e, length, _r in finished)
        global_step += steps
        print(f"update={episode_idx}, global_step={global_step}, episodes={n_finished}, mean_episodic_return={steps / n_finished:.2f}")

lengths = engine.lengths.cpu()
step = int(lengths[0]) if num_envs == 1 else lengths  # :58,65
if num_envs == 1:
    b_returns, b_log_probs = engine.b_returns[0, :step], engine.log_probs[0, :step]  # :71-73
else:
    b_returns, b_log_probs = engine.b_returns, engine.log_probs  # rows past an episode's end are 0
policy_loss = torch.sum(-b_log_probs * b_returns)  # :74 (of the last update, at the parameters before its step)
done = True

env.close()
