"""C51 (categorical DQN) on CartPole-v1 — the drop-in counterpart of the reference single-file script ``deep_rl/c51.py``.

Same top-level names, hyper-parameters, seeding order, storage index conventions, printed lines and final module globals as the
reference, with an env axis ``num_envs`` (NUM_ENVS, default 1).  One loop iteration = ``train_frequency`` env steps of every env
in one launch (the online network is frozen between two updates, c51.py:122-123) followed by one update (two launches).
Env knobs: NUM_ENVS, TOTAL_TIMESTEPS (time steps; default 20_000), MEMORY_SIZE (ring slots; default TOTAL_TIMESTEPS + 1 =
the reference's linear storage), BATCH_SIZE, LEARNING_STARTS, SEED, PRINT_EPISODES.
"""
import os

import numpy as np
import torch

from deep_rl_amd import Adam, C51Engine, C51QNetwork, make

env_id = "CartPole-v1"  # c51.py:40

num_envs = int(os.environ.get("NUM_ENVS", "1"))
device = torch.device("cuda", 0)
torch.cuda.set_device(device)

total_timesteps = int(os.environ.get("TOTAL_TIMESTEPS", "20000"))  # :42
# :43.  The reference's 10_000 is half its run, the end of the epsilon decay (exploration_fraction 0.5); a shorter TOTAL_TIMESTEPS keeps that half (dqn.py's
# reference starts after a tenth, hence // 10 there)
learning_starts = int(os.environ.get("LEARNING_STARTS", str(min(10_000, total_timesteps // 2))))

start_e = 1  # :45
end_e = 0.05
exploration_fraction = 0.5
slope = (end_e - start_e) / (exploration_fraction * total_timesteps)  # :48

train_frequency = 10  # :50
batch_size = int(os.environ.get("BATCH_SIZE", "128"))
gamma = 0.99
learning_rate = 2.5e-4
target_network_frequency = 500  # :54
# the loop below looks at the train / target-sync conditions (:122-123, :166) at chunk boundaries only
assert target_network_frequency % train_frequency == 0, "target_network_frequency must be a multiple of train_frequency"

v_min = -100  # :56
v_max = 100
n_atoms = 101
delta_z = (v_max - v_min) / (n_atoms - 1)
atoms = torch.linspace(v_min, v_max, steps=n_atoms)  # :60 (the kernels hold the same support as compile-time constants)

# Env setup (:63-64)
env = make(env_id, num_envs=num_envs, device=device)

# Seeding (:67-71)
seed = int(os.environ.get("SEED", "1"))  # the reference hard-codes 1; SEED re-keys every counter-based stream
env.seed(seed)
np.random.seed(seed)
torch.manual_seed(seed)
env.action_space.seed(seed)

# Network setup (:74-77)
q_network = C51QNetwork(env, n_atoms=n_atoms)
optimizer = Adam(q_network, lr=learning_rate, eps=0.01 / batch_size)
target_network = C51QNetwork(env, n_atoms=n_atoms)
target_network.load_state_dict(q_network.state_dict())

# Storage setup (:80-83) lives in the engine as a [slots, num_envs] ring
memory_size = int(os.environ.get("MEMORY_SIZE", str(total_timesteps + 1)))
print_episodes = int(os.environ.get("PRINT_EPISODES", "1" if num_envs <= 8 else "0"))
engine = C51Engine(env, q_network, target_network, optimizer, slots=memory_size, batch_size=batch_size, gamma=gamma, start_e=start_e, end_e=end_e,
                   exploration_fraction=exploration_fraction, total_timesteps=total_timesteps,
                   max_episodes_logged=(4 * train_frequency * num_envs if print_episodes else 0))
# At num_envs == 1 the storage globals are views WITHOUT the env axis, i.e. exactly the reference's shapes; the engine keeps writing the same memory through its own
# (T + 1, 1, ...) tensors.
_ref = (lambda t: t.squeeze(1)) if num_envs == 1 else (lambda t: t)
observations, actions, rewards, terminated = _ref(engine.observations), _ref(engine.actions), _ref(engine.rewards), _ref(engine.terminated).view(torch.bool)

# Initiate the environment and store the initial observation (:86-88)
observation = engine.reset()
observation = observation.squeeze(0) if num_envs == 1 else observation
global_step = 0

# Loop (:91)
while global_step < total_timesteps:
    n = min(train_frequency - global_step % train_frequency, total_timesteps - global_step)
    engine.act(n)  # :93-116 for n time steps
    if print_episodes:
        _, finished = engine.drain_episodes()
        for e, t, r, _l in finished:
            print(f"global_step={(global_step + t + 1)}, episodic_return={r}")  # :119 (printed after the increment; no format spec: 22.0)
    global_step += n

    # Optimize the agent (:122-163)
    if global_step >= learning_starts:
        if global_step % train_frequency == 0:
            engine.train_step()
        # Update the target network (:166-167)
        if global_step % target_network_frequency == 0:
            engine.sync_target()

observation = engine.observation.squeeze(0) if num_envs == 1 else engine.observation
batch_inds, target_probs, probs = engine.batch_inds, engine.target_probs, engine.probs
loss = float(engine.loss.item())
env.close()
