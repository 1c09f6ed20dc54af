"""Rainbow (Hessel et al. 2018) on CartPole-v1 — a drop-in single-file script in the style of the reference family.

The reference has no Rainbow script; this is ``noisy_dqn.py`` — ``dqn.py``'s loop, hyper-parameters, seeding order, storage index conventions and printed line with
the dueling network, the double rule, ``per.py``'s prioritized replay, N_STEP-step returns and noisy value and advantage streams — with the sixth ingredient, as
include/mi_rainbow.h fixes it: the streams produce 51 atoms each on the support [V_MIN, V_MAX], the target is the n-step categorical projection of the target
network's distribution of the online network's greedy action, the loss is the importance-weighted cross-entropy against it and a row's cross-entropy is its new
priority.  The default support 0 .. 100 has ``c51.py``'s atom spacing of 2 on the half of its range CartPole's non-negative returns can reach.  NOISY=0 is the mean
network with ``dqn.py``'s epsilon schedule.  An env axis ``num_envs`` (NUM_ENVS, default 1); one loop iteration = ``train_frequency`` env steps of every env
followed by one update.
Env knobs: NUM_ENVS, TOTAL_TIMESTEPS (time steps; default 100_000), MEMORY_SIZE (ring slots; default TOTAL_TIMESTEPS + 1 = linear storage), BATCH_SIZE,
LEARNING_STARTS, SEED, PRINT_EPISODES, PRIORITIZED (default 1; 0: uniform replay), N_STEP (default 3; 1 .. 16, below MEMORY_SIZE), NOISY (default 1), SIGMA_0,
V_MIN (default 0), V_MAX (default 100).
"""
import os

import numpy as np
import torch

from deep_rl_amd import Adam, RainbowEngine, RainbowQNetwork, make

env_id = "CartPole-v1"

num_envs = int(os.environ.get("NUM_ENVS", "1"))
device = torch.device("cuda", 0)
torch.cuda.set_device(device)

total_timesteps = int(os.environ.get("TOTAL_TIMESTEPS", "100000"))
learning_starts = int(os.environ.get("LEARNING_STARTS", str(min(10_000, total_timesteps // 10))))  # as dqn.py's counterpart shortens it

noisy = os.environ.get("NOISY", "1") != "0"
sigma_0 = float(os.environ.get("SIGMA_0", "0.5"))
start_e = 0.0 if noisy else 1   # the noise is the exploration; NOISY=0: dqn.py's schedule
end_e = 0.0 if noisy else 0.05
exploration_fraction = 0.5
slope = (end_e - start_e) / (exploration_fraction * total_timesteps)

train_frequency = 10
batch_size = int(os.environ.get("BATCH_SIZE", "128"))
gamma = 0.99
learning_rate = 2.5e-4
target_network_frequency = 500
prioritized = os.environ.get("PRIORITIZED", "1") != "0"
alpha = 0.6
beta_0 = 0.4
n_step = int(os.environ.get("N_STEP", "3"))
n_atoms = 51
v_min = float(os.environ.get("V_MIN", "0"))
v_max = float(os.environ.get("V_MAX", "100"))
# the loop below looks at the train / target-sync conditions at chunk boundaries only
assert target_network_frequency % train_frequency == 0, "target_network_frequency must be a multiple of train_frequency"

# Env setup
env = make(env_id, num_envs=num_envs, device=device)

# Seeding
seed = int(os.environ.get("SEED", "1"))  # SEED re-keys every counter-based stream
env.seed(seed)
np.random.seed(seed)
torch.manual_seed(seed)
env.action_space.seed(seed)

# Network setup
q_network = RainbowQNetwork(env, sigma_0=sigma_0, n_atoms=n_atoms, v_min=v_min, v_max=v_max)
optimizer = Adam(q_network, lr=learning_rate)  # optim.Adam defaults (eps 1e-8)
target_network = RainbowQNetwork(env, sigma_0=sigma_0, n_atoms=n_atoms, v_min=v_min, v_max=v_max)
target_network.load_state_dict(q_network.state_dict())

# Storage setup lives in the engine as a [slots, num_envs] ring
memory_size = int(os.environ.get("MEMORY_SIZE", str(total_timesteps + 1)))
print_episodes = int(os.environ.get("PRINT_EPISODES", "1" if num_envs <= 8 else "0"))
engine = RainbowEngine(env, q_network, target_network, optimizer, slots=memory_size, batch_size=batch_size, gamma=gamma, learning_starts=learning_starts,
                       start_e=start_e, end_e=end_e, exploration_fraction=exploration_fraction, total_timesteps=total_timesteps,
                       max_episodes_logged=(4 * train_frequency * num_envs if print_episodes else 0), prioritized=prioritized, alpha=alpha, beta_0=beta_0,
                       n_step=n_step, noisy=noisy, n_atoms=n_atoms, v_min=v_min, v_max=v_max)
# At num_envs == 1 the storage globals are views WITHOUT the env axis; the engine keeps writing the same memory through its own (T + 1, 1, ...) tensors.
_ref = (lambda t: t.squeeze(1)) if num_envs == 1 else (lambda t: t)
observations, actions, rewards, terminated = _ref(engine.observations), _ref(engine.actions), _ref(engine.rewards), _ref(engine.terminated).view(torch.bool)
priorities = _ref(engine.priorities) if prioritized else None

# Initiate the environment and store the initial observation
observation = engine.reset()
observation = observation.squeeze(0) if num_envs == 1 else observation
global_step = 0

# Loop
while global_step < total_timesteps:
    n = min(train_frequency - global_step % train_frequency, total_timesteps - global_step)
    engine.act(n)
    if print_episodes:
        _, finished = engine.drain_episodes()
        for e, t, r, _l in finished:
            print(f"global_step={(global_step + t + 1)}, episodic_return={r:.2f}")  # dqn.py's line, printed after the increment
    global_step += n

    # Optimize the agent
    if global_step >= learning_starts:
        if global_step % train_frequency == 0:
            engine.train_step()
        # Update the target network
        if global_step % target_network_frequency == 0:
            engine.sync_target()

observation = engine.observation.squeeze(0) if num_envs == 1 else engine.observation
batch_inds, target_probs, probs, next_actions, prio = engine.batch_inds, engine.target_probs, engine.probs, engine.next_actions, engine.prio
horizon = engine.horizon
max_priority = float(engine.max_priority.item()) if prioritized else None
loss = float(engine.loss.item())
env.close()
