"""IQN (implicit quantile network) on CartPole-v1 — the drop-in counterpart of the reference single-file script ``deep_rl/iqn.py``, re-targeted from Pong.

Same top-level names, seeding order, storage index conventions, printed lines and final module globals as the reference, with an env axis ``num_envs``
(NUM_ENVS, default 1).  What changes with the re-target: ``env_id``, the FeaturesExtractor (each Conv2d(c_in, c_out, k, s) is Linear(c_in, c_out)), f32
observation storage (no uint8, no / 255) and the horizon (total_timesteps, learning_starts, epsilon_decay_steps, target_network_frequency).  One loop iteration =
``train_frequency`` env steps of every env in one launch followed by one update (two launches).
Env knobs: NUM_ENVS, TOTAL_TIMESTEPS (time steps; default 50_000), MEMORY_SIZE (ring slots; default TOTAL_TIMESTEPS + 1 = linear storage), BATCH_SIZE,
LEARNING_STARTS, SEED, PRINT_EPISODES.
"""
import os

import numpy as np
import torch

from deep_rl_amd import Adam, CosineEmbeddingNetwork, FeaturesExtractor, IQNEngine, QuantileNetwork, make, pack

env_id = "CartPole-v1"  # iqn.py:116 (re-targeted)

num_envs = int(os.environ.get("NUM_ENVS", "1"))
device = torch.device("cuda", 0)
torch.cuda.set_device(device)

total_timesteps = int(os.environ.get("TOTAL_TIMESTEPS", "50000"))  # :118 (re-targeted)
learning_starts = int(os.environ.get("LEARNING_STARTS", str(min(1_000, total_timesteps // 2))))  # :119 (re-targeted)

final_epsilon = 0.01  # :121
epsilon_decay_steps = 10_000  # :122 (re-targeted)
slope = -(1.0 - final_epsilon) / epsilon_decay_steps

train_frequency = 4  # :125
batch_size = int(os.environ.get("BATCH_SIZE", "32"))
gamma = 0.99
learning_rate = 5e-5
target_network_frequency = 500  # :129 (re-targeted)
# the loop below looks at the train / target-sync conditions (:224, :296) at chunk boundaries only
assert target_network_frequency % train_frequency == 0, "target_network_frequency must be a multiple of train_frequency"

num_tau_samples = 64  # :131
num_tau_prime_samples = 64
num_quantile_samples = 32
num_cosines = 64
embedding_dim = 1 * 1 * 64  # :135 at spatial extent 1 x 1
kappa = 1.0
memory_size = int(os.environ.get("MEMORY_SIZE", str(total_timesteps + 1)))  # :137

# Env setup (:140-142)
env = make(env_id, num_envs=num_envs, device=device)

# Seeding (:145-150)
seed = int(os.environ.get("SEED", "0"))  # the reference hard-codes 0; SEED re-keys every counter-based stream
torch.manual_seed(seed)
np.random.seed(seed)
env.seed(seed)
env.action_space.seed(seed)

# Network setup (:156-162)
online_features_extractor = FeaturesExtractor(env)
online_cosine_net = CosineEmbeddingNetwork(num_cosines=num_cosines, embedding_dim=embedding_dim, device=device)
online_quantile_net = QuantileNetwork(num_actions=env.action_space.n, embedding_dim=embedding_dim, device=device)

target_features_extractor = FeaturesExtractor(env)
target_cosine_net = CosineEmbeddingNetwork(num_cosines=num_cosines, embedding_dim=embedding_dim, device=device)
target_quantile_net = QuantileNetwork(num_actions=env.action_space.n, embedding_dim=embedding_dim, device=device)

# one 44,898-float buffer per network, in the order of the optimizer's parameter list (:170)
online_params = pack(online_features_extractor, online_cosine_net, online_quantile_net)
target_params = pack(target_features_extractor, target_cosine_net, target_quantile_net)

# Initialize the weights (:165-167)
target_features_extractor.load_state_dict(online_features_extractor.state_dict())
target_cosine_net.load_state_dict(online_cosine_net.state_dict())
target_quantile_net.load_state_dict(online_quantile_net.state_dict())

# Instanciate the optimizer (:170-171)
parameters = [*online_features_extractor.parameters(), *online_cosine_net.parameters(), *online_quantile_net.parameters()]
optimizer = Adam(online_params, lr=learning_rate, eps=1e-2 / batch_size)

# Storage setup (:174-177) lives in the engine as a [slots, num_envs] ring
print_episodes = int(os.environ.get("PRINT_EPISODES", "1" if num_envs <= 8 else "0"))
engine = IQNEngine(env, online_params, target_params, optimizer, slots=memory_size, batch_size=batch_size, gamma=gamma, final_epsilon=final_epsilon,
                   epsilon_decay_steps=epsilon_decay_steps, learning_starts=learning_starts, max_episodes_logged=(4 * train_frequency * num_envs if print_episodes else 0))
# At num_envs == 1 the storage globals are views WITHOUT the env axis, i.e. the reference's shapes
_ref = (lambda t: t.squeeze(1)) if num_envs == 1 else (lambda t: t)
observations, actions, rewards, terminated = _ref(engine.observations), _ref(engine.actions), _ref(engine.rewards), _ref(engine.terminated).view(torch.bool)

# Initiate the envrionment and store the inital observation (:180-182)
observation = engine.reset()
observation = observation.squeeze(0) if num_envs == 1 else observation
global_step = 0

# Loop (:185)
while global_step < total_timesteps:
    n = min(train_frequency - global_step % train_frequency, total_timesteps - global_step)
    engine.act(n)  # :187-217 for n time steps
    if print_episodes:
        _, finished = engine.drain_episodes()
        for e, t, r, _l in finished:
            print(f"global_step={(global_step + t + 1)}, episodic_return={r:.2f}")  # :220
    global_step += n

    # Optimize the agent (:223-293)
    if global_step >= learning_starts:
        if global_step % train_frequency == 0:
            engine.train_step()
        # Update the target network (:296-299)
        if global_step % target_network_frequency == 0:
            engine.sync_target()

observation = engine.observation.squeeze(0) if num_envs == 1 else engine.observation
epsilon = max(1.0 + slope * (global_step - 1), final_epsilon)
batch_inds, taus = engine.batch_inds, engine.taus
current_action_quantiles, target_action_quantiles, next_actions = engine.current_action_quantiles, engine.target_action_quantiles, engine.next_actions
quantile_loss = float(engine.loss.item())
env.close()
