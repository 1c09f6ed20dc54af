"""DoubleDQNEngine — the launch sequence of Double DQN over libmirl_ddqn.so (include/mi_ddqn.h).

The surface of QRDQNEngine: the replay ring and everything around it is RingEngine's (_ring_engine.py); this file adds DQN's epsilon schedule and its
``learning_starts`` clause, the output tensors and the two calls whose arguments are the library's own.  The networks are two plain ``QNetwork``s.
"""
import ctypes as C

import torch

from . import _native_ddqn as K
from ._ring_engine import RingEngine


class DoubleDQNEngine(RingEngine):
    K, ALGO, NEEDS = K, "Double DQN", "two QNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, learning_starts=10_000, start_e=1.0, end_e=0.05,
                 exploration_fraction=0.5, total_timesteps=100_000, max_episodes_logged=None, process_group=None):
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, max_episodes_logged, process_group)
        self.total_timesteps, self.learning_starts = int(total_timesteps), int(learning_starts)
        self.start_e, self.end_e, self.exploration_fraction = float(start_e), float(end_e), float(exploration_fraction)
        self.current = torch.zeros(self.batch_size, dtype=torch.float32, device=self.device)
        self.target_values = torch.zeros(self.batch_size, dtype=torch.float32, device=self.device)

    def act(self, n_steps, forced_actions=None, forced_resets=None):
        """n_steps time steps of every env (the keyed random action before learning_starts, epsilon-greedy through the online network after it, step, auto-reset,
        ring store), one launch."""
        dev = self.device
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        if fa is not None and fa.numel() != int(n_steps) * self.N or fr is not None and fr.numel() != int(n_steps) * self.N * 4:
            raise K.MiError("act: forced_actions / forced_resets must be [n_steps, N] / [n_steps, N, 4]")
        a = K.DDQNAct(K.ptr(self.q.flat), K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(self.episodes) if self.max_ep else None, K.ptr(self.episode_stats),
                      self.global_step, self.total_timesteps, self.learning_starts, self.start_e, self.end_e, self.exploration_fraction, int(n_steps), self.max_ep)
        K.check(K.lib().mi_ddqn_act_steps(self.env.handle, C.byref(self._ring), C.byref(a), self._s()), "mi_ddqn_act_steps")
        self.global_step += int(n_steps)

    def _batch(self, upper):
        return K.DDQNBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.current), K.ptr(self.target_values),
                           K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper,
                           self.batch_size, self.gamma, self.mid_event)

    def target(self):
        """next_actions (the online network's greedy action at the successor) / target_values (the target network's value of it) of batch_inds."""
        b = self._batch(0)
        K.check(K.lib().mi_ddqn_target(C.byref(self._ring), C.byref(b), self._s()), "mi_ddqn_target")

    def forward(self, observation):
        """the action values [..., 2] of the online network through mi_ddqn_forward: the values the acting and the gradient launch compare"""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        K.check(K.lib().mi_ddqn_forward(K.ptr(self.q.flat), K.ptr(obs), obs.shape[0], K.ptr(q), self._s()), "mi_ddqn_forward")
        return q.reshape(*lead, 2)
