"""C51Engine — the launch sequence of reference c51.py:91-167 over libmirl_c51.so (include/mi_c51.h).

The surface of DQNEngine: the replay ring and everything around it is RingEngine's (_ring_engine.py); this file adds C51's epsilon schedule, its output tensors and
the three calls whose arguments are the library's own.
"""
import ctypes as C

import torch

from . import _native_c51 as K
from ._ring_engine import RingEngine


class C51Engine(RingEngine):
    K, ALGO, NEEDS = K, "C51", "two C51QNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, start_e=1.0, end_e=0.05, exploration_fraction=0.5,
                 total_timesteps=20_000, max_episodes_logged=None, process_group=None):
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, max_episodes_logged, process_group)
        self.total_timesteps = int(total_timesteps)
        self.start_e, self.end_e, self.exploration_fraction = float(start_e), float(end_e), float(exploration_fraction)
        self.target_probs = torch.zeros((self.batch_size, K.N_ATOMS), dtype=torch.float32, device=self.device)
        self.probs = torch.zeros((self.batch_size, K.N_ATOMS), dtype=torch.float32, device=self.device)

    def act(self, n_steps, forced_actions=None, forced_resets=None):
        """n_steps iterations of c51.py:91-116 for every env, one launch."""
        dev = self.device
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        if fa is not None and fa.numel() != int(n_steps) * self.N or fr is not None and fr.numel() != int(n_steps) * self.N * 4:
            raise K.MiError("act: forced_actions / forced_resets must be [n_steps, N] / [n_steps, N, 4]")
        K.check(K.lib().mi_c51_act_steps(
            self.env.handle, K.ptr(self.q.flat), int(n_steps), self.global_step, C.byref(self._ring), self.start_e, self.end_e, self.exploration_fraction,
            self.total_timesteps, K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(self.episodes) if self.max_ep else None, K.ptr(self.episode_stats),
            self.max_ep, self._s()), "mi_c51_act_steps")
        self.global_step += int(n_steps)

    def _batch(self, upper):
        return K.C51Batch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.target_probs), K.ptr(self.next_actions), K.ptr(self.probs),
                          K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper, self.batch_size, self.gamma, self.mid_event)

    def target(self):
        """next_actions / target_probs of batch_inds from the target network (c51.py:132-154)."""
        K.check(K.lib().mi_c51_target(K.ptr(self.target_network.flat), C.byref(self._ring), K.ptr(self.batch_inds), self.batch_size, self.gamma, K.ptr(self.next_actions),
                                      K.ptr(self.target_probs), self._s()), "mi_c51_target")
