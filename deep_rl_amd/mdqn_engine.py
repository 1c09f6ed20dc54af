"""MunchausenDQNEngine — Munchausen DQN (Vieillard, Pietquin, Geist 2020): DoubleDQNEngine trained through libmirl_mdqn.so (include/mi_mdqn.h).

Munchausen DQN changes the target of plain DQN and nothing else, so everything but the three training calls is DoubleDQNEngine's, unchanged: ``act`` and ``forward``
go through libmirl_ddqn.so on the same ring and the same 10,934-float vectors of two plain ``QNetwork``s.  This file supplies ``_batch`` (Double DQN's batch plus
``bonus``, ``soft_value`` and the three hyper-parameters), ``target``, and the ``bonus`` / ``soft_value`` tensors; ``grad`` and ``train_step`` are RingEngine's and
reach the new library through ``K``.  ``next_actions`` is the TARGET network's greedy action at the successor here, a diagnostic.  With ``alpha=0``, a ``tau`` small
enough that the soft-max is a hard max in fp32, and synced networks every output is DoubleDQNEngine's bit for bit.
"""
import math

import torch

from . import _native_md as K
from .ddqn_engine import DoubleDQNEngine


class MunchausenDQNEngine(DoubleDQNEngine):
    K, ALGO, NEEDS = K, "Munchausen DQN", "two QNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, learning_starts=10_000, start_e=1.0, end_e=0.05,
                 exploration_fraction=0.5, total_timesteps=100_000, max_episodes_logged=None, process_group=None, alpha=0.9, tau=0.03, clip_lo=-1.0):
        self.alpha, self.tau, self.clip_lo = float(alpha), float(tau), float(clip_lo)
        if not (self.tau > 0.0 and math.isfinite(self.tau) and math.isfinite(self.alpha) and self.clip_lo <= 0.0):
            raise K.MiError("MunchausenDQNEngine: tau must be > 0 and finite, alpha finite and clip_lo <= 0; (%r, %r, %r) given" % (tau, alpha, clip_lo))
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, learning_starts, start_e, end_e, exploration_fraction, total_timesteps,
                         max_episodes_logged, process_group)
        self.bonus = torch.zeros(self.batch_size, dtype=torch.float32, device=self.device)
        self.soft_value = torch.zeros(self.batch_size, dtype=torch.float32, device=self.device)

    def _batch(self, upper):
        return K.MDBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.current), K.ptr(self.target_values),
                         K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper,
                         self.batch_size, self.gamma, self.mid_event, K.ptr(self.bonus), K.ptr(self.soft_value), self.alpha, self.tau, self.clip_lo)

    def target(self):
        """bonus (the target network's clipped tau ln pi of the stored action), soft_value (its soft value at the successor), next_actions (its greedy action
        there) and target_values of batch_inds: the gradient launch's first pass alone."""
        K.target(self._ring, self._batch(0), self._s())
