"""NStepDQNEngine — prioritized dueling Double DQN with n-step returns: PDDDQNEngine trained through libmirl_nstep.so (include/mi_nstep.h).

Multi-step returns change the target and nothing else, so everything but the three training calls is PDDDQNEngine's, unchanged: ``act`` and ``forward`` go through
libmirl_pdd.so on the same ring and the same 11,019-float vectors, ``sample``, the priority bookkeeping and ``beta()`` drive libmirl's prioritized sampler, and
``prioritized=False`` gives uniform replay.  This file supplies ``_batch`` (PDD's batch plus ``horizon``, ``n_step`` and the head slot ``global_step % slots`` at
the time of the call), ``target``, ``grad`` and ``train_step`` through the new library, and the ``horizon`` tensor: the number of steps each row's walk took.
With ``n_step=1`` every output is PDDDQNEngine's bit for bit.
"""
import torch

from . import _native_ns as K
from .optim import Adam
from .pdd_engine import PDDDQNEngine


class NStepDQNEngine(PDDDQNEngine):
    K, ALGO, NEEDS = K, "n-step dueling Double DQN", "two DuelingQNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, learning_starts=10_000, start_e=1.0, end_e=0.05,
                 exploration_fraction=0.5, total_timesteps=100_000, max_episodes_logged=None, process_group=None, prioritized=True, alpha=0.6, beta_0=0.4, n_step=3):
        self.n_step = int(n_step)
        if not 1 <= self.n_step <= K.MAX_N or self.n_step >= int(slots):
            raise K.MiError("NStepDQNEngine: n_step must be in [1, %d] and below slots (%d); %d given" % (K.MAX_N, int(slots), self.n_step))
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, learning_starts, start_e, end_e, exploration_fraction, total_timesteps,
                         max_episodes_logged, process_group, prioritized, alpha, beta_0)
        self.horizon = torch.zeros(self.batch_size, dtype=torch.int32, device=self.device)

    def _batch(self, upper):
        return K.NSBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.current), K.ptr(self.target_values),
                         K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper,
                         self.batch_size, self.gamma, self.mid_event, K.ptr(self.weights) if self.prioritized else None, K.ptr(self.td_abs), K.ptr(self.horizon),
                         self.n_step, self.global_step % self.slots)

    def train_step(self, indices=None):
        """One optimisation step: PDDDQNEngine.train_step with mi_ns_update in the place of mi_pdd_update.  Uniform: RingEngine.train_step (it calls this library
        through ``K``).  Prioritized with deep_rl_amd.Adam: the sampler, mi_ns_update (two launches), the priority scatter; bit-identical to sample() + grad() +
        optimizer.step()."""
        if not self.prioritized:
            return super().train_step(indices)
        o = self.optimizer
        self.sample(indices)
        if type(o) is Adam and o.flat.data_ptr() == self.q.flat.data_ptr():
            g = o.param_groups[0]
            a = K.AdamArgs(K.ptr(o.exp_avg), K.ptr(o.exp_avg_sq), o.step_count + 1, float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"])
            K.update(self._ring, self._batch(0), a, self._s())
            o.step_count += 1   # committed only once the call has accepted the step
            self._scatter()
        else:
            self.grad()
            o.step(self.grads)
        self.update_index += 1

    def target(self):
        """next_actions (the online network's greedy action at the bootstrap observation), target_values (the n-step target) and horizon of batch_inds."""
        K.target(self._ring, self._batch(0), self._s())
