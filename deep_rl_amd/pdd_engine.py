"""PDDDQNEngine — the launch sequence of prioritized dueling Double DQN over libmirl_pdd.so (include/mi_pdd.h).

The surface of DoubleDQNEngine: the replay ring and everything around it is RingEngine's (_ring_engine.py); this file adds DQN's epsilon schedule and its
``learning_starts`` clause, the output tensors, the calls whose arguments are the library's own and — with ``prioritized=True`` — the priorities ring of
PERDQNEngine, driven through libmirl's incremental sampler (mi_per_mark_sums / mi_per_sample_current / mi_per_update_priorities_sums) unchanged.  The networks are
two ``DuelingQNetwork``s of which only ``.flat`` is used: the kernels evaluate the dueling head itself, so ``.eff`` is never read and never needs ``repack()`` here.
"""
import ctypes as C

import torch

from . import _native as N
from . import _native_pdd as K
from ._ring_engine import RingEngine
from .optim import Adam


class PDDDQNEngine(RingEngine):
    K, ALGO, NEEDS = K, "prioritized dueling Double DQN", "two DuelingQNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, learning_starts=10_000, start_e=1.0, end_e=0.05,
                 exploration_fraction=0.5, total_timesteps=100_000, max_episodes_logged=None, process_group=None, prioritized=True, alpha=0.6, beta_0=0.4):
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, max_episodes_logged, process_group)
        self.total_timesteps, self.learning_starts = int(total_timesteps), int(learning_starts)
        self.start_e, self.end_e, self.exploration_fraction = float(start_e), float(end_e), float(exploration_fraction)
        dev, S, Nn = self.device, self.slots, self.N
        self.current = torch.zeros(self.batch_size, dtype=torch.float32, device=dev)
        self.target_values = torch.zeros(self.batch_size, dtype=torch.float32, device=dev)
        self.td_abs = torch.zeros(self.batch_size, dtype=torch.float32, device=dev)
        self.prioritized, self.alpha, self.beta_0 = bool(prioritized), float(alpha), float(beta_0)
        if self.prioritized:   # what PERDQNEngine.__init__ allocates
            self.priorities = torch.zeros((S, Nn), dtype=torch.float32, device=dev)             # per.py:79
            self.max_priority = torch.full((1,), 1e-2, dtype=torch.float32, device=dev)         # :84
            self.weights = torch.zeros(self.batch_size, dtype=torch.float32, device=dev)
            self._owner = torch.full((S * Nn,), -1, dtype=torch.int32, device=dev)
            # the sampler's chunk sums, kept current by mark / update_priorities (zero-filled = current for the zero-filled ring)
            self._per_ws = torch.zeros(N.lib().mi_per_workspace_bytes(S * Nn), dtype=torch.uint8, device=dev)

    def refresh_sums(self):
        """Rebuild the sampler's chunk sums from `priorities` (after anything but act / train_step wrote them: checkpoint load, tests)."""
        if self.prioritized:
            N.check(N.lib().mi_per_sums_refresh(N.ptr(self.priorities), self.slots * self.N, self.alpha, N.ptr(self._per_ws), self._s()), "mi_per_sums_refresh")

    def act(self, n_steps, forced_actions=None, forced_resets=None):
        """n_steps time steps of every env (the keyed random action before learning_starts, epsilon-greedy through the online network after it, step, auto-reset,
        ring store), one launch; prioritized: one more, which gives the new rows the running max_priority (per.py:105) and rebuilds the touched sums."""
        dev, gs = self.device, self.global_step
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        if fa is not None and fa.numel() != int(n_steps) * self.N or fr is not None and fr.numel() != int(n_steps) * self.N * 4:
            raise K.MiError("act: forced_actions / forced_resets must be [n_steps, N] / [n_steps, N, 4]")
        if self.prioritized and not 0 < int(n_steps) < self.slots:
            raise K.MiError("act: a prioritized acting call marks the rows it writes and must be shorter than the ring (n_steps in [1, slots))")
        a = K.PDDAct(K.ptr(self.q.flat), K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(self.episodes) if self.max_ep else None, K.ptr(self.episode_stats),
                     gs, self.total_timesteps, self.learning_starts, self.start_e, self.end_e, self.exploration_fraction, int(n_steps), self.max_ep)
        K.check(K.lib().mi_pdd_act_steps(self.env.handle, C.byref(self._ring), C.byref(a), self._s()), "mi_pdd_act_steps")
        self.global_step += int(n_steps)
        if self.prioritized:
            N.check(N.lib().mi_per_mark_sums(N.ptr(self.priorities), self.N, self.slots, gs, int(n_steps), N.ptr(self.max_priority), self.alpha, N.ptr(self._per_ws),
                                             self._s()), "mi_per_mark_sums")

    def beta(self):
        """per.py:126: beta starts at beta_0 and increases linearly to 1."""
        return (1 - self.beta_0) * self.global_step / self.total_timesteps + self.beta_0

    def sample(self, indices=None):
        """prioritized: batch_inds ~ priorities ** alpha and the importance weights (PERDQNEngine.sample); `indices` keeps the caller's batch and weighs it.
        uniform: RingEngine.sample."""
        if not self.prioritized:
            return super().sample(indices)
        stored = self._upper()
        if stored == 0:
            raise K.MiError("sample: the replay ring is empty (global_step == 0); act() before training")
        if indices is not None:
            super().sample(indices)
        N.check(N.lib().mi_per_sample_current(self.env._seed, self.update_index, N.ptr(self.priorities), stored, self.slots * self.N, float(stored), self.alpha,
                                              self.beta(), self.batch_size, 0 if indices is not None else 1, N.ptr(self._per_ws), N.ptr(self.batch_inds),
                                              N.ptr(self.weights), self._s()), "mi_per_sample_current")

    def _batch(self, upper):
        return K.PDDBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.current), K.ptr(self.target_values),
                          K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper,
                          self.batch_size, self.gamma, self.mid_event, K.ptr(self.weights) if self.prioritized else None, K.ptr(self.td_abs))

    def _scatter(self):
        """priorities[batch_inds] = |td| (the last duplicate wins), max_priority = max(max_priority, |td|), the sums of the touched chunks (per.py:141-145)"""
        N.check(N.lib().mi_per_update_priorities_sums(N.ptr(self.priorities), N.ptr(self.batch_inds), N.ptr(self.td_abs), self.batch_size, N.ptr(self._owner),
                                                      N.ptr(self.max_priority), self.slots * self.N, self.alpha, N.ptr(self._per_ws), self._s()),
                "mi_per_update_priorities_sums")

    def grad(self):
        """weighted loss + gradient + |td| of batch_inds -> self.grads, self.loss, self.td_abs (and target_values, current, next_actions); prioritized: then the
        priority scatter"""
        super().grad()
        if self.prioritized:
            self._scatter()

    def train_step(self, indices=None):
        """One optimisation step.  Uniform: RingEngine.train_step (one call, two launches, the batch drawn in the gradient launch).  Prioritized with
        deep_rl_amd.Adam: the sampler, mi_pdd_update (two launches), the priority scatter; bit-identical to sample() + grad() + optimizer.step()."""
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
        """next_actions (the online network's greedy action at the successor) / target_values (the target network's value of it) of batch_inds."""
        b = self._batch(0)
        K.check(K.lib().mi_pdd_target(C.byref(self._ring), C.byref(b), self._s()), "mi_pdd_target")

    def forward(self, observation):
        """the action values [..., 2] of the online network through mi_pdd_forward: the values the acting and the gradient launch compare"""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        K.check(K.lib().mi_pdd_forward(K.ptr(self.q.flat), K.ptr(obs), obs.shape[0], K.ptr(q), self._s()), "mi_pdd_forward")
        return q.reshape(*lead, 2)
