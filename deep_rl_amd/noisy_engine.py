"""NoisyDQNEngine — n-step prioritized dueling Double DQN that explores with noisy networks: NStepDQNEngine over libmirl_noisy.so (include/mi_noisy.h).

The networks are two ``NoisyDuelingQNetwork``s (11,274 floats: the dueling vector and, behind it, the head's sigma).  With ``noisy=True`` every greedy env step of
the acting launch draws its own head (stream 13, keyed by the env's id and step counter) and every update draws one online and one target head (stream 14, keyed by
the update index); nothing new is carried between calls, so a checkpoint needs nothing new either.  ``start_e = end_e = 0.0`` by default: the noise is the
exploration.  The epsilon table and the ``learning_starts`` clause still work when set.  ``noisy=False`` is the mean network everywhere — the evaluation mode, and
NStepDQNEngine bit for bit on the first 11,019 floats.

``act``, ``forward``, ``_batch``, ``target`` and ``train_step`` go through the new library; the sampler, the priority bookkeeping, ``beta()`` and ``sync_target``
are inherited.
"""
import ctypes as C

import torch

from . import _native as N
from . import _native_nz as K
from .nstep_engine import NStepDQNEngine
from .optim import Adam


class NoisyDQNEngine(NStepDQNEngine):
    K, ALGO, NEEDS = K, "noisy n-step dueling Double DQN", "two NoisyDuelingQNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, learning_starts=10_000, start_e=0.0, end_e=0.0,
                 exploration_fraction=0.5, total_timesteps=100_000, max_episodes_logged=None, process_group=None, prioritized=True, alpha=0.6, beta_0=0.4, n_step=3,
                 noisy=True):
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, learning_starts, start_e, end_e, exploration_fraction, total_timesteps,
                         max_episodes_logged, process_group, prioritized, alpha, beta_0, n_step)
        self.noisy = bool(noisy)

    def act(self, n_steps, forced_actions=None, forced_resets=None):
        """PDDDQNEngine.act through mi_nz_act_steps: with ``noisy`` every greedy step evaluates a head drawn for that (env, step)."""
        dev, gs = self.device, self.global_step
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        if fa is not None and fa.numel() != int(n_steps) * self.N or fr is not None and fr.numel() != int(n_steps) * self.N * 4:
            raise K.MiError("act: forced_actions / forced_resets must be [n_steps, N] / [n_steps, N, 4]")
        if self.prioritized and not 0 < int(n_steps) < self.slots:
            raise K.MiError("act: a prioritized acting call marks the rows it writes and must be shorter than the ring (n_steps in [1, slots))")
        a = K.NZAct(K.ptr(self.q.flat), K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(self.episodes) if self.max_ep else None, K.ptr(self.episode_stats),
                    gs, self.total_timesteps, self.learning_starts, self.start_e, self.end_e, self.exploration_fraction, int(n_steps), self.max_ep,
                    1 if self.noisy else 0, 0)
        K.check(K.lib().mi_nz_act_steps(self.env.handle, C.byref(self._ring), C.byref(a), self._s()), "mi_nz_act_steps")
        self.global_step += int(n_steps)
        if self.prioritized:
            N.check(N.lib().mi_per_mark_sums(N.ptr(self.priorities), self.N, self.slots, gs, int(n_steps), N.ptr(self.max_priority), self.alpha, N.ptr(self._per_ws),
                                             self._s()), "mi_per_mark_sums")

    def _batch(self, upper):
        return K.NZBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.current), K.ptr(self.target_values),
                         K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper,
                         self.batch_size, self.gamma, self.mid_event, K.ptr(self.weights) if self.prioritized else None, K.ptr(self.td_abs), K.ptr(self.horizon),
                         self.n_step, self.global_step % self.slots, 1 if self.noisy else 0, 0)

    def train_step(self, indices=None):
        """One optimisation step: NStepDQNEngine.train_step with mi_nz_update in the place of mi_ns_update; the two heads of update ``update_index`` are drawn in
        the gradient launch."""
        if not self.prioritized:
            return super(NStepDQNEngine, self).train_step(indices)   # PDDDQNEngine's uniform branch: RingEngine.train_step, which calls this library through ``K``
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
        """next_actions, target_values and horizon of batch_inds under the two heads of update ``update_index``."""
        K.target(self._ring, self._batch(0), self._s())

    def forward(self, observation, noise=None):
        """the action values [..., 2] of the online network through mi_nz_forward: the mean network (``noise=None``), or every row under the ONE sample
        ``noise = (a, b, stream)`` of the env's seed — (env_id, step counter, 13) is what an acting step used, (update, 0, 14) an update's online network"""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        key = None
        if noise is not None:
            a, b, stream = noise
            if not 0 <= int(stream) < 16:
                raise K.MiError("forward: the noise key's stream must be in [0, 16); %d given" % int(stream))
            key = C.byref(K.NZKey(self.env._seed, int(a), int(b), int(stream), 0))
        K.check(K.lib().mi_nz_forward(K.ptr(self.q.flat), K.ptr(obs), obs.shape[0], key, K.ptr(q), self._s()), "mi_nz_forward")
        return q.reshape(*lead, 2)
