"""RainbowEngine — Rainbow (Hessel et al. 2018) on CartPole-v1: NoisyDQNEngine over libmirl_rainbow.so (include/mi_rainbow.h).

The networks are two ``RainbowQNetwork``s (36,774 floats: the torso, the means of the noisy value and advantage streams — 51 atoms each — and their sigmas).  The
target is the n-step categorical projection of the target network's distribution of the ONLINE network's greedy action; the loss is the importance-weighted
cross-entropy against it; a row's unweighted cross-entropy is its new replay priority.  ``prio`` (the buffer the priority scatter reads; ``td_abs`` is the same
tensor under the inherited name), ``target_probs`` [batch, 51], ``probs`` [batch, 51] and ``horizon`` are the outputs; ``current`` and ``target_values`` of the
scalar engines are not written.

``act``, ``forward``, ``_batch``, ``target`` and ``train_step`` go through the new library; the sampler, ``beta()``, ``sync_target`` and the priority scatter
are inherited.  ``noisy=False`` is the mean network everywhere.
"""
import ctypes as C
import math

import torch

from . import _native as N
from . import _native_rb as K
from .noisy_engine import NoisyDQNEngine
from .nstep_engine import NStepDQNEngine
from .optim import Adam


class RainbowEngine(NoisyDQNEngine):
    K, ALGO, NEEDS = K, "Rainbow", "two RainbowQNetworks"

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, learning_starts=10_000, start_e=0.0, end_e=0.0,
                 exploration_fraction=0.5, total_timesteps=100_000, max_episodes_logged=None, process_group=None, prioritized=True, alpha=0.6, beta_0=0.4, n_step=3,
                 noisy=True, n_atoms=51, v_min=0.0, v_max=100.0):
        if int(n_atoms) != K.N_ATOMS:
            raise K.MiError("RainbowEngine: the kernels are specialised for n_atoms = %d; %r given" % (K.N_ATOMS, n_atoms))
        self.v_min, self.v_max = float(v_min), float(v_max)
        if not (math.isfinite(self.v_min) and math.isfinite(self.v_max) and self.v_min < self.v_max):
            raise K.MiError("RainbowEngine: the support needs finite v_min < v_max; (%r, %r) given" % (v_min, v_max))
        super().__init__(env, q_network, target_network, optimizer, slots, batch_size, gamma, learning_starts, start_e, end_e, exploration_fraction, total_timesteps,
                         max_episodes_logged, process_group, prioritized, alpha, beta_0, n_step, noisy)
        self.n_atoms = K.N_ATOMS
        self.target_probs = torch.zeros((self.batch_size, K.N_ATOMS), dtype=torch.float32, device=self.device)
        self.probs = torch.zeros((self.batch_size, K.N_ATOMS), dtype=torch.float32, device=self.device)
        self.prio = self.td_abs   # max(row cross-entropy, 0): what _scatter hands to mi_per_update_priorities_sums

    def act(self, n_steps, forced_actions=None, forced_resets=None):
        """NoisyDQNEngine.act through mi_rb_act_steps."""
        dev, gs = self.device, self.global_step
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        if fa is not None and fa.numel() != int(n_steps) * self.N or fr is not None and fr.numel() != int(n_steps) * self.N * 4:
            raise K.MiError("act: forced_actions / forced_resets must be [n_steps, N] / [n_steps, N, 4]")
        if self.prioritized and not 0 < int(n_steps) < self.slots:
            raise K.MiError("act: a prioritized acting call marks the rows it writes and must be shorter than the ring (n_steps in [1, slots))")
        a = K.RBAct(K.ptr(self.q.flat), K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(self.episodes) if self.max_ep else None, K.ptr(self.episode_stats),
                    gs, self.total_timesteps, self.learning_starts, self.start_e, self.end_e, self.exploration_fraction, int(n_steps), self.max_ep,
                    1 if self.noisy else 0, self.v_min, self.v_max, 0)
        K.check(K.lib().mi_rb_act_steps(self.env.handle, C.byref(self._ring), C.byref(a), self._s()), "mi_rb_act_steps")
        self.global_step += int(n_steps)
        if self.prioritized:
            N.check(N.lib().mi_per_mark_sums(N.ptr(self.priorities), self.N, self.slots, gs, int(n_steps), N.ptr(self.max_priority), self.alpha, N.ptr(self._per_ws),
                                             self._s()), "mi_per_mark_sums")

    def _batch(self, upper):
        return K.RBBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.target_probs), K.ptr(self.next_actions),
                         K.ptr(self.probs), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper, self.batch_size,
                         self.gamma, self.mid_event, K.ptr(self.weights) if self.prioritized else None, K.ptr(self.prio), K.ptr(self.horizon), self.n_step,
                         1 if self.noisy else 0, self.global_step % self.slots, self.v_min, self.v_max)

    def train_step(self, indices=None):
        """One optimisation step: NoisyDQNEngine.train_step with mi_rb_update in the place of mi_nz_update (that method names its own binding)."""
        if not self.prioritized:
            return super(NStepDQNEngine, self).train_step(indices)   # RingEngine.train_step, which calls this library through ``K``
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
        """next_actions, target_probs and horizon of batch_inds under the two heads of update ``update_index``."""
        K.target(self._ring, self._batch(0), self._s())

    def forward(self, observation, noise=None, probs=False):
        """the action values [..., 2] of the online network through mi_rb_forward (``probs=True``: ``(probs [..., 2, 51], q)``): the mean network
        (``noise=None``), or every row under the ONE sample ``noise = (a, b, stream)`` of the env's seed, as NoisyDQNEngine.forward"""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        p = torch.empty((obs.shape[0], 2, K.N_ATOMS), dtype=torch.float32, device=self.device) if probs else None
        key = None
        if noise is not None:
            a, b, stream = noise
            if not 0 <= int(stream) < 16:
                raise K.MiError("forward: the noise key's stream must be in [0, 16); %d given" % int(stream))
            key = C.byref(K.RBKey(self.env._seed, int(a), int(b), int(stream), 0))
        K.check(K.lib().mi_rb_forward(K.ptr(self.q.flat), K.ptr(obs), obs.shape[0], key, self.v_min, self.v_max, K.ptr(p), K.ptr(q), self._s()), "mi_rb_forward")
        q = q.reshape(*lead, 2)
        return (p.reshape(*lead, 2, K.N_ATOMS), q) if probs else q
