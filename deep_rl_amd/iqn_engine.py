"""IQNEngine — the launch sequence of reference iqn.py:185-299 (re-targeted to CartPole-v1) over libmirl_iqn.so (include/mi_iqn.h).

The surface of C51Engine: the replay ring and everything around it is RingEngine's (_ring_engine.py); this file adds IQN's epsilon schedule, its tau and quantile
tensors, the teacher forcing of the taus and the two calls whose arguments are the library's own.
"""
import ctypes as C
from types import SimpleNamespace

import torch

from . import _native_iqn as K
from ._ring_engine import RingEngine


class IQNEngine(RingEngine):
    K, ALGO, NEEDS = K, "IQN", "two packed IQN parameter buffers of %d floats" % K.NPARAMS

    def __init__(self, env, params, target_params, optimizer, slots, batch_size=32, gamma=0.99, final_epsilon=0.01, epsilon_decay_steps=10_000, learning_starts=1_000,
                 max_episodes_logged=None, process_group=None):
        """params / target_params: the packed 44,898-float buffers of the three online / target modules (``pack(features_extractor, cosine_net, quantile_net)``)."""
        super().__init__(env, SimpleNamespace(flat=params), SimpleNamespace(flat=target_params), optimizer, slots, batch_size, gamma, max_episodes_logged, process_group)
        self.final_epsilon, self.learning_starts = float(final_epsilon), int(learning_starts)
        self.slope = -(1.0 - self.final_epsilon) / epsilon_decay_steps   # iqn.py:123
        dev, B = self.device, self.batch_size
        self.taus = torch.zeros((B, K.N_TAU), dtype=torch.float32, device=dev)
        self.current_action_quantiles = torch.zeros((B, K.N_TAU), dtype=torch.float32, device=dev)
        self.target_action_quantiles = torch.zeros((B, K.N_TAU_PRIME), dtype=torch.float32, device=dev)
        self._forced = (None, None, None)

    def act(self, n_steps, forced_actions=None, forced_resets=None, forced_taus=None, taus_out=None):
        """n_steps iterations of iqn.py:185-217 for every env, one launch.  taus_out: f32 [n_steps, N, 32] device tensor that receives the taus of the greedy steps."""
        dev, n = self.device, int(n_steps)
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        ft = None if forced_taus is None else forced_taus.to(dev, torch.float32).contiguous()
        if (fa is not None and fa.numel() != n * self.N) or (fr is not None and fr.numel() != n * self.N * 4) or (ft is not None and ft.numel() != n * self.N * K.N_QUANT):
            raise K.MiError("act: forced_actions / forced_resets / forced_taus must be [n_steps, N] / [n_steps, N, 4] / [n_steps, N, 32]")
        if taus_out is not None and (taus_out.dtype != torch.float32 or taus_out.device != self.observation.device or not taus_out.is_contiguous() or taus_out.numel() != n * self.N * K.N_QUANT):
            raise K.MiError("act: taus_out must be a contiguous f32 device tensor of [n_steps, N, 32]")
        a = K.IQNAct(K.ptr(self.q.flat), K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(ft), K.ptr(taus_out), K.ptr(self.episodes) if self.max_ep else None,
                     K.ptr(self.episode_stats), self.global_step, self.learning_starts, self.slope, self.final_epsilon, n, self.max_ep)
        K.check(K.lib().mi_iqn_act_steps(self.env.handle, C.byref(self._ring), C.byref(a), self._s()), "mi_iqn_act_steps")
        self.global_step += n

    def force_taus(self, taus=None, next_taus=None, tau_dashes=None):
        """Teacher forcing: [B, 64] / [B, 32] / [B, 64] tau draws used by target() / grad() / train_step() until cleared with force_taus()."""
        shapes = ((self.batch_size, K.N_TAU), (self.batch_size, K.N_QUANT), (self.batch_size, K.N_TAU_PRIME))
        out = []
        for v, shp in zip((taus, next_taus, tau_dashes), shapes):
            if v is not None:
                v = torch.as_tensor(v, dtype=torch.float32).to(self.device).contiguous()
                if tuple(v.shape) != shp:
                    raise K.MiError("force_taus: shape %s given, %s needed" % (tuple(v.shape), shp))
            out.append(v)
        self._forced = tuple(out)

    def _batch(self, upper):
        f = self._forced
        return K.IQNBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(f[0]), K.ptr(f[1]), K.ptr(f[2]), K.ptr(self.taus),
                          K.ptr(self.current_action_quantiles), K.ptr(self.target_action_quantiles), K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss),
                          K.ptr(self.workspace), self.env._seed, self.update_index, upper, self.batch_size, self.gamma, self.mid_event)

    def target(self):
        """next_actions / target_action_quantiles of batch_inds from the target networks (iqn.py:252-278)."""
        b = self._batch(0)
        K.check(K.lib().mi_iqn_target(C.byref(self._ring), C.byref(b), self._s()), "mi_iqn_target")
