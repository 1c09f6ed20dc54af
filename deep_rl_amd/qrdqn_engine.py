"""QRDQNEngine — device-resident replay ring + the launch sequence of QR-DQN (include/mi_qr.h).

The surface of C51Engine over libmirl_qr.so: the four replay tensors with c51.py's names plus an env axis, laid out as a [slots, N] time-major ring; methods are
thin launch wrappers, nothing is computed in Python.  Single process only.
"""
import ctypes as C

import torch

from . import _native_qr as K
from . import dist as D
from .optim import Adam


class QRDQNEngine:
    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size=128, gamma=0.99, start_e=1.0, end_e=0.05, exploration_fraction=0.5,
                 total_timesteps=50_000, max_episodes_logged=None, process_group=None):
        if D.world_size(process_group) > 1:
            raise K.MiError("QRDQNEngine runs in a single process (world size %d given): sharding is not built for QR-DQN" % D.world_size(process_group))
        if tuple(env.observation_space.shape) != (4,) or q_network.flat.numel() != K.NPARAMS or target_network.flat.numel() != K.NPARAMS:
            raise K.MiError("QRDQNEngine needs a CartPole env and two QRQNetworks")
        self.env, self.q, self.target_network, self.optimizer = env, q_network, target_network, optimizer   # (`target` is the method below)
        self.N, self.device, self.slots = env.num_envs, env.device, int(slots)
        if self.slots < 2 or int(batch_size) < 1:
            raise K.MiError("QRDQNEngine: slots must be >= 2 and batch_size >= 1")
        self.batch_size, self.gamma = int(batch_size), float(gamma)
        self.total_timesteps = int(total_timesteps)
        self.start_e, self.end_e, self.exploration_fraction = float(start_e), float(end_e), float(exploration_fraction)
        dev, S, Nn, B = self.device, self.slots, self.N, self.batch_size
        self.observations = torch.zeros((S, Nn, 4), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((S, Nn), dtype=torch.int64, device=dev)
        self.rewards = torch.zeros((S, Nn), dtype=torch.float32, device=dev)
        self.terminated = torch.zeros((S, Nn), dtype=torch.uint8, device=dev)
        self.batch_inds = torch.zeros(B, dtype=torch.int64, device=dev)
        self.current = torch.zeros((B, K.N_QUANT), dtype=torch.float32, device=dev)
        self.target_quantiles = torch.zeros((B, K.N_QUANT), dtype=torch.float32, device=dev)
        self.next_actions = torch.zeros(B, dtype=torch.int32, device=dev)
        self.grads = torch.zeros(K.NPARAMS, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.workspace = torch.empty(K.lib().mi_qr_workspace_bytes(B), dtype=torch.uint8, device=dev)
        self.max_ep = int(max_episodes_logged if max_episodes_logged is not None else (1024 if Nn <= 8 else 0))
        self.episodes = torch.zeros((max(self.max_ep, 1), 4), dtype=torch.int32, device=dev)
        self.episode_stats = torch.zeros(4, dtype=torch.int32, device=dev)
        self._ring = K.QRRing(K.ptr(self.observations), K.ptr(self.actions), K.ptr(self.rewards), K.ptr(self.terminated), S, Nn, 0)
        self.observation = None
        self.global_step = 0      # time steps taken (each advances every env once)
        self.update_index = 0
        self.mid_event = None

    def _s(self):
        return K.stream_ptr(self.device)

    def reset(self, forced_state=None):
        """observation = env.reset(); observations[global_step] = observation."""
        self.observation = self.env.reset(forced_state)
        self.observations[self.global_step % self.slots].copy_(self.observation)
        return self.observation

    def act(self, n_steps, forced_actions=None, forced_resets=None):
        """n_steps time steps of every env (epsilon-greedy action through the collapsed head, step, auto-reset, ring store), one launch."""
        dev = self.device
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int64).contiguous()
        fr = None if forced_resets is None else forced_resets.to(dev, torch.float64).contiguous()
        if fa is not None and fa.numel() != int(n_steps) * self.N or fr is not None and fr.numel() != int(n_steps) * self.N * 4:
            raise K.MiError("act: forced_actions / forced_resets must be [n_steps, N] / [n_steps, N, 4]")
        a = K.QRAct(K.ptr(self.q.flat), K.ptr(self.observation), K.ptr(fa), K.ptr(fr), K.ptr(self.episodes) if self.max_ep else None, K.ptr(self.episode_stats),
                    self.global_step, self.total_timesteps, self.start_e, self.end_e, self.exploration_fraction, int(n_steps), self.max_ep)
        K.check(K.lib().mi_qr_act_steps(self.env.handle, C.byref(self._ring), C.byref(a), self._s()), "mi_qr_act_steps")
        self.global_step += int(n_steps)

    def drain_episodes(self):
        """Host sync. -> (count, [(env, step_in_call, return, length)] sorted by (step, env)) of the last act() call."""
        st = self.episode_stats.tolist()
        k = min(st[3], self.max_ep)
        if k == 0:
            return st[0], []
        raw = self.episodes[:k].cpu()
        rets = raw[:, 2].contiguous().view(torch.float32)
        eps = sorted((int(raw[i, 1]), int(raw[i, 0]), float(rets[i]), int(raw[i, 3])) for i in range(k))
        return st[0], [(e, t, r, l) for (t, e, r, l) in eps]

    def _upper(self):
        return min(self.global_step, self.slots) * self.N

    def sample(self, indices=None):
        """batch_inds = np.random.randint(global_step, size=batch_size) under libmirl's keyed stream-4 contract; `indices` keeps the caller's batch."""
        if indices is not None:
            idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).to(self.device)
            if idx.numel() != self.batch_size:
                raise K.MiError("sample: %d indices given, batch_size is %d" % (idx.numel(), self.batch_size))
            self.batch_inds.copy_(idx)
            return
        from . import _native as N
        if self._upper() == 0:
            raise K.MiError("sample: the replay ring is empty (global_step == 0); act() before training")
        N.check(N.lib().mi_dqn_sample(self.env._seed, self.update_index, self._upper(), self.batch_size, N.ptr(self.batch_inds), self._s()), "mi_dqn_sample")

    def _batch(self, upper):
        # mid_event: a torch.cuda.Event's handle to be recorded between the two launches (tools/bench_qrdqn.py); None otherwise
        return K.QRBatch(K.ptr(self.q.flat), K.ptr(self.target_network.flat), K.ptr(self.batch_inds), K.ptr(self.current), K.ptr(self.target_quantiles),
                         K.ptr(self.next_actions), K.ptr(self.grads), K.ptr(self.loss), K.ptr(self.workspace), self.env._seed, self.update_index, upper,
                         self.batch_size, self.gamma, self.mid_event)

    def target(self):
        """next_actions / target_quantiles of batch_inds from the target network."""
        b = self._batch(0)
        K.check(K.lib().mi_qr_target(C.byref(self._ring), C.byref(b), self._s()), "mi_qr_target")

    def grad(self):
        """loss + gradient of batch_inds -> self.grads, self.loss (and target_quantiles, next_actions, current)."""
        b = self._batch(0)
        K.check(K.lib().mi_qr_grad(C.byref(self._ring), C.byref(b), self._s()), "mi_qr_grad")

    def train_step(self, indices=None):
        """One optimisation step.  With deep_rl_amd.Adam: ONE call, two launches — the gradient launch draws the batch itself and the launch that sums the slabs
        applies Adam (mi_qr_update, bit-identical to sample() + grad() + optimizer.step())."""
        o = self.optimizer
        if type(o) is Adam and o.flat.data_ptr() == self.q.flat.data_ptr():
            upper = 0
            if indices is None:
                upper = self._upper()
                if upper == 0:
                    raise K.MiError("train_step: the replay ring is empty (global_step == 0); act() before training")
            else:
                self.sample(indices)
            g = o.param_groups[0]
            b = self._batch(upper)
            a = K.QRAdam(K.ptr(o.exp_avg), K.ptr(o.exp_avg_sq), o.step_count + 1, float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"])
            K.check(K.lib().mi_qr_update(C.byref(self._ring), C.byref(b), C.byref(a), self._s()), "mi_qr_update")
            o.step_count += 1   # committed only once the call has accepted the step
        else:
            self.sample(indices)
            self.grad()
            o.step(self.grads)
        self.update_index += 1

    def sync_target(self):
        """target_network.load_state_dict(q_network.state_dict())."""
        self.target_network.flat.copy_(self.q.flat)
