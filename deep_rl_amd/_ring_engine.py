"""RingEngine — what C51Engine, IQNEngine and QRDQNEngine have in common: the device-resident replay ring and the launch sequence around it.

The four replay tensors with the reference's names (c51.py:80-83, iqn.py:174-177) plus an env axis, laid out as a [slots, N] time-major ring; methods are thin launch
wrappers, nothing is computed in Python.  Single process only.

A subclass names its binding module (``K``, one of _native_c51 / _native_iqn / _native_qr: the library's ``Ring`` / ``Batch`` / ``AdamArgs`` structs and its
``workspace_bytes`` / ``grad`` / ``update`` calls) and itself (``ALGO``, ``NEEDS``: error texts), allocates its own output tensors, and supplies ``_batch(upper)``,
``act(...)`` and ``target()``.
"""
import torch

from . import dist as D
from .optim import Adam


class RingEngine:
    K = None       # the binding module
    ALGO = None    # "C51": sharding is not built for ...
    NEEDS = None   # "two C51QNetworks": <class> needs a CartPole env and ...

    def __init__(self, env, q_network, target_network, optimizer, slots, batch_size, gamma, max_episodes_logged, process_group):
        K, name = self.K, type(self).__name__
        if D.world_size(process_group) > 1:
            raise K.MiError("%s runs in a single process (world size %d given): sharding is not built for %s" % (name, D.world_size(process_group), self.ALGO))
        if tuple(env.observation_space.shape) != (4,) or q_network.flat.numel() != K.NPARAMS or target_network.flat.numel() != K.NPARAMS:
            raise K.MiError("%s needs a CartPole env and %s" % (name, self.NEEDS))
        self.env, self.q, self.target_network, self.optimizer = env, q_network, target_network, optimizer   # (`target` is the subclass's method)
        self.N, self.device, self.slots = env.num_envs, env.device, int(slots)
        if self.slots < 2 or int(batch_size) < 1:
            raise K.MiError("%s: slots must be >= 2 and batch_size >= 1" % name)
        self.batch_size, self.gamma = int(batch_size), float(gamma)
        dev, S, Nn, B = self.device, self.slots, self.N, self.batch_size
        self.observations = torch.zeros((S, Nn, 4), dtype=torch.float32, device=dev)   # c51.py:80, iqn.py:174 (f32: no uint8 storage, no / 255)
        self.actions = torch.zeros((S, Nn), dtype=torch.int64, device=dev)             # :81
        self.rewards = torch.zeros((S, Nn), dtype=torch.float32, device=dev)           # :82
        self.terminated = torch.zeros((S, Nn), dtype=torch.uint8, device=dev)          # :83 (bool)
        self.batch_inds = torch.zeros(B, dtype=torch.int64, device=dev)
        self.next_actions = torch.zeros(B, dtype=torch.int32, device=dev)
        self.grads = torch.zeros(K.NPARAMS, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.workspace = torch.empty(K.workspace_bytes(B), dtype=torch.uint8, device=dev)
        self.max_ep = int(max_episodes_logged if max_episodes_logged is not None else (1024 if Nn <= 8 else 0))
        self.episodes = torch.zeros((max(self.max_ep, 1), 4), dtype=torch.int32, device=dev)
        self.episode_stats = torch.zeros(4, dtype=torch.int32, device=dev)
        self._ring = K.Ring(K.ptr(self.observations), K.ptr(self.actions), K.ptr(self.rewards), K.ptr(self.terminated), S, Nn, 0)
        self.observation = None
        self.global_step = 0      # time steps taken (each advances every env once)
        self.update_index = 0
        self.mid_event = None     # a torch.cuda.Event's handle to be recorded between the two launches of grad() / train_step() (tools/bench_*.py); None otherwise

    def _s(self):
        return self.K.stream_ptr(self.device)

    def reset(self, forced_state=None):
        """observation = env.reset(); observations[global_step % slots] = observation (c51.py:86-88, iqn.py:180-182)."""
        self.observation = self.env.reset(forced_state)
        self.observations[self.global_step % self.slots].copy_(self.observation)
        return self.observation

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
        return min(self.global_step, self.slots) * self.N   # iqn.py:225

    def sample(self, indices=None):
        """batch_inds = np.random.randint(upper, size=batch_size) (c51.py:124, iqn.py:226) under libmirl's keyed stream-4 contract; `indices` keeps the caller's batch."""
        if indices is not None:
            idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).to(self.device)
            if idx.numel() != self.batch_size:
                raise self.K.MiError("sample: %d indices given, batch_size is %d" % (idx.numel(), self.batch_size))
            self.batch_inds.copy_(idx)
            return
        from . import _native as N
        if self._upper() == 0:
            raise self.K.MiError("sample: the replay ring is empty (global_step == 0); act() before training")
        N.check(N.lib().mi_dqn_sample(self.env._seed, self.update_index, self._upper(), self.batch_size, N.ptr(self.batch_inds), self._s()), "mi_dqn_sample")

    def grad(self):
        """loss + gradient of batch_inds -> self.grads, self.loss (and the subclass's target / current tensors, next_actions)."""
        self.K.grad(self._ring, self._batch(0), self._s())

    def train_step(self, indices=None):
        """One optimisation step (c51.py:124-163, iqn.py:225-293).  With deep_rl_amd.Adam: ONE call, two launches — the gradient launch draws the batch (and IQN's
        taus) itself and the launch that sums the slabs applies Adam (mi_*_update, bit-identical to sample() + grad() + optimizer.step())."""
        K, o = self.K, self.optimizer
        if type(o) is Adam and o.flat.data_ptr() == self.q.flat.data_ptr():
            upper = 0
            if indices is None:
                upper = self._upper()
                if upper == 0:
                    raise K.MiError("train_step: the replay ring is empty (global_step == 0); act() before training")
            else:
                self.sample(indices)
            g = o.param_groups[0]
            a = K.AdamArgs(K.ptr(o.exp_avg), K.ptr(o.exp_avg_sq), o.step_count + 1, float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"])
            K.update(self._ring, self._batch(upper), a, self._s())
            o.step_count += 1   # committed only once the call has accepted the step
        else:
            self.sample(indices)
            self.grad()
            o.step(self.grads)
        self.update_index += 1

    def sync_target(self):
        """target_network.load_state_dict(q_network.state_dict()) (c51.py:166-167; IQN: the three modules, iqn.py:296-299)."""
        self.target_network.flat.copy_(self.q.flat)
