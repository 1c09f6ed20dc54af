"""ReinforceEngine — the reference's REINFORCE loop (reinforce.py:51-77) with an env axis, on the kernels of libmirl_pg.so (include/mi_reinforce.h).

One UPDATE = every one of the N envs plays ONE episode from a fresh reset to its own done (termination, or TimeLimit truncation at 500 steps), then one
optimizer step on  sum_n sum_t -log_prob[n, t] * Rn[n, t]  with the returns normalised per episode.  At N = 1 that is the reference line for line.

    rollout()          mi_pg_rollout_episodes   reinforce.py:53-66   (one launch; reset, act with live dropout, step, store)
    compute_returns()  mi_pg_returns            :67,71-73
    grad()             mi_pg_grad               :74-76               (deterministic: per-workgroup slabs + a fixed-order sum)
    optimizer_step()   optimizer.step(grads)    :77                  (optim.Adam: libmirl's mi_adam — the same element step as the fused path)
    update()           mi_pg_update             all of the above in one host call (four launches, no host sync), bit-identical to the pieces
"""
import ctypes as C

import torch

from . import _native as N
from . import _native_pg as PG


class ReinforceEngine:
    def __init__(self, env, agent, optimizer, gamma=0.99):
        if getattr(env.spec, "id", None) != "CartPole-v1":
            raise N.MiError("ReinforceEngine is specialised for CartPole-v1")
        if agent.flat.numel() != PG.NPARAMS:
            raise N.MiError("ReinforceEngine needs a DropoutPolicy (898 parameters); got %d" % agent.flat.numel())
        PG.lib()   # a missing libmirl_pg.so is an error here, not at the first launch
        self.env, self.agent, self.optimizer = env, agent, optimizer
        self.gamma = float(gamma)
        self.device = dev = env.device
        self.num_envs = n = env.num_envs
        f32 = dict(dtype=torch.float32, device=dev)
        self.observations = torch.zeros((n, PG.ROWS, 4), **f32)
        self.actions = torch.zeros((n, PG.ROWS), dtype=torch.int32, device=dev)
        self.log_probs = torch.zeros((n, PG.ROWS), **f32)
        self.returns = torch.zeros((n, PG.ROWS), **f32)       # raw R, the reference's global `returns`
        self.b_returns = torch.zeros((n, PG.ROWS), **f32)     # normalised per episode (:73)
        self.mask_bits = torch.zeros((n, PG.ROWS, 4), dtype=torch.int32, device=dev)   # 128 keep bits per row: unit u = bit (u & 31) of word u >> 5
        self.lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        self.episodic_returns = torch.zeros(n, **f32)
        self.grads = torch.zeros(PG.NPARAMS, **f32)
        self.workspace = torch.empty(PG.lib().mi_pg_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.observation = self.observations[:, 0]   # the first observation of the last episodes (kept for the checkpoint format)
        self.update_index = 0

    def _s(self):
        return N.stream_ptr(self.device)

    def _buffers(self, forced_reset=None, forced_actions=None, forced_masks=None):
        o = self.optimizer
        return PG.PGBuffers(*[N.ptr(t) for t in (
            self.agent.flat, getattr(o, "exp_avg", None), getattr(o, "exp_avg_sq", None), self.grads, self.observations, self.actions, self.log_probs,
            self.returns, self.b_returns, self.mask_bits, self.lengths, self.episodic_returns, self.workspace, forced_reset, forced_actions, forced_masks)])

    def reset(self):
        """Clears the storage.  The reference resets the env inside its episode loop (reinforce.py:56); here the episode kernel does, so there is no env call."""
        for t in (self.observations, self.actions, self.log_probs, self.returns, self.b_returns, self.mask_bits, self.lengths, self.episodic_returns):
            t.zero_()
        return self.observation

    def rollout(self, forced_reset=None, forced_actions=None, forced_masks=None):
        """reinforce.py:53-66 for all envs in one launch.  Teacher forcing (tests): forced_reset (N, 4) f64, forced_actions (N, 500), forced_masks (N, 500, 4)."""
        dev, n = self.device, self.num_envs
        fr = None if forced_reset is None else forced_reset.to(dev, torch.float64).reshape(n, 4).contiguous()
        fa = None if forced_actions is None else forced_actions.to(dev, torch.int32).reshape(n, PG.MAX_STEPS).contiguous()
        fm = None if forced_masks is None else forced_masks.to(dev, torch.int32).reshape(n, PG.MAX_STEPS, 4).contiguous()
        buf = self._buffers(fr, fa, fm)
        PG.check(PG.lib().mi_pg_rollout_episodes(self.env.handle, C.byref(buf), self._s()), "mi_pg_rollout_episodes")

    def compute_returns(self):
        """:67,71-73 — raw and per-episode normalised returns from `lengths`."""
        buf = self._buffers()
        PG.check(PG.lib().mi_pg_returns(C.byref(buf), self.num_envs, self.gamma, self._s()), "mi_pg_returns")

    def grad(self):
        """:74-76 — `grads` (898,) of the summed policy loss at the current parameters."""
        buf = self._buffers()
        PG.check(PG.lib().mi_pg_grad(C.byref(buf), self.num_envs, self._s()), "mi_pg_grad")

    def optimizer_step(self):
        """:77."""
        self.optimizer.step(self.grads)
        self.update_index += 1

    def update(self):
        """One update in one host call; bit-identical to rollout(); compute_returns(); grad(); optimizer_step()."""
        o = self.optimizer
        g = o.param_groups[0]
        buf = self._buffers()
        hp = PG.PGHparams(self.gamma, 0, o.step_count + 1, float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"])
        PG.check(PG.lib().mi_pg_update(self.env.handle, C.byref(buf), C.byref(hp), self._s()), "mi_pg_update")
        o.step_count += 1
        self.update_index += 1

    def policy_loss(self):
        """torch.sum(-b_log_probs * b_returns) (:74) over all envs, from the storage (rows past an episode's end are 0)."""
        return torch.sum(-self.log_probs * self.b_returns)

    def drain_episodes(self):
        """Host sync.  -> (count, [(env, length, return), ...] in env order) of the last rollout: every env finishes exactly one episode per update."""
        lens = self.lengths.cpu().tolist()
        rets = self.episodic_returns.cpu().tolist()
        return len(lens), [(e, int(lens[e]), float(rets[e])) for e in range(len(lens))]
