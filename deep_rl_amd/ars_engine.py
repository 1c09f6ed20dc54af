"""ARSEngine — Augmented Random Search (Mania, Guy, Recht 2018; V2-t with discrete actions, V1 with ``normalize=False``) on CartPole-v1 through libmirl_ars.so
(include/mi_ars.h).

Everything lives on the device: the linear policy M (8 floats), the observation statistics, the normaliser and the iteration counter.  ``train(n)`` enqueues the
2 n launches of n iterations with nothing read back between them; ``evaluate`` runs greedy episodes of M in one launch and touches nothing of the state.  There is
no env object, no ring and no optimizer: an episode is keyed (seed, env_id_base + e, iteration) and runs from its reset to its end inside one launch.
"""
import math
import types

import torch

from . import _native_ars as K
from .agent import LinearPolicy

_U64 = 2 ** 64 - 1


class _CartPoleSpec:
    """what LinearPolicy reads of an env"""
    observation_space = types.SimpleNamespace(shape=(4,))
    action_space = types.SimpleNamespace(n=2)

    def __init__(self, device):
        self.device = device


class ARSEngine:
    def __init__(self, n_directions=8, n_top=None, step_size=0.02, noise=0.03, normalize=True, seed=1, env_id_base=0, device="cuda", max_workgroups=0):
        n_top = n_directions if n_top is None else n_top
        # the library's own checks, restated so that a wrong constructor fails before anything is allocated or loaded
        if not (1 <= int(n_directions) <= K.MAX_DIRECTIONS):
            raise K.MiError("ARSEngine: n_directions must be 1 .. %d" % K.MAX_DIRECTIONS)
        if not (1 <= int(n_top) <= int(n_directions)):
            raise K.MiError("ARSEngine: n_top must be 1 .. n_directions")
        if not (math.isfinite(noise) and noise >= 0) or not math.isfinite(step_size):
            raise K.MiError("ARSEngine: noise must be finite and >= 0, step_size finite")
        self.n_directions, self.n_top, self.step_size, self.noise, self.normalize = int(n_directions), int(n_top), float(step_size), float(noise), bool(normalize)
        self.seed, self.env_id_base, self.max_workgroups = int(seed), int(env_id_base), int(max_workgroups)
        self.device = dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            self.device = dev = torch.device("cuda", torch.cuda.current_device())
        self.policy = LinearPolicy(_CartPoleSpec(dev), device=dev)
        self.stats = torch.zeros(K.NSTATS, dtype=torch.float64, device=dev)
        self.norm = torch.cat([torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)]).to(dev)
        self.iteration = torch.zeros(1, dtype=torch.int64, device=dev)
        E = 2 * self.n_directions
        self.deltas = torch.zeros((self.n_directions, K.NPARAMS), dtype=torch.float32, device=dev)
        self.partials = torch.zeros((E, K.NSTATS), dtype=torch.float64, device=dev)
        self.truncated = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.returns = self.lengths = None   # [iterations][2 N] of the last train()
        self.global_step = 0                 # env steps reported by drain_episodes so far

    # -- plumbing --------------------------------------------------------------------------------------------------------------------------------------
    def args(self, returns, lengths, truncated=None, actions=None, n_episodes=0, noise=None, seed=None, env_id_base=None, max_workgroups=None):
        """the mi_ars_args_t of this engine's state with the given outputs"""
        return K.ARSArgs(K.ptr(self.policy.flat), K.ptr(self.stats), K.ptr(self.norm), K.ptr(self.iteration), K.ptr(self.deltas), K.ptr(returns), K.ptr(lengths),
                         K.ptr(truncated), K.ptr(actions), K.ptr(self.partials), (self.seed if seed is None else int(seed)) & _U64,
                         (self.env_id_base if env_id_base is None else int(env_id_base)) & _U64, self.n_directions, self.n_top, int(n_episodes),
                         self.max_workgroups if max_workgroups is None else int(max_workgroups), int(self.normalize), self.step_size,
                         self.noise if noise is None else float(noise), 0)

    # -- training --------------------------------------------------------------------------------------------------------------------------------------
    def train(self, iterations=1):
        """`iterations` iterations, enqueued at once.  -> returns f32 [iterations][2 N] (device; row t, element 2 i + s: direction i with sign +/-)"""
        n = int(iterations)
        if n < 1:
            raise K.MiError("ARSEngine.train: iterations must be >= 1")
        E = 2 * self.n_directions
        with torch.cuda.device(self.device):
            self.returns = torch.empty((n, E), dtype=torch.float32, device=self.device)
            self.lengths = torch.empty((n, E), dtype=torch.int32, device=self.device)
            a = self.args(self.returns, self.lengths, self.truncated)
            K.check(K.lib().mi_ars_iterate(a, n, K.stream_ptr(self.device)), "mi_ars_iterate")
        return self.returns

    def drain_episodes(self):
        """Host sync.  -> (count, [(episode, length, return), ...]) of the last train(), iteration by iteration in episode order"""
        if self.lengths is None:
            return 0, []
        lens, rets = self.lengths.cpu().reshape(-1).tolist(), self.returns.cpu().reshape(-1).tolist()
        E = 2 * self.n_directions
        return len(lens), [(j % E, int(lens[j]), float(rets[j])) for j in range(len(lens))]

    # -- evaluation ------------------------------------------------------------------------------------------------------------------------------------
    def evaluate(self, episodes=100, seed=1, env_id_base=1 << 40, trace=False):
        """`episodes` greedy episodes of M under the current normaliser in one launch; nothing of the state changes.  -> EvalResult (min_gap is None)"""
        from .evaluate import EvalResult

        E = int(episodes)
        if E < 1:
            raise K.MiError("ARSEngine.evaluate: episodes must be >= 1")
        with torch.cuda.device(self.device):
            returns = torch.empty(E, dtype=torch.float32, device=self.device)
            lengths = torch.empty(E, dtype=torch.int32, device=self.device)
            truncated = torch.empty(E, dtype=torch.uint8, device=self.device)
            actions = torch.zeros((E, K.MAX_STEPS), dtype=torch.uint8, device=self.device) if trace else None
            a = self.args(returns, lengths, truncated, actions, n_episodes=E, noise=0.0, seed=seed, env_id_base=env_id_base)
            K.check(K.lib().mi_ars_episodes(a, K.stream_ptr(self.device)), "mi_ars_episodes")
        return EvalResult(returns, lengths, truncated, None, actions, "ARS", K.source_id())
