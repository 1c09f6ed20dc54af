"""Greedy policy evaluation on the device: ``evaluate(policy)`` runs whole CartPole-v1 episodes of a trained value network inside ONE launch of libmirl_eval.so
(include/mi_eval.h) — no epsilon, no noisy heads, the parameters standing still — and returns the per-episode results as device tensors.

    res = deep_rl_amd.evaluate(engine, episodes=100)
    print(res.mean, res.std, res.truncated_fraction)

    python -m deep_rl_amd.evaluate CHECKPOINT.npz [MORE.npz ...] [--episodes N] [--seed S]        (one line per checkpoint)

The engine's (or network's) flat online parameters are read in place: neither copied nor written, and the engine's own env, ring and counters are not touched.
Evaluation episodes are keyed (seed, env_id_base + e, episode 0); the default env_id_base of 2^40 keeps their starts disjoint from any training env's ids.
"""
import math
import sys
import types

import numpy as np
import torch

from . import _native_ev as K
from .agent import C51QNetwork, DuelingQNetwork, NoisyDuelingQNetwork, QRQNetwork, RainbowQNetwork

# engine class name (what checkpoint.py stores as `kind`) -> the network class whose online parameters it trains
ENGINES_EVALUABLE = {
    "DuelingDQNEngine": "DuelingQNetwork", "PDDDQNEngine": "DuelingQNetwork", "NStepDQNEngine": "DuelingQNetwork",
    "NoisyDQNEngine": "NoisyDuelingQNetwork",
    "QRDQNEngine": "QRQNetwork", "C51Engine": "C51QNetwork", "RainbowEngine": "RainbowQNetwork",
}
_NETWORKS = {c.__name__: c for c in (DuelingQNetwork, NoisyDuelingQNetwork, QRQNetwork, C51QNetwork, RainbowQNetwork)}
# most derived first: the first class a network is an instance of decides
_KIND_OF = ((RainbowQNetwork, K.RAINBOW), (NoisyDuelingQNetwork, K.DUELING), (DuelingQNetwork, K.DUELING), (QRQNetwork, K.QR), (C51QNetwork, K.C51))
C51_SUPPORT = (-100.0, 100.0)   # libmirl_c51.so's compile-time support


def _resolve(policy):
    """-> (network, kind, v_min, v_max) of an engine or a network; anything else is a MiError"""
    net = policy if isinstance(policy, torch.nn.Module) else getattr(policy, "q", None)
    for cls, kind in _KIND_OF:
        if isinstance(net, cls):
            break
    else:
        raise K.MiError("evaluate: %s is not supported — the greedy evaluation kernels cover DuelingQNetwork / NoisyDuelingQNetwork (DuelingDQNEngine, PDDDQNEngine, "
                        "NStepDQNEngine, NoisyDQNEngine), QRQNetwork (QRDQNEngine), C51QNetwork (C51Engine) and RainbowQNetwork (RainbowEngine).  The plain QNetwork "
                        "(DQNEngine, PERDQNEngine, DoubleDQNEngine) has no kind: libmirl's and libmirl_ddqn's forward calls give it different bits (include/mi_eval.h). "
                        "IQN, PPO, REINFORCE and SAC are out of scope and there is no torch fallback" % type(policy).__name__)
    v_min, v_max = 0.0, 1.0   # not read by the scalar kinds
    if kind == K.C51:
        v_min, v_max = C51_SUPPORT
    elif kind == K.RAINBOW:   # the engine's support is what it trains under; a bare network carries its own
        src = policy if hasattr(policy, "v_min") else net
        v_min, v_max = float(src.v_min), float(src.v_max)
    flat = net.flat
    if flat.dtype != torch.float32 or not flat.is_cuda or not flat.is_contiguous() or flat.numel() < K.NPARAMS[kind]:
        raise K.MiError("evaluate: the %s parameters must be one contiguous float32 device vector of at least %d elements" % (K.KIND_NAMES[kind], K.NPARAMS[kind]))
    return net, kind, v_min, v_max


class EvalResult:
    """The device tensors ``returns`` f32 [E], ``lengths`` i32 [E], ``truncated`` u8 [E], ``min_gap`` f32 [E] (the smallest |q_1 - q_0| of each episode) and, with
    ``trace``, ``actions`` u8 [E][500] (row e valid for t < lengths[e]); ``source_id`` of the library that produced them.  ``mean``, ``std`` (population), ``min``,
    ``max`` of the returns and ``truncated_fraction`` are computed in float64 with torch on first access (which waits for the launch)."""

    def __init__(self, returns, lengths, truncated, min_gap, actions, kind, source_id):
        self.returns, self.lengths, self.truncated, self.min_gap, self.actions = returns, lengths, truncated, min_gap, actions
        self.kind, self.source_id = kind, source_id
        self._stats = None

    def _get(self, i):
        if self._stats is None:
            # a return is a whole number <= 500, so the sums of r and of r * r are exact in float64 in whatever order torch adds them: the mean is one rounding and
            # the (population) standard deviation sqrt((n * sum r^2 - (sum r)^2) / n^2) two, with no cancellation against a rounded mean
            r, n = self.returns.to(torch.float64), float(self.returns.numel())
            s1, s2 = r.sum().item(), (r * r).sum().item()
            self._stats = (s1 / n, math.sqrt((n * s2 - s1 * s1) / (n * n)), r.min().item(), r.max().item(), self.truncated.to(torch.float64).sum().item() / n)
        return self._stats[i]

    mean = property(lambda self: self._get(0))
    std = property(lambda self: self._get(1))
    min = property(lambda self: self._get(2))
    max = property(lambda self: self._get(3))
    truncated_fraction = property(lambda self: self._get(4))

    @property
    def episodes(self):
        return int(self.returns.numel())

    def line(self):
        """the CLI's line"""
        return "episodes=%d mean_return=%.6f std=%.6f min=%.1f max=%.1f truncated=%.6f" % (self.episodes, self.mean, self.std, self.min, self.max, self.truncated_fraction)


def evaluate(policy, episodes=100, seed=1, env_id_base=1 << 40, *, forced_actions=None, forced_starts=None, trace=False, max_workgroups=0, stream=None):
    """Run `episodes` greedy CartPole-v1 episodes of `policy` (an engine or a network) in one launch.  -> EvalResult.

    forced_actions u8 [E][500] / forced_starts f64 [E][4] (device tensors) teacher-force the actions / replace the keyed starts; `trace` records the actions taken;
    `max_workgroups` caps the launch (0: the library's default; the results do not depend on it); `stream` is a torch.cuda.Stream (None: the current one)."""
    net, kind, v_min, v_max = _resolve(policy)
    E, dev = int(episodes), net.flat.device
    if E < 1:
        raise K.MiError("evaluate: episodes must be >= 1")
    for name, t, dt, shape in (("forced_actions", forced_actions, torch.uint8, (E, K.MAX_STEPS)), ("forced_starts", forced_starts, torch.float64, (E, 4))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous()):
            raise K.MiError("evaluate: %s must be a contiguous %s tensor of shape %s on %s" % (name, dt, shape, dev))
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(s):   # the outputs are allocated on the stream that fills them
            returns = torch.empty(E, dtype=torch.float32, device=dev)
            lengths = torch.empty(E, dtype=torch.int32, device=dev)
            truncated = torch.empty(E, dtype=torch.uint8, device=dev)
            min_gap = torch.empty(E, dtype=torch.float32, device=dev)
            actions = torch.zeros((E, K.MAX_STEPS), dtype=torch.uint8, device=dev) if trace else None
            a = K.EVArgs(K.ptr(net.flat), K.ptr(returns), K.ptr(lengths), K.ptr(truncated), K.ptr(min_gap), K.ptr(actions), K.ptr(forced_actions), K.ptr(forced_starts),
                         int(seed) & (2 ** 64 - 1), int(env_id_base) & (2 ** 64 - 1), kind, E, int(max_workgroups), v_min, v_max, 0)
            K.check(K.lib().mi_ev_episodes(a, s.cuda_stream), "mi_ev_episodes")
    return EvalResult(returns, lengths, truncated, min_gap, actions, kind, K.source_id())


def forward(policy, observation, support=None):
    """q [n][2] of observation [n][4] through the device functions the episode loop uses (mi_ev_forward); `support` overrides (v_min, v_max) of a categorical kind"""
    net, kind, v_min, v_max = _resolve(policy)
    if support is not None:
        v_min, v_max = float(support[0]), float(support[1])
    obs = observation.to(net.flat.device, torch.float32).reshape(-1, 4).contiguous()
    q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=obs.device)
    K.check(K.lib().mi_ev_forward(K.ptr(net.flat), kind, v_min, v_max, K.ptr(obs), obs.shape[0], K.ptr(q), K.stream_ptr(obs.device)), "mi_ev_forward")
    return q


class _CartPoleSpec:
    """what the network constructors read of an env"""
    observation_space = types.SimpleNamespace(shape=(4,))
    action_space = types.SimpleNamespace(n=2)

    def __init__(self, device):
        self.device = device


def load_policy(path, device="cuda", v_min=None, v_max=None):
    """the online network of a checkpoint written by deep_rl_amd.checkpoint.save: `kind` names the engine class, `params` are its online parameters; nothing else is
    read.  A Rainbow checkpoint does not hold its support (it is the engine's constructor argument): RainbowEngine's default unless v_min / v_max are given."""
    from .checkpoint import _npz_path

    with np.load(_npz_path(path), allow_pickle=False) as z:
        if "kind" not in z.files or "params" not in z.files:
            raise K.MiError("evaluate: %s is not an engine checkpoint (no `kind` / `params`)" % path)
        kind, params = str(z["kind"]), z["params"]
    if kind not in ENGINES_EVALUABLE:
        raise K.MiError("evaluate: a checkpoint of %s cannot be evaluated; supported: %s" % (kind, ", ".join(sorted(ENGINES_EVALUABLE))))
    cls, spec = _NETWORKS[ENGINES_EVALUABLE[kind]], _CartPoleSpec(torch.device(device))
    if cls is RainbowQNetwork:
        net = cls(spec, v_min=0.0 if v_min is None else v_min, v_max=100.0 if v_max is None else v_max)
    else:
        net = cls(spec)
    if params.shape != tuple(net.flat.shape):
        raise K.MiError("evaluate: the checkpoint's params have shape %s, a %s has %s" % (params.shape, cls.__name__, tuple(net.flat.shape)))
    net.flat.copy_(torch.from_numpy(params))   # (not load_flat: the dueling network's plain image is not needed here)
    return net


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m deep_rl_amd.evaluate", description="greedy return of a checkpoint's online network on CartPole-v1")
    ap.add_argument("checkpoint", nargs="+", help="checkpoints written by deep_rl_amd.checkpoint.save; one line is printed per checkpoint")
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--v-min", type=float, default=None, help="Rainbow's support (default 0)")
    ap.add_argument("--v-max", type=float, default=None, help="Rainbow's support (default 100)")
    args = ap.parse_args(argv)
    for path in args.checkpoint:
        print(evaluate(load_policy(path, v_min=args.v_min, v_max=args.v_max), episodes=args.episodes, seed=args.seed).line(), flush=True)
    return 0


class _CallableModule(types.ModuleType):
    """``deep_rl_amd.evaluate`` names this module AND is the function: ``deep_rl_amd.evaluate(engine)`` calls ``evaluate.evaluate(engine)``"""

    def __call__(self, *a, **kw):
        return evaluate(*a, **kw)


sys.modules[__name__].__class__ = _CallableModule

if __name__ == "__main__":
    sys.exit(main())
