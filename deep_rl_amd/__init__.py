"""deep_rl_amd — MI355X-native vectorised-rollout + policy-update engine behind the call surface of
qgallouedec/deep_rl's single-file scripts (ppo.py first).

Host code is Python on PyTorch-ROCm for module / optimizer bookkeeping only; the hot path (batched
CartPole stepper, rollout storage, GAE scan, tiny-MLP forward/backward, clip + Adam) is hand-written HIP
for gfx950 in ``csrc/`` behind the C ABI of ``include/mi_rl.h``.  There is no CPU fallback: importing
``deep_rl_amd._native`` without the built ``libmirl.so`` raises.
"""
from . import _native  # noqa: F401
from ._native import set_contraction, get_contraction  # noqa: F401
from .envs import make, CartPoleVecEnv, PendulumVecEnv  # noqa: F401
from .agent import ActorCritic, QNetwork, DuelingQNetwork, SoftQNetwork, Actor, DropoutPolicy, C51QNetwork, QRQNetwork, layer_init, pack  # noqa: F401
from .agent import FeaturesExtractor, CosineEmbeddingNetwork, QuantileNetwork, iqn_forward  # noqa: F401
from .agent import NoisyLinear, NoisyDuelingQNetwork, RainbowQNetwork, LinearPolicy  # noqa: F401
from .optim import ClipAdam, Adam  # noqa: F401
from .engine import PPOEngine  # noqa: F401
from .dqn_engine import DQNEngine, DuelingDQNEngine, PERDQNEngine  # noqa: F401
from .sac_engine import SACEngine  # noqa: F401
from .reinforce_engine import ReinforceEngine  # noqa: F401  (libmirl_pg.so itself loads on first use)
from .c51_engine import C51Engine  # noqa: F401  (libmirl_c51.so itself loads on first use)
from .iqn_engine import IQNEngine  # noqa: F401  (libmirl_iqn.so itself loads on first use)
from .qrdqn_engine import QRDQNEngine  # noqa: F401  (libmirl_qr.so itself loads on first use)
from .ddqn_engine import DoubleDQNEngine  # noqa: F401  (libmirl_ddqn.so itself loads on first use)
from .mdqn_engine import MunchausenDQNEngine  # noqa: F401  (libmirl_mdqn.so itself loads on first use)
from .pdd_engine import PDDDQNEngine  # noqa: F401  (libmirl_pdd.so itself loads on first use)
from .nstep_engine import NStepDQNEngine  # noqa: F401  (libmirl_nstep.so itself loads on first use)
from .noisy_engine import NoisyDQNEngine  # noqa: F401  (libmirl_noisy.so itself loads on first use)
from .rainbow_engine import RainbowEngine  # noqa: F401  (libmirl_rainbow.so itself loads on first use)
from .ars_engine import ARSEngine  # noqa: F401  (libmirl_ars.so itself loads on first use)


def __getattr__(name):
    """``deep_rl_amd.evaluate`` (greedy policy evaluation, libmirl_eval.so) is imported on first use; the module is callable: ``deep_rl_amd.evaluate(engine)``"""
    if name in ("evaluate", "EvalResult"):
        import importlib

        mod = importlib.import_module(".evaluate", __name__)
        return mod if name == "evaluate" else mod.EvalResult
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


__all__ = ["make", "CartPoleVecEnv", "ActorCritic", "QNetwork", "layer_init", "ClipAdam", "PPOEngine", "DQNEngine",
           "DuelingQNetwork", "DuelingDQNEngine", "PERDQNEngine", "PendulumVecEnv", "SoftQNetwork", "Actor", "Adam", "SACEngine", "DropoutPolicy", "ReinforceEngine", "C51QNetwork", "C51Engine", "FeaturesExtractor", "CosineEmbeddingNetwork", "QuantileNetwork", "iqn_forward", "IQNEngine", "QRQNetwork", "QRDQNEngine", "DoubleDQNEngine", "MunchausenDQNEngine", "PDDDQNEngine", "NStepDQNEngine", "NoisyLinear", "NoisyDuelingQNetwork", "NoisyDQNEngine", "RainbowQNetwork", "RainbowEngine", "LinearPolicy", "ARSEngine", "pack", "set_contraction", "get_contraction", "evaluate", "EvalResult"]
