"""ctypes binding of libmirl_iqn.so — the C ABI declared in include/mi_iqn.h (IQN on CartPole-v1).

A fourth library beside libmirl.so, libmirl_pg.so and libmirl_c51.so.  It is loaded LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only
libmirl.so present, and the first use of the IQN networks or engine without a built ``deep_rl_amd/libmirl_iqn.so`` raises ``MiError`` — there is no fallback.
Build all four with ``make -C deep_rl_amd/csrc``.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_IQN_SO", os.path.join(_HERE, "libmirl_iqn.so"))  # MIRL_IQN_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_IQN_VERSION of the include/mi_iqn.h these signatures and struct layouts were written against
NPARAMS = 44898
EMB, NCOS, HID = 64, 64, 512
N_TAU, N_TAU_PRIME, N_QUANT = 64, 64, 32
OFFSETS = dict(FW1=0, FB1=128, FW2=160, FB2=2208, FW3=2272, FB3=6368, CW=6432, CB=10528, QW1=10592, QB1=43360, QW2=43872, QB2=44896)
SIZES = dict(FW1=128, FB1=32, FW2=2048, FB2=64, FW3=4096, FB3=64, CW=4096, CB=64, QW1=32768, QB1=512, QW2=1024, QB2=2)
F_NPARAMS, C_NPARAMS, Q_NPARAMS = 6432, 4160, 34306   # FeaturesExtractor, CosineEmbeddingNetwork, QuantileNetwork
MAX_SLABS = 64
SLAB_STRIDE = 44900
MAX_STEPS_PER_CALL = 64
MI_IQN_OK = 0
MI_IQN_EINVAL = -1


class IQNRing(C.Structure):   # mi_iqn_ring_t
    _fields_ = [("observations", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("terminated", C.c_void_p), ("slots", C.c_int64),
                ("n_envs", C.c_int32), ("reserved", C.c_int32)]


class IQNAct(C.Structure):   # mi_iqn_act_t
    _fields_ = [(n, C.c_void_p) for n in ("params", "obs_cur", "forced_actions", "forced_resets", "forced_taus", "taus_out", "episodes", "episode_stats")] + [
        ("global_step", C.c_int64), ("learning_starts", C.c_int64), ("slope", C.c_double), ("final_epsilon", C.c_double), ("n_steps", C.c_int32), ("max_ep", C.c_int32)]


class IQNBatch(C.Structure):   # mi_iqn_batch_t
    _fields_ = [(n, C.c_void_p) for n in ("params", "target_params", "idx", "forced_taus", "forced_next_taus", "forced_tau_dashes", "taus", "current", "target",
                                           "next_actions", "grads", "loss", "workspace")] + [
        ("seed", C.c_uint64), ("update", C.c_uint64), ("sample_upper", C.c_int64), ("batch", C.c_int32), ("gamma", C.c_float), ("mid_event", C.c_void_p)]


class IQNAdam(C.Structure):   # mi_iqn_adam_t
    _fields_ = [("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_int64), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double)]


_VP, _I, _F, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
SIGNATURES = {
    "mi_iqn_version": (_I, []),
    "mi_iqn_last_error": (C.c_char_p, []),
    "mi_iqn_source_id": (C.c_char_p, []),
    "mi_iqn_workspace_bytes": (_SZ, [_I]),
    "mi_iqn_forward": (_I, [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "mi_iqn_act_steps": (_I, [_VP, C.POINTER(IQNRing), C.POINTER(IQNAct), _VP]),
    "mi_iqn_target": (_I, [C.POINTER(IQNRing), C.POINTER(IQNBatch), _VP]),
    "mi_iqn_quantile_huber": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "mi_iqn_grad": (_I, [C.POINTER(IQNRing), C.POINTER(IQNBatch), _VP]),
    "mi_iqn_update": (_I, [C.POINTER(IQNRing), C.POINTER(IQNBatch), C.POINTER(IQNAdam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_iqn", "IQN")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = IQNRing, IQNBatch, IQNAdam


def workspace_bytes(batch):
    return lib().mi_iqn_workspace_bytes(batch)


def grad(ring, batch, stream):
    check(lib().mi_iqn_grad(C.byref(ring), C.byref(batch), stream), "mi_iqn_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_iqn_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_iqn_update")
