"""ctypes binding of libmirl_pdd.so — the C ABI declared in include/mi_pdd.h (prioritized dueling Double DQN on CartPole-v1).

A seventh library beside libmirl.so, libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so and libmirl_ddqn.so.  It is loaded LAZILY, on the first ``lib()``
call: importing ``deep_rl_amd`` works with only libmirl.so present, and the first use of the engine without a built ``deep_rl_amd/libmirl_pdd.so`` raises
``MiError`` — there is no fallback.  Build all seven with ``make -C deep_rl_amd/csrc``.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_PDD_SO", os.path.join(_HERE, "libmirl_pdd.so"))  # MIRL_PDD_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_PDD_VERSION of the include/mi_pdd.h these signatures and struct layouts were written against
NPARAMS = 11019
H1, H2 = 120, 84
OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_WV, OFF_BV, OFF_WA, OFF_BA = 0, 480, 600, 10680, 10764, 10848, 10849, 11017
MAX_SLABS = 128
SLAB_STRIDE = 11020
MAX_STEPS_PER_CALL = 64
MI_PDD_OK = 0


class PDDRing(C.Structure):   # mi_pdd_ring_t
    _fields_ = [("observations", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("terminated", C.c_void_p), ("slots", C.c_int64),
                ("n_envs", C.c_int32), ("reserved", C.c_int32)]


class PDDAct(C.Structure):   # mi_pdd_act_t
    _fields_ = [(n, C.c_void_p) for n in ("params", "obs_cur", "forced_actions", "forced_resets", "episodes", "episode_stats")] + [
        ("global_step", C.c_int64), ("total_timesteps", C.c_int64), ("learning_starts", C.c_int64), ("start_e", C.c_double), ("end_e", C.c_double),
        ("exploration_fraction", C.c_double), ("n_steps", C.c_int32), ("max_ep", C.c_int32)]


class PDDBatch(C.Structure):   # mi_pdd_batch_t: mi_ddqn_batch_t with weights and td_abs behind it
    _fields_ = [(n, C.c_void_p) for n in ("params", "target_params", "idx", "current", "target", "next_actions", "grads", "loss", "workspace")] + [
        ("sample_seed", C.c_uint64), ("sample_update", C.c_uint64), ("sample_upper", C.c_int64), ("batch", C.c_int32), ("gamma", C.c_float), ("mid_event", C.c_void_p),
        ("weights", C.c_void_p), ("td_abs", C.c_void_p)]


class PDDAdam(C.Structure):   # mi_pdd_adam_t
    _fields_ = [("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_int64), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double)]


_VP, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SIGNATURES = {
    "mi_pdd_version": (_I, []),
    "mi_pdd_last_error": (C.c_char_p, []),
    "mi_pdd_source_id": (C.c_char_p, []),
    "mi_pdd_workspace_bytes": (_SZ, [_I]),
    "mi_pdd_forward": (_I, [_VP, _VP, _I, _VP, _VP]),
    "mi_pdd_act_steps": (_I, [_VP, C.POINTER(PDDRing), C.POINTER(PDDAct), _VP]),
    "mi_pdd_target": (_I, [C.POINTER(PDDRing), C.POINTER(PDDBatch), _VP]),
    "mi_pdd_grad": (_I, [C.POINTER(PDDRing), C.POINTER(PDDBatch), _VP]),
    "mi_pdd_update": (_I, [C.POINTER(PDDRing), C.POINTER(PDDBatch), C.POINTER(PDDAdam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_pdd", "prioritized dueling Double DQN")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = PDDRing, PDDBatch, PDDAdam


def workspace_bytes(batch):
    return lib().mi_pdd_workspace_bytes(batch)


def grad(ring, batch, stream):
    check(lib().mi_pdd_grad(C.byref(ring), C.byref(batch), stream), "mi_pdd_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_pdd_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_pdd_update")
