"""ctypes binding of libmirl_c51.so — the C ABI declared in include/mi_c51.h (C51 categorical DQN on CartPole-v1).

A third library beside libmirl.so and libmirl_pg.so.  It is loaded LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so
present, and the first use of the C51 network or engine without a built ``deep_rl_amd/libmirl_c51.so`` raises ``MiError`` — there is no fallback.  Build all
three with ``make -C deep_rl_amd/csrc``.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_C51_SO", os.path.join(_HERE, "libmirl_c51.so"))  # MIRL_C51_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_C51_VERSION of the include/mi_c51.h these signatures and struct layouts were written against
NPARAMS = 27934
N_ATOMS = 101
V_MIN, V_MAX = -100.0, 100.0
H1, H2 = 120, 84
OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_W3, OFF_B3 = 0, 480, 600, 10680, 10764, 27732
MAX_SLABS = 128
SLAB_STRIDE = 27936
MAX_STEPS_PER_CALL = 64
MI_C51_OK = 0


class C51Ring(C.Structure):   # mi_c51_ring_t
    _fields_ = [("observations", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("terminated", C.c_void_p), ("slots", C.c_int64),
                ("n_envs", C.c_int32), ("reserved", C.c_int32)]


class C51Batch(C.Structure):   # mi_c51_batch_t
    _fields_ = [(n, C.c_void_p) for n in ("params", "target_params", "idx", "target_probs", "next_actions", "probs", "grads", "loss", "workspace")] + [
        ("sample_seed", C.c_uint64), ("sample_update", C.c_uint64), ("sample_upper", C.c_int64), ("batch", C.c_int32), ("gamma", C.c_float), ("mid_event", C.c_void_p)]


class C51Adam(C.Structure):   # mi_c51_adam_t
    _fields_ = [("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_int64), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double)]


_VP, _I, _F, _D, _I64, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_int64, C.c_size_t
SIGNATURES = {
    "mi_c51_version": (_I, []),
    "mi_c51_last_error": (C.c_char_p, []),
    "mi_c51_source_id": (C.c_char_p, []),
    "mi_c51_workspace_bytes": (_SZ, [_I]),
    "mi_c51_forward": (_I, [_VP, _VP, _I, _VP, _VP, _VP]),
    "mi_c51_act_steps": (_I, [_VP, _VP, _I, _I64, C.POINTER(C51Ring), _D, _D, _D, _I64, _VP, _VP, _VP, _VP, _VP, _I, _VP]),
    "mi_c51_target": (_I, [_VP, C.POINTER(C51Ring), _VP, _I, _F, _VP, _VP, _VP]),
    "mi_c51_grad": (_I, [C.POINTER(C51Ring), C.POINTER(C51Batch), _VP]),
    "mi_c51_update": (_I, [C.POINTER(C51Ring), C.POINTER(C51Batch), C.POINTER(C51Adam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_c51", "C51")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = C51Ring, C51Batch, C51Adam


def workspace_bytes(batch):
    return lib().mi_c51_workspace_bytes(batch)


def grad(ring, batch, stream):
    check(lib().mi_c51_grad(C.byref(ring), C.byref(batch), stream), "mi_c51_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_c51_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_c51_update")
