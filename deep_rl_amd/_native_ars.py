"""ctypes binding of libmirl_ars.so — the C ABI declared in include/mi_ars.h (Augmented Random Search on CartPole-v1).

A thirteenth library beside libmirl.so and the eleven others.  It is loaded LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so
present, and the first ``ARSEngine`` without a built ``deep_rl_amd/libmirl_ars.so`` raises ``MiError`` — there is no fallback.  Build all thirteen with
``make -C deep_rl_amd/csrc``.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for ars_engine.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_ARS_SO", os.path.join(_HERE, "libmirl_ars.so"))  # MIRL_ARS_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_ARS_VERSION of the include/mi_ars.h these signatures and the struct layout were written against
MAX_STEPS = 500
MAX_DIRECTIONS = 4096
DEFAULT_WORKGROUPS = 1024
NPARAMS, NSTATS, STREAM = 8, 9, 15
MI_ARS_OK = 0


class ARSArgs(C.Structure):   # mi_ars_args_t
    _fields_ = [(n, C.c_void_p) for n in ("policy", "stats", "norm", "iteration", "deltas", "returns", "lengths", "truncated", "actions", "partials")] + [
        ("seed", C.c_uint64), ("env_id_base", C.c_uint64), ("n_directions", C.c_int32), ("n_top", C.c_int32), ("n_episodes", C.c_int32),
        ("max_workgroups", C.c_int32), ("normalize", C.c_int32), ("step_size", C.c_float), ("noise", C.c_float), ("reserved", C.c_int32)]


_VP, _I = C.c_void_p, C.c_int
SIGNATURES = {
    "mi_ars_version": (_I, []),
    "mi_ars_last_error": (C.c_char_p, []),
    "mi_ars_source_id": (C.c_char_p, []),
    "mi_ars_episodes": (_I, [C.POINTER(ARSArgs), _VP]),
    "mi_ars_update": (_I, [C.POINTER(ARSArgs), _VP]),
    "mi_ars_iterate": (_I, [C.POINTER(ARSArgs), _I, _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_ars", "Augmented Random Search")
