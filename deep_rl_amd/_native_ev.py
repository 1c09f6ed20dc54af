"""ctypes binding of libmirl_eval.so — the C ABI declared in include/mi_eval.h (greedy policy evaluation on CartPole-v1).

An eleventh library beside libmirl.so and the nine others.  It is loaded LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so
present, and the first ``evaluate()`` without a built ``deep_rl_amd/libmirl_eval.so`` raises ``MiError`` — there is no fallback.  Build all eleven with
``make -C deep_rl_amd/csrc``.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for evaluate.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_EVAL_SO", os.path.join(_HERE, "libmirl_eval.so"))  # MIRL_EVAL_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_EV_VERSION of the include/mi_eval.h these signatures and the struct layout were written against
MAX_STEPS = 500
DEFAULT_WORKGROUPS = 1024
DUELING, QR, C51, RAINBOW = 1, 2, 3, 4   # 0 is free: the plain QNetwork has no kind (include/mi_eval.h "Head kinds")
KIND_NAMES = {DUELING: "DUELING", QR: "QR", C51: "C51", RAINBOW: "RAINBOW"}
NPARAMS = {DUELING: 11019, QR: 21644, C51: 27934, RAINBOW: 23769}   # the floats a kind READS (the vector handed in may be longer)
C51_ATOMS, RAINBOW_ATOMS, QR_QUANT = 101, 51, 64
MI_EV_OK = 0


class EVArgs(C.Structure):   # mi_ev_args_t
    _fields_ = [(n, C.c_void_p) for n in ("params", "returns", "lengths", "truncated", "min_gap", "actions", "forced_actions", "forced_starts")] + [
        ("seed", C.c_uint64), ("env_id_base", C.c_uint64), ("kind", C.c_int32), ("n_episodes", C.c_int32), ("max_workgroups", C.c_int32),
        ("v_min", C.c_float), ("v_max", C.c_float), ("reserved", C.c_int32)]


_VP, _I, _F = C.c_void_p, C.c_int, C.c_float
SIGNATURES = {
    "mi_ev_version": (_I, []),
    "mi_ev_last_error": (C.c_char_p, []),
    "mi_ev_source_id": (C.c_char_p, []),
    "mi_ev_forward": (_I, [_VP, _I, _F, _F, _VP, _I, _VP, _VP]),
    "mi_ev_episodes": (_I, [C.POINTER(EVArgs), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_ev", "policy evaluation")
