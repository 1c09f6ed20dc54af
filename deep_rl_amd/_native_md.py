"""ctypes binding of libmirl_mdqn.so — the C ABI declared in include/mi_mdqn.h (Munchausen DQN on CartPole-v1).

A twelfth library.  It is loaded LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so present, and the first use of the engine
without a built ``deep_rl_amd/libmirl_mdqn.so`` raises ``MiError`` — there is no fallback.  Build all twelve with ``make -C deep_rl_amd/csrc``.

The library has no acting and no forward entry point: the engine acts and evaluates through libmirl_ddqn.so.  Its ring and Adam structs are layout-identical to that
library's (the header says so, tests/test_mdqn_abi_cpu.py checks it), so ``Ring`` and ``AdamArgs`` ARE _native_ddqn's classes: one ring struct serves both.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)
from ._native_ddqn import DDQNAdam, DDQNBatch, DDQNRing

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_MDQN_SO", os.path.join(_HERE, "libmirl_mdqn.so"))  # MIRL_MDQN_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_MD_VERSION of the include/mi_mdqn.h these signatures and struct layouts were written against
NPARAMS = 10934
H1, H2 = 120, 84
OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_W3, OFF_B3 = 0, 480, 600, 10680, 10764, 10932
MAX_SLABS = 128
SLAB_STRIDE = 10936
MI_MD_OK = 0


class MDBatch(C.Structure):   # mi_md_batch_t: mi_ddqn_batch_t with bonus, soft_value, alpha, tau and clip_lo behind it
    _fields_ = list(DDQNBatch._fields_) + [("bonus", C.c_void_p), ("soft_value", C.c_void_p), ("alpha", C.c_float), ("tau", C.c_float), ("clip_lo", C.c_float)]


MDRing, MDAdam = DDQNRing, DDQNAdam   # mi_md_ring_t, mi_md_adam_t

_VP, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SIGNATURES = {
    "mi_md_version": (_I, []),
    "mi_md_last_error": (C.c_char_p, []),
    "mi_md_source_id": (C.c_char_p, []),
    "mi_md_workspace_bytes": (_SZ, [_I]),
    "mi_md_target": (_I, [C.POINTER(MDRing), C.POINTER(MDBatch), _VP]),
    "mi_md_grad": (_I, [C.POINTER(MDRing), C.POINTER(MDBatch), _VP]),
    "mi_md_update": (_I, [C.POINTER(MDRing), C.POINTER(MDBatch), C.POINTER(MDAdam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_md", "Munchausen DQN")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = MDRing, MDBatch, MDAdam


def workspace_bytes(batch):
    return lib().mi_md_workspace_bytes(batch)


def target(ring, batch, stream):
    check(lib().mi_md_target(C.byref(ring), C.byref(batch), stream), "mi_md_target")


def grad(ring, batch, stream):
    check(lib().mi_md_grad(C.byref(ring), C.byref(batch), stream), "mi_md_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_md_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_md_update")
