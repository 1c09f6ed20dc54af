"""ctypes binding of libmirl_nstep.so — the C ABI declared in include/mi_nstep.h (n-step returns under prioritized dueling Double DQN on CartPole-v1).

An eighth library beside libmirl.so, libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so and libmirl_pdd.so.  It is loaded LAZILY, on the
first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so present, and the first use of the engine without a built
``deep_rl_amd/libmirl_nstep.so`` raises ``MiError`` — there is no fallback.  Build all eight with ``make -C deep_rl_amd/csrc``.

The library has no acting and no forward entry point: the engine acts and evaluates through libmirl_pdd.so.  Its ring and Adam structs are layout-identical to that
library's (the header says so, tests/test_nstep_abi_cpu.py checks it), so ``Ring`` and ``AdamArgs`` ARE _native_pdd's classes: one ring struct serves both.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)
from ._native_pdd import PDDAdam, PDDBatch, PDDRing

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_NS_SO", os.path.join(_HERE, "libmirl_nstep.so"))  # MIRL_NS_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_NS_VERSION of the include/mi_nstep.h these signatures and struct layouts were written against
NPARAMS = 11019
H1, H2 = 120, 84
OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_WV, OFF_BV, OFF_WA, OFF_BA = 0, 480, 600, 10680, 10764, 10848, 10849, 11017
MAX_SLABS = 128
SLAB_STRIDE = 11020
MAX_N = 16
MI_NS_OK = 0


class NSBatch(C.Structure):   # mi_ns_batch_t: mi_pdd_batch_t with horizon, n_step and head_slot behind it
    _fields_ = list(PDDBatch._fields_) + [("horizon", C.c_void_p), ("n_step", C.c_int32), ("head_slot", C.c_int64)]


NSRing, NSAdam = PDDRing, PDDAdam   # mi_ns_ring_t, mi_ns_adam_t

_VP, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SIGNATURES = {
    "mi_ns_version": (_I, []),
    "mi_ns_last_error": (C.c_char_p, []),
    "mi_ns_source_id": (C.c_char_p, []),
    "mi_ns_workspace_bytes": (_SZ, [_I]),
    "mi_ns_target": (_I, [C.POINTER(NSRing), C.POINTER(NSBatch), _VP]),
    "mi_ns_grad": (_I, [C.POINTER(NSRing), C.POINTER(NSBatch), _VP]),
    "mi_ns_update": (_I, [C.POINTER(NSRing), C.POINTER(NSBatch), C.POINTER(NSAdam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_ns", "n-step dueling Double DQN")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = NSRing, NSBatch, NSAdam


def workspace_bytes(batch):
    return lib().mi_ns_workspace_bytes(batch)


def target(ring, batch, stream):
    check(lib().mi_ns_target(C.byref(ring), C.byref(batch), stream), "mi_ns_target")


def grad(ring, batch, stream):
    check(lib().mi_ns_grad(C.byref(ring), C.byref(batch), stream), "mi_ns_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_ns_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_ns_update")
