"""ctypes binding of libmirl_noisy.so — the C ABI declared in include/mi_noisy.h (noisy-net exploration on n-step prioritized dueling Double DQN on CartPole-v1).

A ninth library beside libmirl.so, libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so, libmirl_pdd.so and libmirl_nstep.so.  It is loaded
LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so present, and the first use of the engine without a built
``deep_rl_amd/libmirl_noisy.so`` raises ``MiError`` — there is no fallback.  Build all nine with ``make -C deep_rl_amd/csrc``.

Its ring and Adam structs are layout-identical to libmirl_pdd.so's (the header says so, tests/test_noisy_abi_cpu.py checks it), so ``Ring`` and ``AdamArgs`` ARE
_native_pdd's classes; the batch is _native_ns's with ``noisy`` behind it, the act struct _native_pdd's with ``noisy`` behind it.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)
from ._native_ns import NSBatch
from ._native_pdd import PDDAct, PDDAdam, PDDRing

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_NZ_SO", os.path.join(_HERE, "libmirl_noisy.so"))  # MIRL_NZ_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_NZ_VERSION of the include/mi_noisy.h these signatures and struct layouts were written against
NPARAMS = 11274
H1, H2 = 120, 84
OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_WV, OFF_BV, OFF_WA, OFF_BA, OFF_SIGMA = 0, 480, 600, 10680, 10764, 10848, 10849, 11017, 11019
NHEAD, NXI = 255, 171
MAX_SLABS = 128
SLAB_STRIDE = 11276
MAX_N = 16
MAX_STEPS_PER_CALL = 64
STREAM_ACT, STREAM_LEARN = 13, 14
MI_NZ_OK = 0


class NZAct(C.Structure):   # mi_nz_act_t: mi_pdd_act_t with noisy behind it
    _fields_ = list(PDDAct._fields_) + [("noisy", C.c_int32), ("reserved", C.c_int32)]


class NZBatch(C.Structure):   # mi_nz_batch_t: mi_ns_batch_t with noisy behind it
    _fields_ = list(NSBatch._fields_) + [("noisy", C.c_int32), ("reserved", C.c_int32)]


class NZKey(C.Structure):   # mi_nz_key_t
    _fields_ = [("seed", C.c_uint64), ("a", C.c_uint64), ("b", C.c_uint64), ("stream", C.c_uint32), ("reserved", C.c_uint32)]


NZRing, NZAdam = PDDRing, PDDAdam   # mi_nz_ring_t, mi_nz_adam_t

_VP, _I, _SZ, _U64 = C.c_void_p, C.c_int, C.c_size_t, C.c_uint64
SIGNATURES = {
    "mi_nz_version": (_I, []),
    "mi_nz_last_error": (C.c_char_p, []),
    "mi_nz_source_id": (C.c_char_p, []),
    "mi_nz_workspace_bytes": (_SZ, [_I]),
    "mi_nz_noise": (_I, [_U64, _U64, _U64, C.c_uint32, _VP, _VP, _VP]),
    "mi_nz_forward": (_I, [_VP, _VP, _I, C.POINTER(NZKey), _VP, _VP]),
    "mi_nz_act_steps": (_I, [_VP, C.POINTER(NZRing), C.POINTER(NZAct), _VP]),
    "mi_nz_target": (_I, [C.POINTER(NZRing), C.POINTER(NZBatch), _VP]),
    "mi_nz_grad": (_I, [C.POINTER(NZRing), C.POINTER(NZBatch), _VP]),
    "mi_nz_update": (_I, [C.POINTER(NZRing), C.POINTER(NZBatch), C.POINTER(NZAdam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_nz", "noisy n-step dueling Double DQN")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = NZRing, NZBatch, NZAdam


def workspace_bytes(batch):
    return lib().mi_nz_workspace_bytes(batch)


def target(ring, batch, stream):
    check(lib().mi_nz_target(C.byref(ring), C.byref(batch), stream), "mi_nz_target")


def grad(ring, batch, stream):
    check(lib().mi_nz_grad(C.byref(ring), C.byref(batch), stream), "mi_nz_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_nz_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_nz_update")


def noise(seed, a, b, stream_tag, xi_out, eps_out, stream):
    """the sample of (seed, a, b, stream_tag) as the kernels form it: xi_out [171] and eps_out [255] float32 device tensors"""
    check(lib().mi_nz_noise(seed, a, b, stream_tag, ptr(xi_out), ptr(eps_out), stream), "mi_nz_noise")
