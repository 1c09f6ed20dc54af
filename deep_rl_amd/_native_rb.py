"""ctypes binding of libmirl_rainbow.so — the C ABI declared in include/mi_rainbow.h (Rainbow: distributional noisy n-step dueling Double DQN on CartPole-v1).

A tenth library beside libmirl.so, libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so, libmirl_pdd.so, libmirl_nstep.so and
libmirl_noisy.so.  It is loaded LAZILY, on the first ``lib()`` call: importing ``deep_rl_amd`` works with only libmirl.so present, and the first use of the engine
without a built ``deep_rl_amd/libmirl_rainbow.so`` raises ``MiError`` — there is no fallback.  Build all ten with ``make -C deep_rl_amd/csrc``.

Its ring, Adam and key structs are layout-identical to libmirl_pdd.so's / libmirl_noisy.so's (the header says so, tests/test_rainbow_abi_cpu.py checks it), so
``Ring``, ``AdamArgs`` and ``RBKey`` ARE those bindings' classes; the act and batch structs are this library's own.
"""
import ctypes as C
import os

from ._native import MiError, lazy_binding, ptr, stream_ptr  # noqa: F401  (MiError, ptr, stream_ptr: re-exported for the engine)
from ._native_nz import NZKey
from ._native_pdd import PDDAct, PDDAdam, PDDRing

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MIRL_RB_SO", os.path.join(_HERE, "libmirl_rainbow.so"))  # MIRL_RB_SO: A/B and diagnostic builds of the same ABI

ABI_VERSION = 1   # == MI_RB_VERSION of the include/mi_rainbow.h these signatures and struct layouts were written against
N_ATOMS = 51
NPARAMS = 36774
H1, H2 = 120, 84
OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_WV, OFF_BV, OFF_WA, OFF_BA, OFF_SIGMA = 0, 480, 600, 10680, 10764, 15048, 15099, 23667, 23769
NHEAD, NROWS, NXI = 13005, 153, 321
MAX_SLABS = 128
SLAB_STRIDE = 36776
MAX_N = 16
MAX_STEPS_PER_CALL = 64
STREAM_ACT, STREAM_LEARN = 13, 14
MI_RB_OK = 0


class RBAct(C.Structure):   # mi_rb_act_t: mi_pdd_act_t with noisy and the support behind it
    _fields_ = list(PDDAct._fields_) + [("noisy", C.c_int32), ("v_min", C.c_float), ("v_max", C.c_float), ("reserved", C.c_int32)]


class RBBatch(C.Structure):   # mi_rb_batch_t
    _fields_ = [(n, C.c_void_p) for n in ("params", "target_params", "idx", "target_probs", "next_actions", "probs", "grads", "loss", "workspace")] + [
        ("sample_seed", C.c_uint64), ("sample_update", C.c_uint64), ("sample_upper", C.c_int64), ("batch", C.c_int32), ("gamma", C.c_float), ("mid_event", C.c_void_p),
        ("weights", C.c_void_p), ("prio", C.c_void_p), ("horizon", C.c_void_p), ("n_step", C.c_int32), ("noisy", C.c_int32), ("head_slot", C.c_int64),
        ("v_min", C.c_float), ("v_max", C.c_float)]


RBRing, RBAdam, RBKey = PDDRing, PDDAdam, NZKey   # mi_rb_ring_t, mi_rb_adam_t, mi_rb_key_t

_VP, _I, _SZ, _U64, _F = C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_float
SIGNATURES = {
    "mi_rb_version": (_I, []),
    "mi_rb_last_error": (C.c_char_p, []),
    "mi_rb_source_id": (C.c_char_p, []),
    "mi_rb_workspace_bytes": (_SZ, [_I]),
    "mi_rb_noise": (_I, [_U64, _U64, _U64, C.c_uint32, _VP, _VP, _VP, _VP]),
    "mi_rb_forward": (_I, [_VP, _VP, _I, C.POINTER(RBKey), _F, _F, _VP, _VP, _VP]),
    "mi_rb_act_steps": (_I, [_VP, C.POINTER(RBRing), C.POINTER(RBAct), _VP]),
    "mi_rb_target": (_I, [C.POINTER(RBRing), C.POINTER(RBBatch), _VP]),
    "mi_rb_grad": (_I, [C.POINTER(RBRing), C.POINTER(RBBatch), _VP]),
    "mi_rb_update": (_I, [C.POINTER(RBRing), C.POINTER(RBBatch), C.POINTER(RBAdam), _VP]),
}

lib, check, source_id = lazy_binding(SO_PATH, SIGNATURES, ABI_VERSION, "mi_rb", "Rainbow")

# what RingEngine (_ring_engine.py) drives, under the same names in every ring-replay binding
Ring, Batch, AdamArgs = RBRing, RBBatch, RBAdam


def workspace_bytes(batch):
    return lib().mi_rb_workspace_bytes(batch)


def target(ring, batch, stream):
    check(lib().mi_rb_target(C.byref(ring), C.byref(batch), stream), "mi_rb_target")


def grad(ring, batch, stream):
    check(lib().mi_rb_grad(C.byref(ring), C.byref(batch), stream), "mi_rb_grad")


def update(ring, batch, adam, stream):
    check(lib().mi_rb_update(C.byref(ring), C.byref(batch), C.byref(adam), stream), "mi_rb_update")


def noise(seed, a, b, stream_tag, xi_out, fin_out, fout_out, stream):
    """the sample of (seed, a, b, stream_tag) as the kernels form it: xi_out [321], fin_out [153, 84] and fout_out [153] float32 device tensors"""
    check(lib().mi_rb_noise(seed, a, b, stream_tag, ptr(xi_out), ptr(fin_out), ptr(fout_out), stream), "mi_rb_noise")
