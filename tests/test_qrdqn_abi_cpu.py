"""CPU-only checks of the fifth library's boundary: libmirl_qr.so loads without a GPU, exports and binds every symbol include/mi_qr.h declares, reports errors
through return codes — and leaves libmirl.so, libmirl_pg.so, libmirl_qr.so and libmirl_iqn.so what the committed profiles describe."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import pytest

import _libsrc as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep_rl_amd", "csrc")
QR_ALLSRC = S.ALLSRC["_native_qr"]


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_iqn, _native_pg, _native_qr

    if not all(os.path.exists(p) for p in (_native_qr.SO_PATH, _native_c51.SO_PATH, _native_iqn.SO_PATH, _native_pg.SO_PATH, _native.SO_PATH)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_qr


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_qr.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_qr_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 10
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_qr.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_qr_version() == K.ABI_VERSION == int(re.search(r"#define MI_QR_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MI_QR_NPARAMS", K.NPARAMS), ("MI_QR_N_QUANT", K.N_QUANT), ("MI_QR_H1", K.H1), ("MI_QR_H2", K.H2), ("MI_QR_W1", K.OFF_W1),
                         ("MI_QR_B1", K.OFF_B1), ("MI_QR_W2", K.OFF_W2), ("MI_QR_B2", K.OFF_B2), ("MI_QR_W3", K.OFF_W3), ("MI_QR_B3", K.OFF_B3),
                         ("MI_QR_MAX_SLABS", K.MAX_SLABS), ("MI_QR_SLAB_STRIDE", K.SLAB_STRIDE), ("MI_QR_MAX_STEPS_PER_CALL", K.MAX_STEPS_PER_CALL)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro
    assert K.NPARAMS == 21_644 == K.OFF_B3 + 2 * K.N_QUANT and K.OFF_W3 + 2 * K.N_QUANT * K.H2 == K.OFF_B3 and K.OFF_W2 + K.H1 * K.H2 == K.OFF_B2
    assert K.SLAB_STRIDE % 4 == 0 and K.SLAB_STRIDE > K.NPARAMS and K.OFF_W3 % 4 == 0 and K.OFF_W2 % 4 == 0


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2),", r"\1;", body))


def test_struct_layouts_match_header(K):
    hdr = _header()
    assert _struct_fields(hdr, "mi_qr_ring_t") == [f[0] for f in K.QRRing._fields_]
    assert _struct_fields(hdr, "mi_qr_act_t") == [f[0] for f in K.QRAct._fields_]
    assert _struct_fields(hdr, "mi_qr_batch_t") == [f[0] for f in K.QRBatch._fields_]
    assert _struct_fields(hdr, "mi_qr_adam_t") == [f[0] for f in K.QRAdam._fields_]
    assert C.sizeof(K.QRRing) == 4 * 8 + 8 + 4 + 4
    assert C.sizeof(K.QRAct) == 6 * 8 + 2 * 8 + 3 * 8 + 4 + 4
    assert C.sizeof(K.QRBatch) == 9 * 8 + 3 * 8 + 4 + 4 + 8
    assert C.sizeof(K.QRAdam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_qr_workspace_bytes(0) == 0 and L.mi_qr_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_qr_workspace_bytes(128) == L.mi_qr_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_qr as K
L, out = K.lib(), {}
for name, (res, args) in sorted(K.SIGNATURES.items()):
    vals = []
    for a in args:
        if a in (C.c_void_p, C.c_char_p) or (hasattr(a, "_type_") and not isinstance(a._type_, str)):
            vals.append(None)
        elif a in (C.c_float, C.c_double):
            vals.append(0.0)
        else:
            vals.append(0)
    r = getattr(L, name)(*vals)
    out[name] = r if isinstance(r, int) else None
    print("DONE", name, flush=True)
# structs that are there but empty are errors too, as are a ring without buffers, a batch of 0 rows and misaligned pointers
r, b, a, o = K.QRRing(), K.QRBatch(), K.QRAct(), K.QRAdam()
out["empty:act"] = L.mi_qr_act_steps(None, C.byref(r), C.byref(a), None)
fake = (C.c_char * 64)()
out["empty:act_handle"] = L.mi_qr_act_steps(C.addressof(fake), C.byref(r), C.byref(a), None)
out["empty:target"] = L.mi_qr_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_qr_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_qr_update(C.byref(r), C.byref(b), C.byref(o), None)
out["empty:huber"] = L.mi_qr_quantile_huber(None, None, 128, None, None, None)
out["misaligned:forward"] = L.mi_qr_forward(4, 4, 1, 4, 4, None)
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_qr_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_qr_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_and_zero_arguments(K):
    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    text = res.pop("text")
    assert "invalid argument" in text
    assert set(k for k in res if ":" not in k) == set(K.SIGNATURES)
    harmless = {"mi_qr_version", "mi_qr_last_error", "mi_qr_source_id", "mi_qr_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_QR_EINVAL


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_QR_SO"] = os.path.join(%r, "no_such_libmirl_qr.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_qr
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.QRDQNEngine is not None and deep_rl_amd.QRQNetwork is not None
try:
    _native_qr.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_fifth_library(K):
    """libmirl_qr.so loads lazily: with it absent `import deep_rl_amd` and libmirl.so work, and the first use of the C51 path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_fifth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_prof_mark would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_qr_version() == K.ABI_VERSION
    assert not hasattr(L, "mi_version") and not hasattr(L, "mi_env_create") and not hasattr(L, "mi_pg_version") and not hasattr(L, "mi_c51_version") and not hasattr(L, "mi_iqn_version")


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + [os.path.join(CSRC, "mi_qr.hip"), "-o", os.path.join(d, "x.o")], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]


def test_the_other_libraries_are_still_the_profiled_ones(K):
    """the feature changes no token of the four older libraries: their source ids are what their own sources and the committed profiles give, and the new library has
    an id of its own that csrc/srcid.py reproduces"""
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C5
    from deep_rl_amd import _native_iqn as IQ
    from deep_rl_amd import _native_pg as PG

    mine = N.lib().mi_source_id().decode()
    rec = json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json")))
    assert rec.get("source_id") == mine

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    assert srcid(S.ALLSRC["_native_pg"]) == PG.source_id()
    assert srcid(S.ALLSRC["_native_c51"]) == C5.source_id()
    assert srcid(S.ALLSRC["_native_iqn"]) == IQ.source_id()
    assert PG.source_id() in open(os.path.join(ROOT, "profiles", "reinforce_bench.json")).read()
    assert json.load(open(os.path.join(ROOT, "profiles", "c51_bench.json")))["c51_source_id"] == C5.source_id()
    assert IQ.source_id() in open(os.path.join(ROOT, "profiles", "iqn_bench.json")).read()
    assert srcid(QR_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "qrdqn_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["qrdqn_source_id"] == K.source_id()
    assert len({mine, PG.source_id(), C5.source_id(), IQ.source_id(), K.source_id()}) == 5
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "QR_ALLSRC = " + " ".join(QR_ALLSRC) in mk and "$(OUT_QR)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_QR)" in mk.split("clean:")[1]


def test_engine_surface_is_callable_where_it_must_be():
    """the surface of C51Engine: methods are methods on the class (an instance attribute of the same name would shadow them); a world size > 1 is a loud error"""
    import inspect

    from deep_rl_amd import QRDQNEngine, checkpoint

    names = ("reset", "act", "drain_episodes", "sample", "target", "grad", "train_step", "sync_target")
    for name in names:
        assert inspect.isfunction(getattr(QRDQNEngine, name)), name
    src = "".join(inspect.getsource(c.__init__) for c in QRDQNEngine.__mro__ if "__init__" in vars(c) and c is not object)   # the base class allocates the ring
    for name in names:
        assert "self.%s =" % name not in src and "self.%s," % name not in src, name
    for name in ("observations", "actions", "rewards", "terminated", "batch_inds", "grads", "loss", "current", "target_quantiles", "next_actions", "episode_stats"):
        assert "self.%s = " % name in src, name
    assert "world_size(process_group) > 1" in src and "raise K.MiError" in src
    assert inspect.getsource(checkpoint).count("QRDQNEngine") >= 5
