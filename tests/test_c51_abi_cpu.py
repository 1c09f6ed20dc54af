"""CPU-only checks of the third library's boundary: libmirl_c51.so loads without a GPU, exports and binds every symbol include/mi_c51.h declares, reports errors
through return codes — and leaves libmirl.so and libmirl_pg.so what the committed profiles describe."""
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
C51_ALLSRC = S.ALLSRC["_native_c51"]


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_pg

    if not all(os.path.exists(p) for p in (_native_c51.SO_PATH, _native_pg.SO_PATH, _native.SO_PATH)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_c51


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_c51.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_c51_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 9
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_c51.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_c51_version() == K.ABI_VERSION == int(re.search(r"#define MI_C51_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MI_C51_NPARAMS", K.NPARAMS), ("MI_C51_N_ATOMS", K.N_ATOMS), ("MI_C51_H1", K.H1), ("MI_C51_H2", K.H2), ("MI_C51_W1", K.OFF_W1),
                         ("MI_C51_B1", K.OFF_B1), ("MI_C51_W2", K.OFF_W2), ("MI_C51_B2", K.OFF_B2), ("MI_C51_W3", K.OFF_W3), ("MI_C51_B3", K.OFF_B3),
                         ("MI_C51_MAX_SLABS", K.MAX_SLABS), ("MI_C51_SLAB_STRIDE", K.SLAB_STRIDE), ("MI_C51_MAX_STEPS_PER_CALL", K.MAX_STEPS_PER_CALL)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro
    assert K.NPARAMS == 27_934 == K.OFF_B3 + 2 * K.N_ATOMS and K.OFF_W3 + 2 * K.N_ATOMS * K.H2 == K.OFF_B3 and K.OFF_W2 + K.H1 * K.H2 == K.OFF_B2
    assert float(re.search(r"#define MI_C51_V_MIN \((-?[0-9.]+)f\)", hdr).group(1)) == K.V_MIN and float(re.search(r"#define MI_C51_V_MAX ([0-9.]+)f", hdr).group(1)) == K.V_MAX


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2),", r"\1;", body))


def test_struct_layouts_match_header(K):
    hdr = _header()
    assert _struct_fields(hdr, "mi_c51_ring_t") == [f[0] for f in K.C51Ring._fields_]
    assert _struct_fields(hdr, "mi_c51_batch_t") == [f[0] for f in K.C51Batch._fields_]
    assert _struct_fields(hdr, "mi_c51_adam_t") == [f[0] for f in K.C51Adam._fields_]
    assert C.sizeof(K.C51Ring) == 4 * 8 + 8 + 4 + 4
    assert C.sizeof(K.C51Batch) == 9 * 8 + 3 * 8 + 4 + 4 + 8
    assert C.sizeof(K.C51Adam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_c51_workspace_bytes(0) == 0 and L.mi_c51_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_c51_workspace_bytes(128) == L.mi_c51_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_c51 as K
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
# structs that are there but empty are errors too, as are a ring without buffers behind a non-NULL everything-else and a batch of 0 rows
r, b, a = K.C51Ring(), K.C51Batch(), K.C51Adam()
out["empty:act"] = L.mi_c51_act_steps(None, None, 10, 0, C.byref(r), 1.0, 0.05, 0.5, 20000, None, None, None, None, None, 0, None)
out["empty:target"] = L.mi_c51_target(None, C.byref(r), None, 128, 0.99, None, None, None)
out["empty:grad"] = L.mi_c51_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_c51_update(C.byref(r), C.byref(b), C.byref(a), None)
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_c51_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_c51_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_and_zero_arguments(K):
    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    text = res.pop("text")
    assert "invalid argument" in text
    assert set(k for k in res if not k.startswith("empty:")) == set(K.SIGNATURES)
    harmless = {"mi_c51_version", "mi_c51_last_error", "mi_c51_source_id", "mi_c51_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert isinstance(r, int) and r < 0, (name, r)


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_C51_SO"] = os.path.join(%r, "no_such_libmirl_c51.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_c51
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.C51Engine is not None and deep_rl_amd.C51QNetwork is not None
try:
    _native_c51.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_third_library(K):
    """libmirl_c51.so loads lazily: with it absent `import deep_rl_amd` and libmirl.so work, and the first use of the C51 path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_third_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_prof_mark would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_c51_version() == K.ABI_VERSION
    assert not hasattr(L, "mi_version") and not hasattr(L, "mi_env_create") and not hasattr(L, "mi_pg_version")


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + [os.path.join(CSRC, "mi_c51.hip"), "-o", os.path.join(d, "x.o")], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]


def test_the_other_libraries_are_still_the_profiled_ones(K):
    """the feature changes no token of libmirl.so or libmirl_pg.so: their source ids are what the committed profiles and their own sources give, and the new
    library has an id of its own that csrc/srcid.py reproduces"""
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_pg as PG

    mine = N.lib().mi_source_id().decode()
    rec = json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json")))
    assert rec.get("source_id") == mine

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    assert srcid(S.ALLSRC["_native_pg"]) == PG.source_id()
    bench = os.path.join(ROOT, "profiles", "reinforce_bench.json")
    if os.path.exists(bench):
        assert PG.source_id() in open(bench).read()
    assert srcid(C51_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "c51_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["c51_source_id"] == K.source_id()
    assert len({mine, PG.source_id(), K.source_id()}) == 3
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "C51_ALLSRC = " + " ".join(C51_ALLSRC) in mk


def test_engine_surface_is_callable_where_it_must_be():
    """the surface of DQNEngine plus target() / grad(): methods are methods on the class (an instance attribute of the same name would shadow them)"""
    import inspect

    from deep_rl_amd import C51Engine

    for name in ("reset", "act", "drain_episodes", "sample", "target", "grad", "train_step", "sync_target"):
        assert inspect.isfunction(getattr(C51Engine, name)), name
    src = "".join(inspect.getsource(c.__init__) for c in C51Engine.__mro__ if "__init__" in vars(c) and c is not object)   # the base class allocates the ring
    for name in ("reset", "act", "drain_episodes", "sample", "target", "grad", "train_step", "sync_target"):
        assert "self.%s =" % name not in src and "self.%s," % name not in src, name
    for name in ("observations", "actions", "rewards", "terminated", "batch_inds", "grads", "loss", "target_probs", "next_actions", "episode_stats"):
        assert "self.%s = " % name in src, name
