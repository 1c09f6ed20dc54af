"""CPU-only checks of the second library's boundary: libmirl_pg.so loads without a GPU, exports and binds every symbol include/mi_reinforce.h declares, reports
errors through return codes — and leaves libmirl.so what the committed profiles describe."""
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


@pytest.fixture(scope="module")
def PG():
    from deep_rl_amd import _native, _native_pg

    if not os.path.exists(_native_pg.SO_PATH) or not os.path.exists(_native.SO_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native_pg


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_reinforce.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(PG):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_pg_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 10
    L = C.CDLL(PG.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_pg.so does not export %s" % name
    assert declared == set(PG.SIGNATURES), declared ^ set(PG.SIGNATURES)
    assert PG.lib().mi_pg_version() == PG.ABI_VERSION == int(re.search(r"#define MI_PG_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MI_PG_NPARAMS", PG.NPARAMS), ("MI_PG_MAX_STEPS", PG.MAX_STEPS), ("MI_PG_ROWS", PG.ROWS), ("MI_PG_HID", PG.HID)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value
    assert int(re.search(r"#define MI_PG_STREAM_DROPOUT (\d+)u", hdr).group(1)) == PG.STREAM_DROPOUT >= 8   # 0-5 and 7 belong to libmirl
    assert int(re.search(r"#define MI_PG_KEEP_BELOW (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == PG.KEEP_BELOW == int(0.4 * 2 ** 32)


def test_struct_layouts_match_header(PG):
    hdr = _header()
    body = re.search(r"typedef struct mi_pg_buffers_t \{(.*?)\}", hdr, flags=re.S).group(1)
    fields = re.findall(r"\*\s*([a-z_0-9]+)\s*;", body)
    assert fields == [f[0] for f in PG.PGBuffers._fields_]
    assert C.sizeof(PG.PGBuffers) == 16 * 8
    assert C.sizeof(PG.PGHparams) == 4 + 4 + 8 + 4 * 8
    assert PG.lib().mi_pg_workspace_bytes(1) == 898 * 4 and PG.lib().mi_pg_workspace_bytes(4096) == 1024 * 898 * 4
    sid = PG.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_pg as PG
L, out = PG.lib(), {}
for name, (res, args) in sorted(PG.SIGNATURES.items()):
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
# structs that are there but empty, and an env handle that is not CartPole, are errors too
b, h = PG.PGBuffers(), PG.PGHparams()
out["empty:rollout"] = L.mi_pg_rollout_episodes(None, C.byref(b), None)
out["empty:returns"] = L.mi_pg_returns(C.byref(b), 8, 0.99, None)
out["empty:grad"] = L.mi_pg_grad(C.byref(b), 8, None)
out["empty:update"] = L.mi_pg_update(None, C.byref(b), C.byref(h), None)
out["text"] = L.mi_pg_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_and_zero_arguments(PG):
    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    text = res.pop("text")
    assert "invalid argument" in text
    assert set(k for k in res if not k.startswith("empty:")) == set(PG.SIGNATURES)
    harmless = {"mi_pg_version", "mi_pg_last_error", "mi_pg_source_id", "mi_pg_workspace_bytes"}   # (0 envs need 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert isinstance(r, int) and r < 0, (name, r)


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_PG_SO"] = os.path.join(%r, "no_such_libmirl_pg.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_pg
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.ReinforceEngine is not None and deep_rl_amd.DropoutPolicy is not None
try:
    _native_pg.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_second_library(PG):
    """libmirl_pg.so loads lazily: with it absent `import deep_rl_amd` and libmirl.so work, and the first use of the REINFORCE path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_second_library_needs_no_symbol_of_the_first(PG):
    """ctypes loads both RTLD_LOCAL: an unresolved mi_set_error / mi_prof_mark would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(PG.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_pg_version() == PG.ABI_VERSION
    assert not hasattr(L, "mi_version") and not hasattr(L, "mi_env_create")


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


@pytest.mark.parametrize("defs", [[], ["-DPG_STAMPS"]])
def test_device_only_and_diagnostic_builds_compile(defs):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + defs + [os.path.join(CSRC, "mi_reinforce.hip"), "-o", os.path.join(d, "x.o")], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]


def test_first_library_is_still_the_profiled_one(PG):
    """the feature changes no token of libmirl.so: its source id is the one the committed profiles record, and the new library has an id of its own"""
    from deep_rl_amd import _native as N

    mine = N.lib().mi_source_id().decode()
    rec = json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json")))
    assert rec.get("source_id") == mine
    assert PG.source_id() != mine
    out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + S.ALLSRC["_native_pg"],
                         cwd=CSRC, capture_output=True, text=True, timeout=60)
    assert out.stdout.strip() == PG.source_id()
