"""CPU-only checks of the sixth library's boundary: libmirl_ddqn.so loads without a GPU, exports and binds every symbol include/mi_ddqn.h declares, reports errors
through return codes — and leaves libmirl.so, libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so and libmirl_qr.so what the committed profiles describe."""
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
DDQN_ALLSRC = S.ALLSRC["_native_ddqn"]


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_ddqn, _native_iqn, _native_pg, _native_qr

    if not all(os.path.exists(m.SO_PATH) for m in (_native_ddqn, _native_qr, _native_c51, _native_iqn, _native_pg, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_ddqn


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_ddqn.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_ddqn_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_ddqn_" + n for n in ("version", "last_error", "source_id", "workspace_bytes", "forward", "act_steps", "target", "grad", "update")}
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_ddqn.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_ddqn_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_DDQN_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MI_DDQN_NPARAMS", K.NPARAMS), ("MI_DDQN_H1", K.H1), ("MI_DDQN_H2", K.H2), ("MI_DDQN_W1", K.OFF_W1), ("MI_DDQN_B1", K.OFF_B1),
                         ("MI_DDQN_W2", K.OFF_W2), ("MI_DDQN_B2", K.OFF_B2), ("MI_DDQN_W3", K.OFF_W3), ("MI_DDQN_B3", K.OFF_B3), ("MI_DDQN_MAX_SLABS", K.MAX_SLABS),
                         ("MI_DDQN_SLAB_STRIDE", K.SLAB_STRIDE), ("MI_DDQN_MAX_STEPS_PER_CALL", K.MAX_STEPS_PER_CALL)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro
    from deep_rl_amd import _native as N
    assert K.NPARAMS == 10_934 == N.DQN_NPARAMS == K.OFF_B3 + 2 and K.OFF_W3 + 2 * K.H2 == K.OFF_B3 and K.OFF_W2 + K.H1 * K.H2 == K.OFF_B2   # the QNetwork of libmirl's DQN
    assert K.SLAB_STRIDE % 4 == 0 and K.SLAB_STRIDE > K.NPARAMS and K.OFF_W2 % 4 == 0
    assert hasattr(K, "Ring") and hasattr(K, "Batch") and hasattr(K, "AdamArgs") and callable(K.workspace_bytes) and callable(K.grad) and callable(K.update)


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2),", r"\1;", body))


def test_struct_layouts_match_header(K):
    hdr = _header()
    assert _struct_fields(hdr, "mi_ddqn_ring_t") == [f[0] for f in K.DDQNRing._fields_]
    assert _struct_fields(hdr, "mi_ddqn_act_t") == [f[0] for f in K.DDQNAct._fields_] and "learning_starts" in _struct_fields(hdr, "mi_ddqn_act_t")
    assert _struct_fields(hdr, "mi_ddqn_batch_t") == [f[0] for f in K.DDQNBatch._fields_]
    assert _struct_fields(hdr, "mi_ddqn_adam_t") == [f[0] for f in K.DDQNAdam._fields_]
    for name in ("next_actions", "target", "current", "grads", "loss", "sample_seed", "sample_update", "sample_upper", "mid_event"):
        assert name in _struct_fields(hdr, "mi_ddqn_batch_t"), name
    assert C.sizeof(K.DDQNRing) == 4 * 8 + 8 + 4 + 4
    assert C.sizeof(K.DDQNAct) == 6 * 8 + 3 * 8 + 3 * 8 + 4 + 4
    assert C.sizeof(K.DDQNBatch) == 9 * 8 + 3 * 8 + 4 + 4 + 8
    assert C.sizeof(K.DDQNAdam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_ddqn_workspace_bytes(0) == 0 and L.mi_ddqn_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_ddqn_workspace_bytes(128) == L.mi_ddqn_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_ddqn as K
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
r, b, a, o = K.DDQNRing(), K.DDQNBatch(), K.DDQNAct(), K.DDQNAdam()
out["empty:act"] = L.mi_ddqn_act_steps(None, C.byref(r), C.byref(a), None)
fake = (C.c_char * 64)()
out["empty:act_handle"] = L.mi_ddqn_act_steps(C.addressof(fake), C.byref(r), C.byref(a), None)
out["empty:target"] = L.mi_ddqn_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_ddqn_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_ddqn_update(C.byref(r), C.byref(b), C.byref(o), None)
out["misaligned:forward"] = L.mi_ddqn_forward(4, 4, 1, 4, None)
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_ddqn_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_ddqn_last_error().decode()
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
    harmless = {"mi_ddqn_version", "mi_ddqn_last_error", "mi_ddqn_source_id", "mi_ddqn_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_DDQN_EINVAL


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_DDQN_SO"] = os.path.join(%r, "no_such_libmirl_ddqn.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_ddqn
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.DoubleDQNEngine is not None and "DoubleDQNEngine" in deep_rl_amd.__all__
try:
    _native_ddqn.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_sixth_library(K):
    """libmirl_ddqn.so loads lazily: with it absent `import deep_rl_amd` and libmirl.so work, and the first use of the Double DQN path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_sixth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_prof_mark would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_ddqn_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_pg_version", "mi_c51_version", "mi_iqn_version", "mi_qr_version"):
        assert not hasattr(L, other), other


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + [os.path.join(CSRC, "mi_ddqn.hip"), "-o", os.path.join(d, "x.o")], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]


def test_the_other_libraries_are_still_the_profiled_ones(K):
    """the feature changes no token of the five older libraries: their source ids are what their own sources and the committed profiles give, and the new library
    has an id of its own that csrc/srcid.py reproduces"""
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C5
    from deep_rl_amd import _native_iqn as IQ
    from deep_rl_amd import _native_pg as PG
    from deep_rl_amd import _native_qr as QR

    mine = N.lib().mi_source_id().decode()
    rec = json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json")))
    assert rec.get("source_id") == mine

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    assert srcid(S.ALLSRC["_native_pg"]) == PG.source_id()
    assert srcid(S.ALLSRC["_native_c51"]) == C5.source_id()
    assert srcid(S.ALLSRC["_native_iqn"]) == IQ.source_id()
    assert srcid(S.ALLSRC["_native_qr"]) == QR.source_id()
    assert PG.source_id() in open(os.path.join(ROOT, "profiles", "reinforce_bench.json")).read()
    assert json.load(open(os.path.join(ROOT, "profiles", "c51_bench.json")))["c51_source_id"] == C5.source_id()
    assert IQ.source_id() in open(os.path.join(ROOT, "profiles", "iqn_bench.json")).read()
    qr_bench = os.path.join(ROOT, "profiles", "qrdqn_bench.json")
    if os.path.exists(qr_bench):
        assert json.load(open(qr_bench))["qrdqn_source_id"] == QR.source_id()
    assert srcid(DDQN_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "ddqn_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["ddqn_source_id"] == K.source_id()
    assert len({mine, PG.source_id(), C5.source_id(), IQ.source_id(), QR.source_id(), K.source_id()}) == 6
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "DDQN_ALLSRC = " + " ".join(DDQN_ALLSRC) in mk and "$(OUT_DDQN)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_DDQN)" in mk.split("clean:")[1]
    assert "-DMI_DDQN_SOURCE_ID" in mk
    # the table of tests/_libsrc.py is the Makefile's: every entry equals its `X_ALLSRC =` line, and there is no such line without an entry
    lines = dict(re.findall(r"^(\w*ALLSRC) = (.*)$", mk, re.M))
    assert set(S.ALLSRC) == set(S.MAKE_VAR) and sorted(S.MAKE_VAR.values()) == sorted(lines) and len(lines) == 12
    for mod, files in S.ALLSRC.items():
        assert lines[S.MAKE_VAR[mod]].split() == files, mod
    assert re.search(r"^SRCS\s*= (.*)$", mk, re.M).group(1).split() == S.SRCS
    # mi_qhead.h, the plain head, is in the lists of this library and of libmirl_mdqn.so and in no other
    assert sorted(v for v, line in lines.items() if "mi_qhead.h" in line.split()) == ["DDQN_ALLSRC", "MD_ALLSRC"]


def test_engine_surface_is_callable_where_it_must_be():
    """the surface of QRDQNEngine: methods are methods on the class (an instance attribute of the same name would shadow them); a world size > 1 is a loud error"""
    import inspect

    from deep_rl_amd import DoubleDQNEngine, checkpoint
    from deep_rl_amd._ring_engine import RingEngine

    assert issubclass(DoubleDQNEngine, RingEngine)
    names = ("reset", "act", "drain_episodes", "sample", "target", "grad", "train_step", "sync_target")
    for name in names:
        assert inspect.isfunction(getattr(DoubleDQNEngine, name)), name
    src = "".join(inspect.getsource(c.__init__) for c in DoubleDQNEngine.__mro__ if "__init__" in vars(c) and c is not object)   # the base class allocates the ring
    for name in names:
        assert "self.%s =" % name not in src and "self.%s," % name not in src, name
    for name in ("observations", "actions", "rewards", "terminated", "batch_inds", "grads", "loss", "current", "target_values", "next_actions", "episode_stats"):
        assert "self.%s = " % name in src, name
    assert "world_size(process_group) > 1" in src and "raise K.MiError" in src
    sig = inspect.signature(DoubleDQNEngine.__init__)
    assert list(sig.parameters)[1:] == ["env", "q_network", "target_network", "optimizer", "slots", "batch_size", "gamma", "learning_starts", "start_e", "end_e",
                                        "exploration_fraction", "total_timesteps", "max_episodes_logged", "process_group"]
    assert (sig.parameters["batch_size"].default, sig.parameters["gamma"].default, sig.parameters["learning_starts"].default,
            sig.parameters["total_timesteps"].default) == (128, 0.99, 10_000, 100_000)
    assert inspect.getsource(checkpoint).count("DoubleDQNEngine") >= 5
