"""CPU-only checks of the twelfth library's boundary: libmirl_mdqn.so loads without a GPU, exports and binds every symbol include/mi_mdqn.h declares, lays its structs
out as libmirl_ddqn.so's with the Munchausen members behind them, reports errors through return codes, keeps every kernel out of scratch — and leaves the older
libraries what their own sources give."""
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
MD_ALLSRC = S.ALLSRC["_native_md"]


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_ddqn, _native_md

    if not all(os.path.exists(m.SO_PATH) for m in (_native_md, _native_ddqn, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_md


def _header(name="mi_mdqn.h"):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_md_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_md_" + n for n in ("version", "last_error", "source_id", "workspace_bytes", "target", "grad", "update")}      # no acting, no forward
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_mdqn.so does not export %s" % name
    assert not hasattr(L, "mi_md_forward") and not hasattr(L, "mi_md_act_steps")
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_md_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_MD_VERSION (\d+)", hdr).group(1))
    dd = _header("mi_ddqn.h")
    for macro, value in (("NPARAMS", K.NPARAMS), ("H1", K.H1), ("H2", K.H2), ("W1", K.OFF_W1), ("B1", K.OFF_B1), ("W2", K.OFF_W2), ("B2", K.OFF_B2), ("W3", K.OFF_W3),
                         ("B3", K.OFF_B3), ("MAX_SLABS", K.MAX_SLABS), ("SLAB_STRIDE", K.SLAB_STRIDE)):
        assert int(re.search(r"#define MI_MD_%s (\d+)" % macro, hdr).group(1)) == value == int(re.search(r"#define MI_DDQN_%s (\d+)" % macro, dd).group(1)), macro
    assert hasattr(K, "Ring") and hasattr(K, "Batch") and hasattr(K, "AdamArgs")
    assert all(callable(getattr(K, n)) for n in ("workspace_bytes", "grad", "update", "target"))
    assert "MIRL_MDQN_SO" in open(os.path.join(ROOT, "deep_rl_amd", "_native_md.py")).read()


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2),", r"\1;", body))


def test_struct_layouts_match_header_and_ddqn(K):
    hdr, dd = _header(), _header("mi_ddqn.h")
    from deep_rl_amd import _native_ddqn as DQ
    assert _struct_fields(hdr, "mi_md_ring_t") == [f[0] for f in K.MDRing._fields_] == _struct_fields(dd, "mi_ddqn_ring_t")
    assert _struct_fields(hdr, "mi_md_adam_t") == [f[0] for f in K.MDAdam._fields_] == _struct_fields(dd, "mi_ddqn_adam_t")
    assert _struct_fields(hdr, "mi_md_batch_t") == [f[0] for f in K.MDBatch._fields_] == _struct_fields(dd, "mi_ddqn_batch_t") + ["bonus", "soft_value", "alpha", "tau", "clip_lo"]
    # the member TYPES of the shared part are the same text in both headers
    body = lambda h, n: re.sub(r"\s+", " ", re.search(r"typedef struct %s \{(.*?)\}" % n, h, flags=re.S).group(1)).strip()   # noqa: E731
    assert body(hdr, "mi_md_ring_t") == body(dd, "mi_ddqn_ring_t") and body(hdr, "mi_md_adam_t") == body(dd, "mi_ddqn_adam_t")
    assert body(hdr, "mi_md_batch_t").startswith(body(dd, "mi_ddqn_batch_t"))
    assert body(hdr, "mi_md_batch_t")[len(body(dd, "mi_ddqn_batch_t")):].split() == "float* bonus; float* soft_value; float alpha; float tau; float clip_lo;".split()
    assert K.Ring is DQ.DDQNRing and K.AdamArgs is DQ.DDQNAdam                                          # one ring struct serves both libraries
    assert all(getattr(K.MDBatch, n).offset == getattr(DQ.DDQNBatch, n).offset and getattr(K.MDBatch, n).size == getattr(DQ.DDQNBatch, n).size for n, _ in DQ.DDQNBatch._fields_)
    assert C.sizeof(DQ.DDQNBatch) == 112
    assert [getattr(K.MDBatch, n).offset for n in ("bonus", "soft_value", "alpha", "tau", "clip_lo")] == [112, 120, 128, 132, 136] and C.sizeof(K.MDBatch) == 144
    assert C.sizeof(K.MDRing) == 4 * 8 + 8 + 4 + 4 and C.sizeof(K.MDAdam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_md_workspace_bytes(0) == 0 and L.mi_md_workspace_bytes(-3) == 0 and L.mi_md_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_md_workspace_bytes(128) == L.mi_md_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4 == DQ.lib().mi_ddqn_workspace_bytes(4096)
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_md as K
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
# structs that are there but empty are errors too, as are a ring without buffers, a batch of 0 rows, a missing output and misaligned pointers
r, b, o = K.MDRing(), K.MDBatch(), K.MDAdam()
out["empty:target"] = L.mi_md_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_md_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_md_update(C.byref(r), C.byref(b), C.byref(o), None)
# a ring (4 slots, 1 env) and a batch whose every pointer is set (never dereferenced on the host: every check comes before the launch) but the one under test
r2 = K.MDRing(16, 16, 16, 16, 4, 1, 0)
def batch(**kw):
    b = K.MDBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, 16, 16, 0.9, 0.03, -1.0)
    for k, v in kw.items():
        setattr(b, k, v)
    return b
calls = dict(target=lambda b: L.mi_md_target(C.byref(r2), C.byref(b), None), grad=lambda b: L.mi_md_grad(C.byref(r2), C.byref(b), None),
             update=lambda b: L.mi_md_update(C.byref(r2), C.byref(b), C.byref(o), None))
inf, nan = float("inf"), float("nan")
for who, call in calls.items():
    for key, kw in (("tau_0", dict(tau=0.0)), ("tau_neg", dict(tau=-0.03)), ("tau_inf", dict(tau=inf)), ("tau_nan", dict(tau=nan)), ("tau_subnormal", dict(tau=1e-45)),
                    ("alpha_inf", dict(alpha=inf)), ("alpha_nan", dict(alpha=nan)), ("clip_pos", dict(clip_lo=0.5)), ("clip_nan", dict(clip_lo=nan)),
                    ("null:bonus", dict(bonus=None)), ("null:soft_value", dict(soft_value=None)), ("null:target", dict(target=None)),
                    ("null:next_actions", dict(next_actions=None)), ("null:idx", dict(idx=None)), ("null:target_params", dict(target_params=None)),
                    ("misaligned:target_params", dict(target_params=20)), ("zero:batch", dict(batch=0)), ("neg:batch", dict(batch=-5))):
        out[key + ":" + who] = call(batch(**kw))
        out["text:" + key + ":" + who] = L.mi_md_last_error().decode()
for who in ("grad", "update"):
    for key, kw in (("null:current", dict(current=None)), ("null:grads", dict(grads=None)), ("null:loss", dict(loss=None)), ("null:workspace", dict(workspace=None)),
                    ("null:params", dict(params=None)), ("misaligned:params", dict(params=20)), ("misaligned:workspace", dict(workspace=24)),
                    ("range:sample_upper", dict(sample_upper=5)), ("neg:sample_upper", dict(sample_upper=-1))):
        out[key + ":" + who] = calls[who](batch(**kw))
out["null:ring"] = L.mi_md_grad(None, C.byref(batch()), None)
out["null:batch"] = L.mi_md_grad(C.byref(r2), None, None)
out["misaligned:observations"] = L.mi_md_target(C.byref(K.MDRing(20, 16, 16, 16, 4, 1, 0)), C.byref(batch()), None)
out["slots_1"] = L.mi_md_target(C.byref(K.MDRing(16, 16, 16, 16, 1, 1, 0)), C.byref(batch()), None)
out["null:opt"] = L.mi_md_update(C.byref(r2), C.byref(batch()), None, None)
out["empty:opt"] = calls["update"](batch())
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_md_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_md_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_zero_and_out_of_range_arguments(K):
    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    assert "invalid argument" in res.pop("text")
    texts = {k[5:]: res.pop(k) for k in list(res) if k.startswith("text:")}
    for who in ("target", "grad", "update"):
        for key in ("tau_0", "tau_neg", "tau_inf", "tau_nan", "tau_subnormal"):
            assert "tau must be > 0 and finite" in texts[key + ":" + who], (key, who, texts[key + ":" + who])
        for key in ("clip_pos", "clip_nan"):
            assert "clip_lo must be <= 0" in texts[key + ":" + who], (key, who)
        for key in ("alpha_inf", "alpha_nan"):
            assert "alpha must be finite" in texts[key + ":" + who], (key, who)
    assert set(k for k in res if ":" not in k and k != "slots_1") == set(K.SIGNATURES)
    assert len(res) >= 7 + 3 + 3 * 18 + 2 * 9 + 7
    harmless = {"mi_md_version", "mi_md_last_error", "mi_md_source_id", "mi_md_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_MD_EINVAL


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_MDQN_SO"] = os.path.join(%r, "no_such_libmirl_mdqn.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_ddqn, _native_md
assert _native.lib().mi_version() == _native.ABI_VERSION and _native_ddqn.lib().mi_ddqn_version() == _native_ddqn.ABI_VERSION
assert deep_rl_amd.MunchausenDQNEngine is not None and "MunchausenDQNEngine" in deep_rl_amd.__all__
try:
    _native_md.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_twelfth_library(K):
    """libmirl_mdqn.so loads lazily: with it absent `import deep_rl_amd`, libmirl.so and libmirl_ddqn.so work, and the first use of the engine's path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_twelfth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_ddqn_* would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_md_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_pg_version", "mi_c51_version", "mi_iqn_version", "mi_qr_version", "mi_ddqn_version",
                  "mi_ddqn_forward", "mi_ddqn_act_steps", "mi_pdd_version", "mi_ns_version"):
        assert not hasattr(L, other), other


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles_without_scratch():
    """every kernel of the library: no scratch, no spilled vector register (the figures DESIGN §25 quotes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_mdqn.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("mdqn_target_kernel", "mdqn_grad_kernel", "mdqn_reduce_kernel"))
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * 3
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * 3
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)) <= 256


def test_the_other_libraries_are_still_what_their_sources_give(K):
    """the feature changes no token of the older libraries or of the shared headers: their source ids are what their own sources give and what the committed
    profiles recorded, and the new library has an id of its own that csrc/srcid.py reproduces"""
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_ddqn as DQ
    from deep_rl_amd import _native_ns as NS
    from deep_rl_amd import _native_pdd as PD

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    assert json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json"))).get("source_id") == N.lib().mi_source_id().decode()
    assert srcid(S.ALLSRC["_native_ddqn"]) == DQ.source_id()
    assert json.load(open(os.path.join(ROOT, "profiles", "ddqn_bench.json")))["ddqn_source_id"] == DQ.source_id()
    assert srcid(S.ALLSRC["_native_pdd"]) == PD.source_id()
    assert srcid(S.ALLSRC["_native_ns"]) == NS.source_id()
    assert srcid(MD_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "mdqn_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["mdqn_source_id"] == K.source_id()
    assert len({N.lib().mi_source_id().decode(), DQ.source_id(), PD.source_id(), NS.source_id(), K.source_id()}) == 5
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "MD_ALLSRC = " + " ".join(MD_ALLSRC) in mk and "$(OUT_MD)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_MD)" in mk.split("clean:")[1]
    assert "-DMI_MD_SOURCE_ID" in mk and "OUT_MD ?= ../libmirl_mdqn.so" in mk
    # mi_qhead.h, the plain head, is in the lists of this library and of libmirl_ddqn.so and in no other
    assert sorted(v for v, line in re.findall(r"^(\w*ALLSRC) = (.*)$", mk, re.M) if "mi_qhead.h" in line.split()) == ["DDQN_ALLSRC", "MD_ALLSRC"]
    assert "_native_md.lib().mi_md_version() == _native_md.ABI_VERSION" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_engine_surface_is_callable_where_it_must_be():
    """DoubleDQNEngine's surface plus the three knobs: acting and forward are inherited (libmirl_ddqn.so), the training calls go through the new library"""
    import inspect

    from deep_rl_amd import DoubleDQNEngine, MunchausenDQNEngine, _native_md, checkpoint
    from deep_rl_amd._native import MiError
    from deep_rl_amd._ring_engine import RingEngine

    assert issubclass(MunchausenDQNEngine, DoubleDQNEngine) and MunchausenDQNEngine.K is _native_md
    for name in ("act", "forward", "reset", "drain_episodes", "sample", "sync_target"):
        assert getattr(MunchausenDQNEngine, name) is getattr(DoubleDQNEngine, name), name
    for name in ("grad", "train_step"):
        assert getattr(MunchausenDQNEngine, name) is getattr(RingEngine, name), name                    # they reach the library through K
    assert set(n for n in vars(MunchausenDQNEngine) if not n.startswith("__") or n == "__init__") == {"K", "ALGO", "NEEDS", "__init__", "_batch", "target"}
    sig = inspect.signature(MunchausenDQNEngine.__init__)
    assert list(sig.parameters)[1:] == list(inspect.signature(DoubleDQNEngine.__init__).parameters)[1:] + ["alpha", "tau", "clip_lo"]
    assert (sig.parameters["alpha"].default, sig.parameters["tau"].default, sig.parameters["clip_lo"].default) == (0.9, 0.03, -1.0)
    src = inspect.getsource(sys.modules[MunchausenDQNEngine.__module__])
    assert "self.bonus = " in src and "self.soft_value = " in src and "mi_ddqn" not in src
    # the checks of the constructor come before anything is allocated or loaded
    for kw in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(alpha=float("inf")), dict(clip_lo=0.1)):
        with pytest.raises(MiError, match="tau must be > 0"):
            MunchausenDQNEngine(None, None, None, None, 8, **kw)
    assert "MunchausenDQNEngine" not in inspect.getsource(checkpoint)                                   # checkpoints work through the base class
    script = open(os.path.join(ROOT, "deep_rl_amd", "munchausen_dqn.py")).read()
    for knob in ('"ALPHA", "0.9"', '"TAU", "0.03"', '"CLIP_LO", "-1.0"', "MunchausenDQNEngine(", "alpha=alpha, tau=tau, clip_lo=clip_lo"):
        assert knob in script, knob
