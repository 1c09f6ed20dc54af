"""CPU-only checks of the eighth library's boundary: libmirl_nstep.so loads without a GPU, exports and binds every symbol include/mi_nstep.h declares, shares its
ring and Adam layouts and its batch prefix with libmirl_pdd.so, reports errors through return codes — the walk's own arguments included — and leaves the seven
older libraries what their own sources give."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

import _libsrc as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep_rl_amd", "csrc")
NS_ALLSRC = S.ALLSRC["_native_ns"]


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_ddqn, _native_iqn, _native_ns, _native_pdd, _native_pg, _native_qr

    if not all(os.path.exists(m.SO_PATH) for m in (_native_ns, _native_pdd, _native_ddqn, _native_qr, _native_c51, _native_iqn, _native_pg, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_ns


def _header(name="mi_nstep.h"):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_ns_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_ns_" + n for n in ("version", "last_error", "source_id", "workspace_bytes", "target", "grad", "update")}      # no acting, no forward
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_nstep.so does not export %s" % name
    assert not hasattr(L, "mi_ns_forward") and not hasattr(L, "mi_ns_act_steps")
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_ns_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_NS_VERSION (\d+)", hdr).group(1))
    from deep_rl_amd import _native_pdd as PD
    pdd = _header("mi_pdd.h")
    for macro, value in (("NPARAMS", K.NPARAMS), ("H1", K.H1), ("H2", K.H2), ("W1", K.OFF_W1), ("B1", K.OFF_B1), ("W2", K.OFF_W2), ("B2", K.OFF_B2), ("WV", K.OFF_WV),
                         ("BV", K.OFF_BV), ("WA", K.OFF_WA), ("BA", K.OFF_BA), ("MAX_SLABS", K.MAX_SLABS), ("SLAB_STRIDE", K.SLAB_STRIDE)):
        assert int(re.search(r"#define MI_NS_%s (\d+)" % macro, hdr).group(1)) == value == int(re.search(r"#define MI_PDD_%s (\d+)" % macro, pdd).group(1)), macro
    assert int(re.search(r"#define MI_NS_MAX_N (\d+)", hdr).group(1)) == K.MAX_N == 16
    assert (K.NPARAMS, K.MAX_SLABS, K.SLAB_STRIDE) == (PD.NPARAMS, PD.MAX_SLABS, PD.SLAB_STRIDE) == (11_019, 128, 11_020)
    assert hasattr(K, "Ring") and hasattr(K, "Batch") and hasattr(K, "AdamArgs") and callable(K.workspace_bytes) and callable(K.grad) and callable(K.update) and callable(K.target)
    src = open(os.path.join(CSRC, "mi_nstep.hip")).read()
    walk = open(os.path.join(CSRC, "mi_nwalk.h")).read()
    assert "static_assert(MI_NS_W1 == TS_W1 && MI_NS_B1 == TS_B1 && MI_NS_W2 == TS_W2 && MI_NS_B2 == TS_B2" in src and "static_assert(MI_NS_MAX_N == NW_MAX_N" in src
    assert '#include "mi_nwalk.h"' in src and "rg_check_batch(" in src and "rg_check_opt(" in src and "rg_launch_grad<" in src and "rg_check_ring(" in src
    for text in (src, walk, open(os.path.join(CSRC, "mi_dueling.h")).read()):
        assert "asm" not in text and "atomicAdd(" not in text
    assert '#include "mi_dueling.h"' in src and "template <bool ROW, bool NEXT>" not in src      # the head and the batch row are the shared header's, not a copy
    assert "__syncthreads" not in walk and "__shared__" not in walk and "truncation" in walk and "truncation" in open(os.path.join(ROOT, "include", "mi_nstep.h")).read()


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2),", r"\1;", body))


def test_struct_layouts_match_header_and_pdd(K):
    hdr, pd = _header(), _header("mi_pdd.h")
    from deep_rl_amd import _native_pdd as PD
    assert _struct_fields(hdr, "mi_ns_ring_t") == [f[0] for f in K.NSRing._fields_] == _struct_fields(pd, "mi_pdd_ring_t")
    assert _struct_fields(hdr, "mi_ns_adam_t") == [f[0] for f in K.NSAdam._fields_] == _struct_fields(pd, "mi_pdd_adam_t")
    assert _struct_fields(hdr, "mi_ns_batch_t") == [f[0] for f in K.NSBatch._fields_] == _struct_fields(pd, "mi_pdd_batch_t") + ["horizon", "n_step", "head_slot"]
    # the member TYPES of the shared part are the same text in both headers
    body = lambda h, n: re.sub(r"\s+", " ", re.search(r"typedef struct %s \{(.*?)\}" % n, h, flags=re.S).group(1)).strip()   # noqa: E731
    assert body(hdr, "mi_ns_ring_t") == body(pd, "mi_pdd_ring_t") and body(hdr, "mi_ns_adam_t") == body(pd, "mi_pdd_adam_t")
    assert body(hdr, "mi_ns_batch_t").startswith(body(pd, "mi_pdd_batch_t"))
    assert body(hdr, "mi_ns_batch_t")[len(body(pd, "mi_pdd_batch_t")):].split() == "int32_t* horizon; int32_t n_step; int64_t head_slot;".split()
    assert K.Ring is PD.PDDRing and K.AdamArgs is PD.PDDAdam                                            # one ring struct serves both libraries
    assert all(getattr(K.NSBatch, n).offset == getattr(PD.PDDBatch, n).offset and getattr(K.NSBatch, n).size == getattr(PD.PDDBatch, n).size for n, _ in PD.PDDBatch._fields_)
    assert C.sizeof(PD.PDDBatch) == 128 and (K.NSBatch.horizon.offset, K.NSBatch.n_step.offset, K.NSBatch.head_slot.offset) == (128, 136, 144) and C.sizeof(K.NSBatch) == 152
    assert C.sizeof(K.NSRing) == 4 * 8 + 8 + 4 + 4 and C.sizeof(K.NSAdam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_ns_workspace_bytes(0) == 0 and L.mi_ns_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_ns_workspace_bytes(128) == L.mi_ns_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4 == PD.lib().mi_pdd_workspace_bytes(4096)
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_ns as K
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
# structs that are there but empty are errors too, as are a ring without buffers, a batch of 0 rows, a batch without td_abs and misaligned pointers
r, b, o = K.NSRing(), K.NSBatch(), K.NSAdam()
out["empty:target"] = L.mi_ns_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_ns_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_ns_update(C.byref(r), C.byref(b), C.byref(o), None)
# a ring (4 slots, 1 env) and a batch whose every pointer is set (never dereferenced on the host: every check comes before the launch) but the one under test
r2 = K.NSRing(16, 16, 16, 16, 4, 1, 0)
r3 = K.NSRing(16, 16, 16, 16, 64, 1, 0)   # 64 slots: n_step 17 is out of range by MI_NS_MAX_N alone
out["n_step_17:slots_64"] = [L.mi_ns_target(C.byref(r3), C.byref(K.NSBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, None, 16, 16, 17, 0)), None),
                             L.mi_ns_grad(C.byref(r3), C.byref(K.NSBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, None, 16, 16, 17, 0)), None)]
def batch(**kw):
    b = K.NSBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, None, 16, 16, 3, 0)
    for k, v in kw.items():
        setattr(b, k, v)
    return b
calls = dict(target=lambda b: L.mi_ns_target(C.byref(r2), C.byref(b), None), grad=lambda b: L.mi_ns_grad(C.byref(r2), C.byref(b), None),
             update=lambda b: L.mi_ns_update(C.byref(r2), C.byref(b), C.byref(o), None))
for who, call in calls.items():
    out["n_step_0:" + who] = call(batch(n_step=0))
    out["n_step_17:" + who] = call(batch(n_step=17))
    out["n_step_slots:" + who] = call(batch(n_step=4))
    out["n_step_-1:" + who] = call(batch(n_step=-1))
    out["head_-1:" + who] = call(batch(head_slot=-1))
    out["head_slots:" + who] = call(batch(head_slot=4))
    out["null:horizon:" + who] = call(batch(horizon=None))
    out["text:horizon:" + who] = L.mi_ns_last_error().decode()
out["null:td_abs"] = calls["grad"](batch(td_abs=None))
out["text:td_abs"] = L.mi_ns_last_error().decode()
out["zero:batch"] = calls["grad"](batch(batch=0))
out["misaligned:params"] = calls["grad"](batch(params=20))
out["misaligned:params:target"] = calls["target"](batch(params=20))
out["range:sample_upper"] = calls["grad"](batch(sample_upper=5))
out["null:opt"] = L.mi_ns_update(C.byref(r2), C.byref(batch()), None, None)
out["empty:opt"] = calls["update"](batch())
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_ns_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_ns_last_error().decode()
print("RESULT", json.dumps(out))
"""


def json_result(stdout):
    import json
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("RESULT")][0][7:])


def test_every_entry_point_survives_null_zero_and_out_of_range_arguments(K):
    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json_result(p.stdout)
    text, text_td = res.pop("text"), res.pop("text:td_abs")
    assert res.pop("n_step_17:slots_64") == [-1, -1]
    assert "invalid argument" in text and "a batch buffer is NULL" in text_td
    for who in ("target", "grad", "update"):
        assert "horizon is NULL" in res.pop("text:horizon:" + who)
    assert set(k for k in res if ":" not in k) == set(K.SIGNATURES)
    assert sum(k.startswith(("n_step_", "head_", "null:horizon")) for k in res) == 3 * 7
    harmless = {"mi_ns_version", "mi_ns_last_error", "mi_ns_source_id", "mi_ns_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_NS_EINVAL


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_NS_SO"] = os.path.join(%r, "no_such_libmirl_nstep.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_ns, _native_pdd
assert _native.lib().mi_version() == _native.ABI_VERSION and _native_pdd.lib().mi_pdd_version() == 1
assert deep_rl_amd.NStepDQNEngine is not None and "NStepDQNEngine" in deep_rl_amd.__all__
try:
    _native_ns.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_eighth_library(K):
    """libmirl_nstep.so loads lazily: with it absent `import deep_rl_amd`, libmirl.so and libmirl_pdd.so work, and the first use of the engine's path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_eighth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_pdd_* would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_ns_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_per_sample_current", "mi_dueling_pack", "mi_pg_version", "mi_c51_version", "mi_iqn_version",
                  "mi_qr_version", "mi_ddqn_version", "mi_pdd_version", "mi_pdd_forward", "mi_pdd_act_steps"):
        assert not hasattr(L, other), other


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles_without_scratch():
    """every kernel of the library: no scratch, no spilled vector register (the figures DESIGN §20 quotes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_nstep.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("ns_target_kernel", "ns_grad_kernel", "ns_reduce_kernel"))
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * 3
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * 3
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)) <= 256


def test_the_other_libraries_are_still_what_their_sources_give(K):
    """the feature changes no token of the seven older libraries or of the shared headers: their source ids are what their own sources give and what the committed
    profiles recorded, and the new library has an id of its own that csrc/srcid.py reproduces"""
    import json

    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C5
    from deep_rl_amd import _native_ddqn as DQ
    from deep_rl_amd import _native_iqn as IQ
    from deep_rl_amd import _native_pdd as PD
    from deep_rl_amd import _native_pg as PG
    from deep_rl_amd import _native_qr as QR

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = lambda var: re.search(r"^%s = (.*)$" % var, mk, flags=re.M).group(1).split()   # noqa: E731
    older = (("ALLSRC", N.lib().mi_source_id().decode()), ("PG_ALLSRC", PG.source_id()), ("C51_ALLSRC", C5.source_id()), ("IQN_ALLSRC", IQ.source_id()),
             ("QR_ALLSRC", QR.source_id()), ("DDQN_ALLSRC", DQ.source_id()), ("PDD_ALLSRC", PD.source_id()))
    srcs = S.SRCS
    for var, sid in older:
        files = allsrc(var)
        assert "mi_nwalk.h" not in files and "mi_nstep.hip" not in files
        assert srcid(srcs + files[1:] if var == "ALLSRC" else files) == sid, var
    prof = lambda name: json.load(open(os.path.join(ROOT, "profiles", name)))   # noqa: E731
    assert prof("latest_pmc.json").get("source_id") == older[0][1] and prof("ddqn_bench.json")["ddqn_source_id"] == DQ.source_id()
    assert prof("pdd_bench.json")["pdd_source_id"] == PD.source_id()                               # mi_ring.h / mi_torso.h / mi_common.h / mi_pdd.hip did not move
    assert allsrc("NS_ALLSRC") == NS_ALLSRC and srcid(NS_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "nstep_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["nstep_source_id"] == K.source_id()
    assert len({sid for _, sid in older} | {K.source_id()}) == 8
    assert "$(OUT_NS)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_NS)" in mk.split("clean:")[1]
    assert "-DMI_NS_SOURCE_ID" in mk and "OUT_NS ?= ../libmirl_nstep.so" in mk
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_native_ns.lib().mi_ns_version() == _native_ns.ABI_VERSION" in entry


def test_engine_surface_is_callable_where_it_must_be():
    """PDDDQNEngine's surface plus n_step: acting, forward, the sampler and the priority bookkeeping are inherited, the training calls go through the new library"""
    import inspect

    from deep_rl_amd import NStepDQNEngine, PDDDQNEngine, _native_ns, checkpoint

    assert issubclass(NStepDQNEngine, PDDDQNEngine) and NStepDQNEngine.K is _native_ns
    for name in ("act", "forward", "sample", "beta", "refresh_sums", "_scatter", "grad", "reset", "drain_episodes", "sync_target"):
        assert getattr(NStepDQNEngine, name) is getattr(PDDDQNEngine, name), name
    for name in ("_batch", "target", "train_step", "__init__"):
        assert name in vars(NStepDQNEngine) and inspect.isfunction(vars(NStepDQNEngine)[name]), name
    sig = inspect.signature(NStepDQNEngine.__init__)
    assert list(sig.parameters)[1:] == list(inspect.signature(PDDDQNEngine.__init__).parameters)[1:] + ["n_step"] and sig.parameters["n_step"].default == 3
    src = inspect.getsource(sys.modules[NStepDQNEngine.__module__])
    assert "self.horizon = " in src and "self.global_step % self.slots" in src and "mi_pdd" not in src.replace("mi_pdd_update", "")
    ck = inspect.getsource(checkpoint)
    assert ck.count("NStepDQNEngine") >= 3 and "n_step" in ck
    script = open(os.path.join(ROOT, "deep_rl_amd", "nstep_dqn.py")).read()
    assert 'os.environ.get("N_STEP", "3")' in script and "NStepDQNEngine(" in script and 'os.environ.get("PRIORITIZED", "1")' in script
