"""CPU-only checks of the ninth library's boundary: libmirl_noisy.so loads without a GPU, exports and binds every symbol include/mi_noisy.h declares, shares its ring
and Adam layouts with libmirl_pdd.so, its batch prefix with libmirl_nstep.so and its act prefix with libmirl_pdd.so, reports errors through return codes, compiles
without scratch, and leaves the eight older libraries what their own sources give."""
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
NZ_ALLSRC = S.ALLSRC["_native_nz"]
ENTRY = ("version", "last_error", "source_id", "workspace_bytes", "noise", "forward", "act_steps", "target", "grad", "update")


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_ddqn, _native_iqn, _native_ns, _native_nz, _native_pdd, _native_pg, _native_qr

    if not all(os.path.exists(m.SO_PATH) for m in (_native_nz, _native_ns, _native_pdd, _native_ddqn, _native_qr, _native_c51, _native_iqn, _native_pg, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_nz


def _header(name="mi_noisy.h"):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_nz_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_nz_" + n for n in ENTRY}
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_noisy.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_nz_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_NZ_VERSION (\d+)", hdr).group(1))
    pdd = _header("mi_pdd.h")
    for macro, value in (("H1", K.H1), ("H2", K.H2), ("W1", K.OFF_W1), ("B1", K.OFF_B1), ("W2", K.OFF_W2), ("B2", K.OFF_B2), ("WV", K.OFF_WV), ("BV", K.OFF_BV),
                         ("WA", K.OFF_WA), ("BA", K.OFF_BA), ("MAX_SLABS", K.MAX_SLABS), ("MAX_STEPS_PER_CALL", K.MAX_STEPS_PER_CALL)):
        assert int(re.search(r"#define MI_NZ_%s (\d+)" % macro, hdr).group(1)) == value == int(re.search(r"#define MI_PDD_%s (\d+)" % macro, pdd).group(1)), macro
    for macro, value in (("NPARAMS", 11274), ("SIGMA", 11019), ("NHEAD", 255), ("NXI", 171), ("SLAB_STRIDE", 11276), ("MAX_N", 16), ("STREAM_ACT", 13), ("STREAM_LEARN", 14)):
        assert int(re.search(r"#define MI_NZ_%s (\d+)" % macro, hdr).group(1)) == value, macro
    assert (K.NPARAMS, K.OFF_SIGMA, K.NHEAD, K.NXI, K.SLAB_STRIDE, K.MAX_N, K.STREAM_ACT, K.STREAM_LEARN) == (11274, 11019, 255, 171, 11276, 16, 13, 14)
    assert K.OFF_SIGMA == int(re.search(r"#define MI_PDD_NPARAMS (\d+)", pdd).group(1)) and K.NPARAMS == K.OFF_SIGMA + K.NHEAD and K.SLAB_STRIDE % 4 == 0 and K.SLAB_STRIDE > K.NPARAMS
    assert hasattr(K, "Ring") and hasattr(K, "Batch") and hasattr(K, "AdamArgs") and all(callable(getattr(K, n)) for n in ("workspace_bytes", "grad", "update", "target", "noise"))
    src = open(os.path.join(CSRC, "mi_noisy.hip")).read()
    assert "static_assert(MI_NZ_W1 == TS_W1 && MI_NZ_B1 == TS_B1 && MI_NZ_W2 == TS_W2 && MI_NZ_B2 == TS_B2" in src and "static_assert(MI_NZ_MAX_N == NW_MAX_N" in src
    for inc in ('#include "mi_nwalk.h"', '#include "mi_ring.h"', '#include "mi_torso.h"', '#include "mi_common.h"'):
        assert inc in src
    for call in ("rg_check_batch(", "rg_check_opt(", "rg_launch_grad<", "rg_check_ring(", "rg_act_prelude(", "rg_act_loop<", "rg_reduce<PD_NP, PD_STRIDE>"):
        assert call in src, call
    assert '#include "mi_dueling.h"' in src and "template <bool ROW, bool NEXT>" not in src      # the head and the batch row are the shared header's, not a copy
    code = re.sub(r"//.*", "", src + open(os.path.join(CSRC, "mi_dueling.h")).read())
    assert "asm" not in code and "atomicAdd(" not in code and "mi_sac" not in code
    # the streams 13 and 14 are new: no other source uses them as a Philox stream tag
    assert "MI_NZ_STREAM_ACT" in src and "MI_NZ_STREAM_LEARN" in src
    tags = []
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".h", ".inc")) and name != "mi_noisy.hip":
            tags += [int(x) for x in re.findall(r"#define \w*STREAM_\w+\s+(\d+)u\b", open(os.path.join(CSRC, name)).read())]
    assert len(tags) >= 12 and max(tags) <= 12


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2|seed|a),", r"\1;", body))


def test_struct_layouts_match_header_pdd_and_nstep(K):
    hdr, pd, ns = _header(), _header("mi_pdd.h"), _header("mi_nstep.h")
    from deep_rl_amd import _native_ns as NS
    from deep_rl_amd import _native_pdd as PD
    assert _struct_fields(hdr, "mi_nz_ring_t") == [f[0] for f in K.NZRing._fields_] == _struct_fields(pd, "mi_pdd_ring_t")
    assert _struct_fields(hdr, "mi_nz_adam_t") == [f[0] for f in K.NZAdam._fields_] == _struct_fields(pd, "mi_pdd_adam_t")
    assert _struct_fields(hdr, "mi_nz_batch_t") == [f[0] for f in K.NZBatch._fields_] == _struct_fields(ns, "mi_ns_batch_t") + ["noisy", "reserved"]
    assert _struct_fields(hdr, "mi_nz_act_t") == [f[0] for f in K.NZAct._fields_] == _struct_fields(pd, "mi_pdd_act_t") + ["noisy", "reserved"]
    assert _struct_fields(hdr, "mi_nz_key_t") == [f[0] for f in K.NZKey._fields_] == ["seed", "a", "b", "stream", "reserved"]
    # the member TYPES of the shared parts are the same text in the headers (comments stripped)
    body = lambda h, n: re.sub(r"\s+", " ", re.search(r"typedef struct %s \{(.*?)\}" % n, h, flags=re.S).group(1)).strip()   # noqa: E731
    assert body(hdr, "mi_nz_ring_t") == body(pd, "mi_pdd_ring_t") and body(hdr, "mi_nz_adam_t") == body(pd, "mi_pdd_adam_t")
    assert body(hdr, "mi_nz_batch_t").startswith(body(ns, "mi_ns_batch_t")) and body(hdr, "mi_nz_batch_t")[len(body(ns, "mi_ns_batch_t")):].split() == "int32_t noisy; int32_t reserved;".split()
    assert body(hdr, "mi_nz_act_t").startswith(body(pd, "mi_pdd_act_t")) and body(hdr, "mi_nz_act_t")[len(body(pd, "mi_pdd_act_t")):].split() == "int32_t noisy; int32_t reserved;".split()
    assert K.Ring is PD.PDDRing and K.AdamArgs is PD.PDDAdam
    assert all(getattr(K.NZBatch, n).offset == getattr(NS.NSBatch, n).offset and getattr(K.NZBatch, n).size == getattr(NS.NSBatch, n).size for n, _ in NS.NSBatch._fields_)
    assert all(getattr(K.NZAct, n).offset == getattr(PD.PDDAct, n).offset and getattr(K.NZAct, n).size == getattr(PD.PDDAct, n).size for n, _ in PD.PDDAct._fields_)
    assert C.sizeof(NS.NSBatch) == 152 and (K.NZBatch.noisy.offset, C.sizeof(K.NZBatch)) == (152, 160)
    assert C.sizeof(PD.PDDAct) == 104 and (K.NZAct.noisy.offset, C.sizeof(K.NZAct)) == (104, 112) and C.sizeof(K.NZKey) == 32 and K.NZKey.stream.offset == 24
    L = K.lib()
    assert L.mi_nz_workspace_bytes(0) == 0 and L.mi_nz_workspace_bytes(-3) == 0 and L.mi_nz_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_nz_workspace_bytes(128) == L.mi_nz_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_nz as K
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
# structs that are there but empty are errors too
r, b, o, a0 = K.NZRing(), K.NZBatch(), K.NZAdam(), K.NZAct()
out["empty:target"] = L.mi_nz_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_nz_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_nz_update(C.byref(r), C.byref(b), C.byref(o), None)
out["empty:act"] = L.mi_nz_act_steps(None, C.byref(r), C.byref(a0), None)
out["text:act"] = L.mi_nz_last_error().decode()
# a ring (4 slots, 1 env) and a batch whose every pointer is set (never dereferenced on the host: every check comes before the launch) but the one under test
r2 = K.NZRing(16, 16, 16, 16, 4, 1, 0)
r3 = K.NZRing(16, 16, 16, 16, 64, 1, 0)   # 64 slots: n_step 17 is out of range by MI_NZ_MAX_N alone
mk = lambda n: K.NZBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, None, 16, 16, n, 0, 1, 0)
out["n_step_17:slots_64"] = [L.mi_nz_target(C.byref(r3), C.byref(mk(17)), None), L.mi_nz_grad(C.byref(r3), C.byref(mk(17)), None)]
def batch(**kw):
    b = mk(3)
    for k, v in kw.items():
        setattr(b, k, v)
    return b
calls = dict(target=lambda b: L.mi_nz_target(C.byref(r2), C.byref(b), None), grad=lambda b: L.mi_nz_grad(C.byref(r2), C.byref(b), None),
             update=lambda b: L.mi_nz_update(C.byref(r2), C.byref(b), C.byref(o), None))
for who, call in calls.items():
    out["n_step_0:" + who] = call(batch(n_step=0))
    out["n_step_17:" + who] = call(batch(n_step=17))
    out["n_step_slots:" + who] = call(batch(n_step=4))
    out["n_step_-1:" + who] = call(batch(n_step=-1))
    out["head_-1:" + who] = call(batch(head_slot=-1))
    out["head_slots:" + who] = call(batch(head_slot=4))
    out["null:horizon:" + who] = call(batch(horizon=None))
    out["text:horizon:" + who] = L.mi_nz_last_error().decode()
out["null:td_abs"] = calls["grad"](batch(td_abs=None))
out["text:td_abs"] = L.mi_nz_last_error().decode()
out["zero:batch"] = calls["grad"](batch(batch=0))
out["misaligned:params"] = calls["grad"](batch(params=20))
out["misaligned:params:target"] = calls["target"](batch(params=20))
out["misaligned:workspace"] = calls["grad"](batch(workspace=24))
out["range:sample_upper"] = calls["grad"](batch(sample_upper=5))
out["null:opt"] = L.mi_nz_update(C.byref(r2), C.byref(batch()), None, None)
out["empty:opt"] = calls["update"](batch())
# forward and noise: NULL, misaligned, a stream tag that does not fit 4 bits
key = K.NZKey(1, 2, 3, 16, 0)
out["forward:stream_16"] = L.mi_nz_forward(16, 16, 1, C.byref(key), 16, None)
out["text:forward"] = L.mi_nz_last_error().decode()
out["forward:misaligned"] = L.mi_nz_forward(20, 16, 1, None, 16, None)
out["forward:n_0"] = L.mi_nz_forward(16, 16, 0, None, 16, None)
out["forward:null_q"] = L.mi_nz_forward(16, 16, 1, None, None, None)
out["noise:stream_16"] = L.mi_nz_noise(1, 2, 3, 16, 16, 16, None)
out["text:noise"] = L.mi_nz_last_error().decode()
out["noise:null_eps"] = L.mi_nz_noise(1, 2, 3, 14, 16, None, None)
out["noise:null_xi"] = L.mi_nz_noise(1, 2, 3, 14, None, 16, None)
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_nz_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_nz_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_zero_and_out_of_range_arguments(K):
    import json

    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    text, text_td = res.pop("text"), res.pop("text:td_abs")
    assert res.pop("n_step_17:slots_64") == [-1, -1]
    assert "invalid argument" in text and "a batch buffer is NULL" in text_td
    assert res.pop("text:act").startswith("mi_nz_act_steps:") and res.pop("text:forward").startswith("mi_nz_forward:") and res.pop("text:noise").startswith("mi_nz_noise:")
    for who in ("target", "grad", "update"):
        t = res.pop("text:horizon:" + who)
        assert "horizon is NULL" in t and t.startswith("mi_nz_target" if who == "target" else "nz_grad"), t      # the entry point (or its one shared body) is named
    assert set(k for k in res if ":" not in k) == set(K.SIGNATURES)
    assert sum(k.startswith(("n_step_", "head_", "null:horizon")) for k in res) == 3 * 7
    harmless = {"mi_nz_version", "mi_nz_last_error", "mi_nz_source_id", "mi_nz_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_NZ_EINVAL


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_NZ_SO"] = os.path.join(%r, "no_such_libmirl_noisy.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_ns, _native_nz, _native_pdd
assert _native.lib().mi_version() == _native.ABI_VERSION and _native_pdd.lib().mi_pdd_version() == 1 and _native_ns.lib().mi_ns_version() == 1
assert deep_rl_amd.NoisyDQNEngine is not None and {"NoisyDQNEngine", "NoisyDuelingQNetwork", "NoisyLinear"} <= set(deep_rl_amd.__all__)
try:
    _native_nz.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_ninth_library(K):
    """libmirl_noisy.so loads lazily: with it absent `import deep_rl_amd` and the older libraries work, and the first use of the engine's path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_ninth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_pdd_* / mi_ns_* would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_nz_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_per_sample_current", "mi_dueling_pack", "mi_pg_version", "mi_c51_version", "mi_iqn_version",
                  "mi_qr_version", "mi_ddqn_version", "mi_pdd_version", "mi_pdd_forward", "mi_pdd_act_steps", "mi_ns_version", "mi_ns_grad"):
        assert not hasattr(L, other), other


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]
KERNELS = ("nz_noise_kernel", "nz_forward_kernel", "nz_target_kernel", "nz_grad_kernel", "nz_reduce_kernel",
           "nz_act_kernelILb0ELb0", "nz_act_kernelILb0ELb1", "nz_act_kernelILb1ELb0", "nz_act_kernelILb1ELb1")   # acting: <teacher-forced, noisy>


def test_device_only_build_compiles_without_scratch():
    """every kernel of the library: no scratch, no spilled vector register (the figures DESIGN §21 quotes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_noisy.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == len(KERNELS) and all(any(k in n for n in names) for k in KERNELS), names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * len(KERNELS)
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * len(KERNELS)
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)) <= 256


def test_the_other_libraries_are_still_what_their_sources_give(K):
    """the feature changes no token of the eight older libraries or of the shared headers: their source ids are what their own sources give and what the committed
    profiles recorded, and the new library has an id of its own that csrc/srcid.py reproduces"""
    import json

    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C5
    from deep_rl_amd import _native_ddqn as DQ
    from deep_rl_amd import _native_iqn as IQ
    from deep_rl_amd import _native_ns as NS
    from deep_rl_amd import _native_pdd as PD
    from deep_rl_amd import _native_pg as PG
    from deep_rl_amd import _native_qr as QR

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = lambda var: re.search(r"^%s = (.*)$" % var, mk, flags=re.M).group(1).split()   # noqa: E731
    older = (("ALLSRC", N.lib().mi_source_id().decode()), ("PG_ALLSRC", PG.source_id()), ("C51_ALLSRC", C5.source_id()), ("IQN_ALLSRC", IQ.source_id()),
             ("QR_ALLSRC", QR.source_id()), ("DDQN_ALLSRC", DQ.source_id()), ("PDD_ALLSRC", PD.source_id()), ("NS_ALLSRC", NS.source_id()))
    srcs = S.SRCS
    for var, sid in older:
        files = allsrc(var)
        assert "mi_noisy.hip" not in files and "../../include/mi_noisy.h" not in files
        assert srcid(srcs + files[1:] if var == "ALLSRC" else files) == sid, var
    prof = lambda name: json.load(open(os.path.join(ROOT, "profiles", name)))   # noqa: E731
    assert prof("latest_pmc.json").get("source_id") == older[0][1] and prof("ddqn_bench.json")["ddqn_source_id"] == DQ.source_id()
    assert prof("pdd_bench.json")["pdd_source_id"] == PD.source_id() and prof("nstep_bench.json")["nstep_source_id"] == NS.source_id()
    assert allsrc("NZ_ALLSRC") == NZ_ALLSRC and srcid(NZ_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "noisy_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["noisy_source_id"] == K.source_id()
    assert len({sid for _, sid in older} | {K.source_id()}) == 9
    assert "$(OUT_NZ)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_NZ)" in mk.split("clean:")[1]
    assert "-DMI_NZ_SOURCE_ID" in mk and "OUT_NZ ?= ../libmirl_noisy.so" in mk
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_native_nz.lib().mi_nz_version() == _native_nz.ABI_VERSION" in entry


def test_engine_and_network_surface():
    """NStepDQNEngine's surface plus noisy: the sampler, the priority bookkeeping, beta() and sync_target are inherited, everything that meets the network goes
    through the new library; the network's flat vector is all mu, then all sigma"""
    import inspect

    import numpy as np
    import torch

    from deep_rl_amd import NoisyDQNEngine, NoisyDuelingQNetwork, NoisyLinear, NStepDQNEngine, PDDDQNEngine, _native_nz, checkpoint

    assert issubclass(NoisyDQNEngine, NStepDQNEngine) and NoisyDQNEngine.K is _native_nz
    for name in ("sample", "beta", "refresh_sums", "_scatter", "grad", "reset", "drain_episodes", "sync_target"):
        assert getattr(NoisyDQNEngine, name) is getattr(PDDDQNEngine, name), name
    for name in ("act", "forward", "_batch", "target", "train_step", "__init__"):
        assert name in vars(NoisyDQNEngine) and inspect.isfunction(vars(NoisyDQNEngine)[name]), name
    sig = inspect.signature(NoisyDQNEngine.__init__)
    assert list(sig.parameters)[1:] == list(inspect.signature(NStepDQNEngine.__init__).parameters)[1:] + ["noisy"]
    assert (sig.parameters["noisy"].default, sig.parameters["start_e"].default, sig.parameters["end_e"].default) == (True, 0.0, 0.0)
    src = inspect.getsource(sys.modules[NoisyDQNEngine.__module__])
    assert "mi_pdd_" not in src and "mi_ns_" not in src.replace("mi_ns_update", "") and "mi_nz_act_steps" in src and "mi_nz_forward" in src
    assert isinstance(NoisyDQNEngine.__new__(NoisyDQNEngine), (NStepDQNEngine, PDDDQNEngine))           # checkpoint.py's isinstance chains know it
    assert "NoisyDQNEngine" in inspect.getsource(checkpoint)

    class Env:
        class observation_space:
            shape = (4,)

        class action_space:
            n = 2

    torch.manual_seed(3)
    net = NoisyDuelingQNetwork(Env, device="cpu")
    lin = net.value_stream
    assert isinstance(lin, NoisyLinear) and isinstance(net.advantage_stream, NoisyLinear) and net.flat.numel() == 11274 and net.flat.dtype == torch.float32
    f = net.flat.numpy()
    b = 1 / np.sqrt(84)
    assert np.abs(f[10764:11019]).max() <= b and np.abs(f[10764:11019]).max() > 0.8 * b and np.allclose(f[11019:], 0.5 / np.sqrt(84), rtol=1e-6, atol=0)
    # views, in the header's order: Wv bv Wa ba, then their sigmas
    for off, p in ((10764, lin.weight_mu), (10848, lin.bias_mu), (10849, net.advantage_stream.weight_mu), (11017, net.advantage_stream.bias_mu),
                   (11019, lin.weight_sigma), (11019 + 84, lin.bias_sigma), (11019 + 85, net.advantage_stream.weight_sigma), (11019 + 253, net.advantage_stream.bias_sigma)):
        assert p.data_ptr() == net.flat.data_ptr() + 4 * off and np.array_equal(p.detach().numpy().reshape(-1), f[off:off + p.numel()]), off
    assert sum(p.numel() for p in net.parameters()) == 11274 and len(list(net.parameters())) == 12
    x = torch.randn(5, 4)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _noisy_ref as Z
    assert np.abs(net(x).detach().numpy() - Z.forward(f, x.numpy())).max() < 1e-5                                    # forward is the mean network
    assert NoisyLinear(84, 2, sigma_0=0.25).weight_sigma.detach().numpy().max() == np.float32(0.25 / np.sqrt(84))
