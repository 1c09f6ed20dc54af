"""CPU-only checks of the tenth library's boundary: libmirl_rainbow.so loads without a GPU, exports and binds every symbol include/mi_rainbow.h declares, shares
its ring, Adam and key layouts with the older libraries, reports errors through return codes, compiles without scratch, and leaves the nine older libraries what
their own sources give."""
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
RB_ALLSRC = S.ALLSRC["_native_rb"]
ENTRY = ("version", "last_error", "source_id", "workspace_bytes", "noise", "forward", "act_steps", "target", "grad", "update")


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_ddqn, _native_iqn, _native_ns, _native_nz, _native_pdd, _native_pg, _native_qr, _native_rb

    if not all(os.path.exists(m.SO_PATH) for m in (_native_rb, _native_nz, _native_ns, _native_pdd, _native_ddqn, _native_qr, _native_c51, _native_iqn, _native_pg, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_rb


def _header(name="mi_rainbow.h"):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_rb_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_rb_" + n for n in ENTRY}
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_rainbow.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_rb_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_RB_VERSION (\d+)", hdr).group(1))
    for macro, value in (("H1", K.H1), ("H2", K.H2), ("W1", K.OFF_W1), ("B1", K.OFF_B1), ("W2", K.OFF_W2), ("B2", K.OFF_B2), ("WV", K.OFF_WV), ("BV", K.OFF_BV),
                         ("WA", K.OFF_WA), ("BA", K.OFF_BA), ("SIGMA", K.OFF_SIGMA), ("MAX_SLABS", K.MAX_SLABS), ("MAX_STEPS_PER_CALL", K.MAX_STEPS_PER_CALL),
                         ("N_ATOMS", K.N_ATOMS), ("NPARAMS", K.NPARAMS), ("NHEAD", K.NHEAD), ("NROWS", K.NROWS), ("NXI", K.NXI), ("SLAB_STRIDE", K.SLAB_STRIDE),
                         ("MAX_N", K.MAX_N), ("STREAM_ACT", K.STREAM_ACT), ("STREAM_LEARN", K.STREAM_LEARN)):
        assert int(re.search(r"#define MI_RB_%s (\d+)" % macro, hdr).group(1)) == value, macro
    assert (K.N_ATOMS, K.NPARAMS, K.OFF_WV, K.OFF_BV, K.OFF_WA, K.OFF_BA, K.OFF_SIGMA, K.NHEAD, K.NXI, K.SLAB_STRIDE, K.MAX_SLABS, K.MAX_N, K.STREAM_ACT,
            K.STREAM_LEARN) == (51, 36774, 10764, 15048, 15099, 23667, 23769, 13005, 321, 36776, 128, 16, 13, 14)
    assert K.OFF_BV == K.OFF_WV + 51 * 84 and K.OFF_WA == K.OFF_BV + 51 and K.OFF_BA == K.OFF_WA + 2 * 51 * 84 and K.OFF_SIGMA == K.OFF_BA + 102
    assert K.NPARAMS == K.OFF_SIGMA + K.NHEAD and K.NXI == 84 + 51 + 84 + 102 and K.SLAB_STRIDE % 4 == 0 and K.SLAB_STRIDE > K.NPARAMS
    assert hasattr(K, "Ring") and hasattr(K, "Batch") and hasattr(K, "AdamArgs") and all(callable(getattr(K, n)) for n in ("workspace_bytes", "grad", "update", "target", "noise"))
    src = open(os.path.join(CSRC, "mi_rainbow.hip")).read()
    assert "static_assert(MI_RB_W1 == TS_W1 && MI_RB_B1 == TS_B1 && MI_RB_W2 == TS_W2 && MI_RB_B2 == TS_B2" in src and "static_assert(MI_RB_MAX_N == NW_MAX_N" in src
    for inc in ('#include "mi_nwalk.h"', '#include "mi_ring.h"', '#include "mi_torso.h"', '#include "mi_common.h"'):
        assert inc in src
    for call in ("rg_check_batch(", "rg_check_opt(", "rg_launch_grad<", "rg_check_ring(", "rg_act_prelude(", "rg_act_loop<", "rg_reduce<RB_NP, RB_STRIDE>", "nw_walk("):
        assert call in src, call
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomicAdd(" not in code and "mi_sac" not in code and "mi_noisy" not in code
    full = open(os.path.join(ROOT, "include", "mi_rainbow.h")).read()
    assert "ONLY TAG 15 IS FREE" in full and "not the KL divergence" in full          # what the header has to say about the stream tags and the priority


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2|seed|a),", r"\1;", body))


def test_struct_layouts_match_header_and_older_libraries(K):
    hdr, pd, nz = _header(), _header("mi_pdd.h"), _header("mi_noisy.h")
    from deep_rl_amd import _native_nz as NZ
    from deep_rl_amd import _native_pdd as PD
    assert _struct_fields(hdr, "mi_rb_ring_t") == [f[0] for f in K.RBRing._fields_] == _struct_fields(pd, "mi_pdd_ring_t")
    assert _struct_fields(hdr, "mi_rb_adam_t") == [f[0] for f in K.RBAdam._fields_] == _struct_fields(pd, "mi_pdd_adam_t")
    assert _struct_fields(hdr, "mi_rb_key_t") == [f[0] for f in K.RBKey._fields_] == _struct_fields(nz, "mi_nz_key_t") == ["seed", "a", "b", "stream", "reserved"]
    assert _struct_fields(hdr, "mi_rb_batch_t") == [f[0] for f in K.RBBatch._fields_]
    assert _struct_fields(hdr, "mi_rb_act_t") == [f[0] for f in K.RBAct._fields_] == _struct_fields(pd, "mi_pdd_act_t") + ["noisy", "v_min", "v_max", "reserved"]
    body = lambda h, n: re.sub(r"\s+", " ", re.search(r"typedef struct %s \{(.*?)\}" % n, h, flags=re.S).group(1)).strip()   # noqa: E731
    assert body(hdr, "mi_rb_ring_t") == body(pd, "mi_pdd_ring_t") and body(hdr, "mi_rb_adam_t") == body(pd, "mi_pdd_adam_t") and body(hdr, "mi_rb_key_t") == body(nz, "mi_nz_key_t")
    assert body(hdr, "mi_rb_act_t").startswith(body(pd, "mi_pdd_act_t"))
    assert body(hdr, "mi_rb_act_t")[len(body(pd, "mi_pdd_act_t")):].split() == "int32_t noisy; float v_min; float v_max; int32_t reserved;".split()
    # the member types of the batch, in the header's order
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "int64_t*": C.c_void_p, "int32_t*": C.c_void_p, "void*": C.c_void_p, "uint64_t": C.c_uint64,
             "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    decl = [d.strip().rsplit(" ", 1) for d in body(hdr, "mi_rb_batch_t").split(";") if d.strip()]
    assert [(n, ctype[t]) for t, n in decl] == list(K.RBBatch._fields_)
    assert K.Ring is PD.PDDRing and K.AdamArgs is PD.PDDAdam and K.RBKey is NZ.NZKey
    assert all(getattr(K.RBAct, n).offset == getattr(PD.PDDAct, n).offset and getattr(K.RBAct, n).size == getattr(PD.PDDAct, n).size for n, _ in PD.PDDAct._fields_)
    assert C.sizeof(PD.PDDAct) == 104 and (K.RBAct.noisy.offset, K.RBAct.v_min.offset, K.RBAct.v_max.offset, C.sizeof(K.RBAct)) == (104, 108, 112, 120)
    B = K.RBBatch
    assert (B.workspace.offset, B.sample_seed.offset, B.batch.offset, B.gamma.offset, B.mid_event.offset, B.weights.offset, B.prio.offset, B.horizon.offset, B.n_step.offset,
            B.noisy.offset, B.head_slot.offset, B.v_min.offset, B.v_max.offset, C.sizeof(B)) == (64, 72, 96, 100, 104, 112, 120, 128, 136, 140, 144, 152, 156, 160)
    L = K.lib()
    assert L.mi_rb_workspace_bytes(0) == 0 and L.mi_rb_workspace_bytes(-3) == 0 and L.mi_rb_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_rb_workspace_bytes(128) == L.mi_rb_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_rb as K
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
r, b, o, a0 = K.RBRing(), K.RBBatch(), K.RBAdam(), K.RBAct()
out["empty:target"] = L.mi_rb_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_rb_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_rb_update(C.byref(r), C.byref(b), C.byref(o), None)
out["empty:act"] = L.mi_rb_act_steps(None, C.byref(r), C.byref(a0), None)
out["text:act"] = L.mi_rb_last_error().decode()
# a ring (4 slots, 1 env) and a batch whose every pointer is set (never dereferenced on the host: every check comes before the launch) but the one under test
r2 = K.RBRing(16, 16, 16, 16, 4, 1, 0)
r3 = K.RBRing(16, 16, 16, 16, 64, 1, 0)   # 64 slots: n_step 17 is out of range by MI_RB_MAX_N alone
mk = lambda n: K.RBBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, None, 16, 16, n, 1, 0, 0.0, 100.0)
out["n_step_17:slots_64"] = [L.mi_rb_target(C.byref(r3), C.byref(mk(17)), None), L.mi_rb_grad(C.byref(r3), C.byref(mk(17)), None)]
def batch(**kw):
    b = mk(3)
    for k, v in kw.items():
        setattr(b, k, v)
    return b
calls = dict(target=lambda b: L.mi_rb_target(C.byref(r2), C.byref(b), None), grad=lambda b: L.mi_rb_grad(C.byref(r2), C.byref(b), None),
             update=lambda b: L.mi_rb_update(C.byref(r2), C.byref(b), C.byref(o), None))
inf, nan = float("inf"), float("nan")
for who, call in calls.items():
    out["n_step_0:" + who] = call(batch(n_step=0))
    out["n_step_17:" + who] = call(batch(n_step=17))
    out["n_step_slots:" + who] = call(batch(n_step=4))
    out["n_step_-1:" + who] = call(batch(n_step=-1))
    out["head_-1:" + who] = call(batch(head_slot=-1))
    out["head_slots:" + who] = call(batch(head_slot=4))
    out["null:horizon:" + who] = call(batch(horizon=None))
    out["text:horizon:" + who] = L.mi_rb_last_error().decode()
    out["support_equal:" + who] = call(batch(v_min=1.0, v_max=1.0))
    out["support_reversed:" + who] = call(batch(v_min=2.0, v_max=1.0))
    out["support_inf:" + who] = call(batch(v_max=inf))
    out["support_-inf:" + who] = call(batch(v_min=-inf))
    out["support_nan:" + who] = call(batch(v_min=nan))
    out["support_span_inf:" + who] = call(batch(v_min=-3e38, v_max=3e38))
    out["text:support:" + who] = L.mi_rb_last_error().decode()
    out["null:target_probs:" + who] = call(batch(target_probs=None))
out["null:prio"] = calls["grad"](batch(prio=None))
out["text:prio"] = L.mi_rb_last_error().decode()
out["zero:batch"] = calls["grad"](batch(batch=0))
out["misaligned:params"] = calls["grad"](batch(params=20))
out["misaligned:params:target"] = calls["target"](batch(params=20))
out["misaligned:workspace"] = calls["grad"](batch(workspace=24))
out["range:sample_upper"] = calls["grad"](batch(sample_upper=5))
out["null:opt"] = L.mi_rb_update(C.byref(r2), C.byref(batch()), None, None)
out["empty:opt"] = calls["update"](batch())
# forward and noise: NULL, misaligned, a stream tag that does not fit 4 bits, a bad support
key = K.RBKey(1, 2, 3, 16, 0)
out["forward:stream_16"] = L.mi_rb_forward(16, 16, 1, C.byref(key), 0.0, 100.0, 16, 16, None)
out["text:forward"] = L.mi_rb_last_error().decode()
out["forward:misaligned"] = L.mi_rb_forward(20, 16, 1, None, 0.0, 100.0, 16, 16, None)
out["forward:n_0"] = L.mi_rb_forward(16, 16, 0, None, 0.0, 100.0, 16, 16, None)
out["forward:null_both"] = L.mi_rb_forward(16, 16, 1, None, 0.0, 100.0, None, None, None)
out["forward:support_equal"] = L.mi_rb_forward(16, 16, 1, None, 5.0, 5.0, 16, 16, None)
out["forward:support_nan"] = L.mi_rb_forward(16, 16, 1, None, 0.0, nan, 16, 16, None)
out["noise:stream_16"] = L.mi_rb_noise(1, 2, 3, 16, 16, 16, 16, None)
out["text:noise"] = L.mi_rb_last_error().decode()
out["noise:null_fout"] = L.mi_rb_noise(1, 2, 3, 14, 16, 16, None, None)
out["noise:null_fin"] = L.mi_rb_noise(1, 2, 3, 14, 16, None, 16, None)
out["noise:null_xi"] = L.mi_rb_noise(1, 2, 3, 14, None, 16, 16, None)
# acting: a handle that is there, a bad support
a1 = K.RBAct(16, 16, None, None, None, None, 0, 100, 0, 0.0, 0.0, 0.5, 1, 0, 1, 3.0, 3.0, 0)
out["act:support_equal"] = L.mi_rb_act_steps(16, C.byref(r2), C.byref(a1), None)
out["text:act_support"] = L.mi_rb_last_error().decode()
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_rb_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_rb_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_zero_and_out_of_range_arguments(K):
    import json

    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    text, text_prio = res.pop("text"), res.pop("text:prio")
    assert res.pop("n_step_17:slots_64") == [-1, -1]
    assert "invalid argument" in text and "a batch buffer is NULL" in text_prio
    assert res.pop("text:act").startswith("mi_rb_act_steps:") and res.pop("text:forward").startswith("mi_rb_forward:") and res.pop("text:noise").startswith("mi_rb_noise:")
    assert "finite v_min < v_max" in res.pop("text:act_support")
    for who in ("target", "grad", "update"):
        t = res.pop("text:horizon:" + who)
        assert "horizon is NULL" in t and t.startswith("mi_rb_target" if who == "target" else "rb_grad"), t      # the entry point (or its one shared body) is named
        assert "finite v_min < v_max" in res.pop("text:support:" + who)
    assert set(k for k in res if ":" not in k) == set(K.SIGNATURES)
    assert sum(k.startswith(("n_step_", "head_", "null:horizon", "support_", "null:target_probs")) for k in res) == 3 * 14
    harmless = {"mi_rb_version", "mi_rb_last_error", "mi_rb_source_id", "mi_rb_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_RB_EINVAL


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_RB_SO"] = os.path.join(%r, "no_such_libmirl_rainbow.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_nz, _native_rb
assert _native.lib().mi_version() == _native.ABI_VERSION and _native_nz.lib().mi_nz_version() == 1
assert deep_rl_amd.RainbowEngine is not None and {"RainbowEngine", "RainbowQNetwork"} <= set(deep_rl_amd.__all__)
try:
    _native_rb.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_tenth_library(K):
    """libmirl_rainbow.so loads lazily: with it absent `import deep_rl_amd` and the older libraries work, and the first use of the engine's path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_tenth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved symbol of another library would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_rb_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_per_sample_current", "mi_dueling_pack", "mi_pg_version", "mi_c51_version", "mi_c51_forward",
                  "mi_iqn_version", "mi_qr_version", "mi_ddqn_version", "mi_pdd_version", "mi_pdd_forward", "mi_ns_version", "mi_ns_grad", "mi_nz_version", "mi_nz_noise"):
        assert not hasattr(L, other), other


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]
KERNELS = ("rb_noise_kernel", "rb_forward_kernel", "rb_target_kernel", "rb_grad_kernel", "rb_reduce_kernel",
           "rb_act_kernelILb0ELb0", "rb_act_kernelILb0ELb1", "rb_act_kernelILb1ELb0", "rb_act_kernelILb1ELb1")   # acting: <teacher-forced, noisy>


def test_device_only_build_compiles_without_scratch():
    """every kernel of the library: no scratch, no spilled vector register (the figures DESIGN §22 quotes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_rainbow.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == len(KERNELS) and all(any(k in n for n in names) for k in KERNELS), names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * len(KERNELS)
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * len(KERNELS)
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)) <= 256


def test_the_other_libraries_are_still_what_their_sources_give(K):
    """the feature changes no token of the nine older libraries or of the shared headers: their source ids are what their own sources give and what the committed
    profiles recorded, and the new library has an id of its own that csrc/srcid.py reproduces"""
    import json

    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C5
    from deep_rl_amd import _native_ddqn as DQ
    from deep_rl_amd import _native_iqn as IQ
    from deep_rl_amd import _native_ns as NS
    from deep_rl_amd import _native_nz as NZ
    from deep_rl_amd import _native_pdd as PD
    from deep_rl_amd import _native_pg as PG
    from deep_rl_amd import _native_qr as QR

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    mk = open(os.path.join(CSRC, "Makefile")).read()
    allsrc = lambda var: re.search(r"^%s = (.*)$" % var, mk, flags=re.M).group(1).split()   # noqa: E731
    older = (("ALLSRC", N.lib().mi_source_id().decode()), ("PG_ALLSRC", PG.source_id()), ("C51_ALLSRC", C5.source_id()), ("IQN_ALLSRC", IQ.source_id()),
             ("QR_ALLSRC", QR.source_id()), ("DDQN_ALLSRC", DQ.source_id()), ("PDD_ALLSRC", PD.source_id()), ("NS_ALLSRC", NS.source_id()), ("NZ_ALLSRC", NZ.source_id()))
    srcs = S.SRCS
    for var, sid in older:
        files = allsrc(var)
        assert "mi_rainbow.hip" not in files and "../../include/mi_rainbow.h" not in files
        assert srcid(srcs + files[1:] if var == "ALLSRC" else files) == sid, var
    prof = lambda name: json.load(open(os.path.join(ROOT, "profiles", name)))   # noqa: E731
    assert prof("latest_pmc.json").get("source_id") == older[0][1] and prof("ddqn_bench.json")["ddqn_source_id"] == DQ.source_id()
    assert prof("pdd_bench.json")["pdd_source_id"] == PD.source_id() and prof("nstep_bench.json")["nstep_source_id"] == NS.source_id()
    assert prof("noisy_bench.json")["noisy_source_id"] == NZ.source_id()
    assert allsrc("RB_ALLSRC") == RB_ALLSRC and srcid(RB_ALLSRC) == K.source_id()
    for name in ("rainbow_bench.json", "rainbow_gpu_maxima.json", "rainbow_learning.json"):
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            assert json.load(open(path))["rainbow_source_id"] == K.source_id(), name
    assert len({sid for _, sid in older} | {K.source_id()}) == 10
    assert "$(OUT_RB)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_RB)" in mk.split("clean:")[1]
    assert "-DMI_RB_SOURCE_ID" in mk and "OUT_RB ?= ../libmirl_rainbow.so" in mk
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_native_rb.lib().mi_rb_version() == _native_rb.ABI_VERSION" in entry


def test_engine_and_network_surface():
    """NoisyDQNEngine's surface plus the support: the sampler, the priority bookkeeping, beta() and sync_target are inherited, everything that meets the network
    goes through the new library; the network's flat vector is all mu, then all sigma, at the header's offsets"""
    import inspect

    import numpy as np
    import torch

    from deep_rl_amd import NoisyDQNEngine, NoisyLinear, PDDDQNEngine, RainbowEngine, RainbowQNetwork, _native_rb, checkpoint

    assert issubclass(RainbowEngine, NoisyDQNEngine) and RainbowEngine.K is _native_rb
    for name in ("sample", "beta", "refresh_sums", "_scatter", "grad", "reset", "drain_episodes", "sync_target"):
        assert getattr(RainbowEngine, name) is getattr(PDDDQNEngine, name), name
    for name in ("act", "forward", "_batch", "target", "train_step", "__init__"):
        assert name in vars(RainbowEngine) and inspect.isfunction(vars(RainbowEngine)[name]), name
    sig = inspect.signature(RainbowEngine.__init__)
    assert list(sig.parameters)[1:] == list(inspect.signature(NoisyDQNEngine.__init__).parameters)[1:] + ["n_atoms", "v_min", "v_max"]
    assert (sig.parameters["n_atoms"].default, sig.parameters["v_min"].default, sig.parameters["v_max"].default, sig.parameters["n_step"].default) == (51, 0.0, 100.0, 3)
    src = inspect.getsource(sys.modules[RainbowEngine.__module__])
    assert "mi_pdd_" not in src and "mi_ns_" not in src and "mi_nz_" not in src.replace("mi_nz_update", "") and "mi_rb_act_steps" in src and "mi_rb_forward" in src
    assert inspect.getsource(checkpoint).index("RainbowEngine, NoisyDQNEngine") > 0                      # named ahead of its bases

    class Env:
        class observation_space:
            shape = (4,)

        class action_space:
            n = 2

    torch.manual_seed(3)
    net = RainbowQNetwork(Env, device="cpu")
    v, a = net.value_stream, net.advantage_stream
    assert isinstance(v, NoisyLinear) and isinstance(a, NoisyLinear) and net.flat.numel() == 36774 and net.flat.dtype == torch.float32
    f = net.flat.numpy()
    b = 1 / np.sqrt(84)
    assert np.abs(f[10764:23769]).max() <= b and np.abs(f[10764:23769]).max() > 0.8 * b and np.allclose(f[23769:], 0.5 / np.sqrt(84), rtol=1e-6, atol=0)
    # views, in the header's order: Wv bv Wa ba, then their sigmas
    for off, p in ((10764, v.weight_mu), (15048, v.bias_mu), (15099, a.weight_mu), (23667, a.bias_mu),
                   (23769, v.weight_sigma), (23769 + 4284, v.bias_sigma), (23769 + 4335, a.weight_sigma), (23769 + 12903, a.bias_sigma)):
        assert p.data_ptr() == net.flat.data_ptr() + 4 * off and np.array_equal(p.detach().numpy().reshape(-1), f[off:off + p.numel()]), off
    assert v.weight_mu.shape == (51, 84) and a.weight_mu.shape == (102, 84)
    assert sum(p.numel() for p in net.parameters()) == 36774 and len(list(net.parameters())) == 12
    x = torch.randn(5, 4)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _rainbow_ref as Z
    probs, q = Z.forward(f, x.numpy(), (0.0, 100.0))
    assert np.abs(net(x).detach().numpy() - q).max() < 1e-4 and np.abs(net.get_probs(x).detach().numpy() - probs).max() < 1e-6     # forward is the mean network's q
    with pytest.raises(Exception):
        RainbowQNetwork(Env, device="cpu", n_atoms=101)
