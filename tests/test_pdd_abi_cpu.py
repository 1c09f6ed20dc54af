"""CPU-only checks of the seventh library's boundary: libmirl_pdd.so loads without a GPU, exports and binds every symbol include/mi_pdd.h declares, reports errors
through return codes — and leaves the six older libraries what their own sources give."""
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
PDD_ALLSRC = S.ALLSRC["_native_pdd"]


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_ddqn, _native_iqn, _native_pdd, _native_pg, _native_qr

    if not all(os.path.exists(m.SO_PATH) for m in (_native_pdd, _native_ddqn, _native_qr, _native_c51, _native_iqn, _native_pg, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_pdd


def _header(name="mi_pdd.h"):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_pdd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_pdd_" + n for n in ("version", "last_error", "source_id", "workspace_bytes", "forward", "act_steps", "target", "grad", "update")}
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_pdd.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_pdd_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_PDD_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MI_PDD_NPARAMS", K.NPARAMS), ("MI_PDD_H1", K.H1), ("MI_PDD_H2", K.H2), ("MI_PDD_W1", K.OFF_W1), ("MI_PDD_B1", K.OFF_B1),
                         ("MI_PDD_W2", K.OFF_W2), ("MI_PDD_B2", K.OFF_B2), ("MI_PDD_WV", K.OFF_WV), ("MI_PDD_BV", K.OFF_BV), ("MI_PDD_WA", K.OFF_WA),
                         ("MI_PDD_BA", K.OFF_BA), ("MI_PDD_MAX_SLABS", K.MAX_SLABS), ("MI_PDD_SLAB_STRIDE", K.SLAB_STRIDE),
                         ("MI_PDD_MAX_STEPS_PER_CALL", K.MAX_STEPS_PER_CALL)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro
    from deep_rl_amd import _native as N
    # the QNetwork of dueling_dqn.py in the flat order DuelingQNetwork.flat has: torso, Wv[84] bv, Wa[2][84] ba[2]
    assert K.NPARAMS == 11_019 == N.DUELING_NPARAMS == K.OFF_BA + 2 and K.OFF_WV == K.OFF_B2 + K.H2 == 10_764 and K.OFF_BV == K.OFF_WV + K.H2 == 10_848
    assert K.OFF_WA == K.OFF_BV + 1 == 10_849 and K.OFF_BA == K.OFF_WA + 2 * K.H2 == 11_017 and K.OFF_W2 + K.H1 * K.H2 == K.OFF_B2
    assert K.NPARAMS - K.OFF_WV == 255                       # one head gradient element per thread of the 256-thread workgroup
    assert K.SLAB_STRIDE % 4 == 0 and K.SLAB_STRIDE > K.NPARAMS and K.OFF_W2 % 4 == 0
    assert hasattr(K, "Ring") and hasattr(K, "Batch") and hasattr(K, "AdamArgs") and callable(K.workspace_bytes) and callable(K.grad) and callable(K.update)
    src = open(os.path.join(CSRC, "mi_pdd.hip")).read()
    dueling = open(os.path.join(CSRC, "mi_dueling.h")).read()
    assert "static_assert(MI_PDD_W1 == TS_W1 && MI_PDD_B1 == TS_B1 && MI_PDD_W2 == TS_W2 && MI_PDD_B2 == TS_B2" in src
    for text in (src, dueling):
        assert "asm" not in text and "atomicAdd(" not in text
    assert '#include "mi_dueling.h"' in src and "template <bool ROW, bool NEXT>" not in src      # the head and the batch row are the shared header's, not a copy


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2),", r"\1;", body))


def test_struct_layouts_match_header(K):
    hdr, dd = _header(), _header("mi_ddqn.h")
    assert _struct_fields(hdr, "mi_pdd_ring_t") == [f[0] for f in K.PDDRing._fields_] == _struct_fields(dd, "mi_ddqn_ring_t")
    assert _struct_fields(hdr, "mi_pdd_act_t") == [f[0] for f in K.PDDAct._fields_] == _struct_fields(dd, "mi_ddqn_act_t") and "learning_starts" in _struct_fields(hdr, "mi_pdd_act_t")
    assert _struct_fields(hdr, "mi_pdd_batch_t") == [f[0] for f in K.PDDBatch._fields_] == _struct_fields(dd, "mi_ddqn_batch_t") + ["weights", "td_abs"]
    assert _struct_fields(hdr, "mi_pdd_adam_t") == [f[0] for f in K.PDDAdam._fields_] == _struct_fields(dd, "mi_ddqn_adam_t")
    from deep_rl_amd import _native_ddqn as DQ
    for mine, theirs in ((K.PDDRing, DQ.DDQNRing), (K.PDDAct, DQ.DDQNAct), (K.PDDAdam, DQ.DDQNAdam)):    # layout-identical to Double DQN's
        assert C.sizeof(mine) == C.sizeof(theirs) and [(n, getattr(mine, n).offset) for n, _ in mine._fields_] == [(n, getattr(theirs, n).offset) for n, _ in theirs._fields_]
    assert all(getattr(K.PDDBatch, n).offset == getattr(DQ.DDQNBatch, n).offset for n, _ in DQ.DDQNBatch._fields_)
    assert C.sizeof(K.PDDRing) == 4 * 8 + 8 + 4 + 4
    assert C.sizeof(K.PDDAct) == 6 * 8 + 3 * 8 + 3 * 8 + 4 + 4
    assert C.sizeof(K.PDDBatch) == 9 * 8 + 3 * 8 + 4 + 4 + 8 + 2 * 8 and K.PDDBatch.weights.offset == 112 and K.PDDBatch.td_abs.offset == 120
    assert C.sizeof(K.PDDAdam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_pdd_workspace_bytes(0) == 0 and L.mi_pdd_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_pdd_workspace_bytes(128) == L.mi_pdd_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_pdd as K
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
r, b, a, o = K.PDDRing(), K.PDDBatch(), K.PDDAct(), K.PDDAdam()
out["empty:act"] = L.mi_pdd_act_steps(None, C.byref(r), C.byref(a), None)
fake = (C.c_char * 64)()
out["empty:act_handle"] = L.mi_pdd_act_steps(C.addressof(fake), C.byref(r), C.byref(a), None)
out["empty:target"] = L.mi_pdd_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_pdd_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_pdd_update(C.byref(r), C.byref(b), C.byref(o), None)
out["misaligned:forward"] = L.mi_pdd_forward(4, 4, 1, 4, None)
# a ring and a batch whose every pointer is set (never dereferenced on the host: the check comes first) but td_abs
r2 = K.PDDRing(16, 16, 16, 16, 4, 1, 0)
b2 = K.PDDBatch(*([16] * 9), 0, 0, 0, 1, 0.99, None, None, None)
out["null:td_abs"] = L.mi_pdd_grad(C.byref(r2), C.byref(b2), None)
out["text:td_abs"] = L.mi_pdd_last_error().decode()
b2.td_abs, b2.batch = 16, 0
out["zero:batch"] = L.mi_pdd_grad(C.byref(r2), C.byref(b2), None)
b2.batch, b2.params = 1, 20
out["misaligned:params"] = L.mi_pdd_grad(C.byref(r2), C.byref(b2), None)
b2.params, b2.sample_upper = 16, 5
out["range:sample_upper"] = L.mi_pdd_grad(C.byref(r2), C.byref(b2), None)
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_pdd_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_pdd_last_error().decode()
print("RESULT", json.dumps(out))
"""


def test_every_entry_point_survives_null_and_zero_arguments(K):
    p = subprocess.run([sys.executable, "-c", _NULL_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    done = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("DONE")]
    assert p.returncode == 0, "crashed after %s: %s" % (done[-1] if done else "nothing", p.stderr[-800:])
    res = json_result(p.stdout)
    text, text_td = res.pop("text"), res.pop("text:td_abs")
    assert "invalid argument" in text and "a batch buffer is NULL" in text_td
    assert set(k for k in res if ":" not in k) == set(K.SIGNATURES)
    harmless = {"mi_pdd_version", "mi_pdd_last_error", "mi_pdd_source_id", "mi_pdd_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == -1, (name, r)   # MI_PDD_EINVAL


def json_result(stdout):
    import json
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("RESULT")][0][7:])


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_PDD_SO"] = os.path.join(%r, "no_such_libmirl_pdd.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_pdd
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.PDDDQNEngine is not None and "PDDDQNEngine" in deep_rl_amd.__all__
try:
    _native_pdd.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_seventh_library(K):
    """libmirl_pdd.so loads lazily: with it absent `import deep_rl_amd` and libmirl.so work, and the first use of the engine's path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_seventh_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_per_* would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_pdd_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_per_sample_current", "mi_dueling_pack", "mi_pg_version", "mi_c51_version", "mi_iqn_version",
                  "mi_qr_version", "mi_ddqn_version"):
        assert not hasattr(L, other), other


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles_without_scratch():
    """every kernel of the library: no scratch, no spilled vector register (the figures DESIGN §19 quotes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_pdd.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 6 and all(any(k in n for n in names) for k in ("pdd_forward_kernel", "pdd_act_kernel", "pdd_target_kernel", "pdd_grad_kernel", "pdd_reduce_kernel"))
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * 6
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * 6
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)) <= 256


def test_the_other_libraries_are_still_what_their_sources_give(K):
    """the feature changes no token of the six older libraries or of the shared headers: their source ids are what their own sources give, and the new library has an
    id of its own that csrc/srcid.py reproduces"""
    import json

    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C5
    from deep_rl_amd import _native_ddqn as DQ
    from deep_rl_amd import _native_iqn as IQ
    from deep_rl_amd import _native_pg as PG
    from deep_rl_amd import _native_qr as QR

    mine = N.lib().mi_source_id().decode()
    assert json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json"))).get("source_id") == mine

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    assert srcid(S.ALLSRC["_native_ddqn"]) == DQ.source_id()
    assert json.load(open(os.path.join(ROOT, "profiles", "ddqn_bench.json")))["ddqn_source_id"] == DQ.source_id()      # mi_ring.h / mi_torso.h / mi_common.h did not move
    assert srcid(PDD_ALLSRC) == K.source_id()
    bench = os.path.join(ROOT, "profiles", "pdd_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["pdd_source_id"] == K.source_id()
    assert len({mine, PG.source_id(), C5.source_id(), IQ.source_id(), QR.source_id(), DQ.source_id(), K.source_id()}) == 7
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "PDD_ALLSRC = " + " ".join(PDD_ALLSRC) in mk and "$(OUT_PDD)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_PDD)" in mk.split("clean:")[1]
    assert "-DMI_PDD_SOURCE_ID" in mk and "OUT_PDD ?= ../libmirl_pdd.so" in mk


def test_engine_surface_is_callable_where_it_must_be():
    """the surface of DoubleDQNEngine plus the prioritized arguments: methods are methods on the class (an instance attribute of the same name would shadow them); a
    world size > 1 is a loud error"""
    import inspect

    from deep_rl_amd import PDDDQNEngine, checkpoint
    from deep_rl_amd._ring_engine import RingEngine

    assert issubclass(PDDDQNEngine, RingEngine)
    names = ("reset", "act", "drain_episodes", "sample", "target", "grad", "train_step", "sync_target", "forward", "refresh_sums", "beta")
    for name in names:
        assert inspect.isfunction(getattr(PDDDQNEngine, name)), name
    src = "".join(inspect.getsource(c.__init__) for c in PDDDQNEngine.__mro__ if "__init__" in vars(c) and c is not object)   # the base class allocates the ring
    for name in names:
        assert "self.%s =" % name not in src and "self.%s," % name not in src, name
    for name in ("observations", "actions", "rewards", "terminated", "batch_inds", "grads", "loss", "current", "target_values", "next_actions", "episode_stats", "td_abs",
                 "priorities", "max_priority", "weights", "_owner", "_per_ws"):
        assert "self.%s = " % name in src, name
    assert "world_size(process_group) > 1" in src and "raise K.MiError" in src
    sig = inspect.signature(PDDDQNEngine.__init__)
    assert list(sig.parameters)[1:] == ["env", "q_network", "target_network", "optimizer", "slots", "batch_size", "gamma", "learning_starts", "start_e", "end_e",
                                        "exploration_fraction", "total_timesteps", "max_episodes_logged", "process_group", "prioritized", "alpha", "beta_0"]
    assert (sig.parameters["batch_size"].default, sig.parameters["gamma"].default, sig.parameters["learning_starts"].default,
            sig.parameters["total_timesteps"].default) == (128, 0.99, 10_000, 100_000)
    assert (sig.parameters["prioritized"].default, sig.parameters["alpha"].default, sig.parameters["beta_0"].default) == (True, 0.6, 0.4)
    assert inspect.getsource(checkpoint).count("PDDDQNEngine") >= 5 and "refresh_sums" in inspect.getsource(checkpoint)
    eng_src = inspect.getsource(sys.modules[PDDDQNEngine.__module__])
    for call in ("mi_per_mark_sums", "mi_per_sample_current", "mi_per_update_priorities_sums", "mi_per_sums_refresh", "mi_pdd_act_steps", "mi_pdd_target", "mi_pdd_forward"):
        assert call in eng_src, call
    assert ".eff" not in eng_src.replace("``.eff``", "") and "repack()" not in eng_src.replace("``repack()``", "")
