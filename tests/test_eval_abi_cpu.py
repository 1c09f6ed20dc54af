"""CPU-only checks of the eleventh library's boundary: libmirl_eval.so loads without a GPU, exports and binds every symbol include/mi_eval.h declares, reports
errors through return codes before any HIP call, compiles without scratch or spills — and leaves the ten older libraries what they were."""
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
EV_ALLSRC = S.ALLSRC["_native_ev"]
# the ten older libraries: (binding module, the Makefile's source list, the id this feature found and must leave)
OLDER = (
    ("_native_pg", S.ALLSRC["_native_pg"], "c30878346b6f"),
    ("_native_c51", S.ALLSRC["_native_c51"], "976edde66621"),
    ("_native_iqn", S.ALLSRC["_native_iqn"], "e35a43ebf95c"),
    ("_native_qr", S.ALLSRC["_native_qr"], "8100cd09ac96"),
    ("_native_ddqn", S.ALLSRC["_native_ddqn"], "08f332993a59"),
    ("_native_pdd", S.ALLSRC["_native_pdd"], "65d24581dff3"),
    ("_native_ns", S.ALLSRC["_native_ns"], "ffb74331a9c8"),
    ("_native_nz", S.ALLSRC["_native_nz"], "74e65f9c5f40"),
    ("_native_rb", S.ALLSRC["_native_rb"], "47a9b95b193c"),
)
LIBMIRL_ID = "6106efad96ba"


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_ev

    if not all(os.path.exists(p) for p in (_native_ev.SO_PATH, _native.SO_PATH)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_ev


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_eval.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_ev_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_ev_" + n for n in ("version", "last_error", "source_id", "forward", "episodes")}
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_eval.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_ev_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_EV_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MI_EV_MAX_STEPS", K.MAX_STEPS), ("MI_EV_DEFAULT_WORKGROUPS", K.DEFAULT_WORKGROUPS),
                         ("MI_EV_NPARAMS_DUELING", K.NPARAMS[K.DUELING]), ("MI_EV_NPARAMS_QR", K.NPARAMS[K.QR]), ("MI_EV_NPARAMS_C51", K.NPARAMS[K.C51]),
                         ("MI_EV_NPARAMS_RAINBOW", K.NPARAMS[K.RAINBOW]), ("MI_EV_C51_ATOMS", K.C51_ATOMS), ("MI_EV_RAINBOW_ATOMS", K.RAINBOW_ATOMS),
                         ("MI_EV_QR_QUANT", K.QR_QUANT)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro
    kinds = re.search(r"enum \{ (MI_EV_DUELING.*?) \};", hdr).group(1)
    assert [s.strip() for s in kinds.split(",")] == ["MI_EV_%s = %d" % (n, i) for i, n in sorted(K.KIND_NAMES.items())]
    assert (K.DUELING, K.QR, K.C51, K.RAINBOW) == (1, 2, 3, 4) and not hasattr(K, "PLAIN") and "MI_EV_PLAIN" not in hdr   # 0 is free: the plain QNetwork has no kind
    # mi_ev_forward(params, kind, v_min, v_max, obs, n, q, stream)
    proto = re.search(r"int mi_ev_forward\((.*?)\);", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["params", "kind", "v_min", "v_max", "obs", "n", "q", "stream"]
    body = re.search(r"typedef struct mi_ev_args_t \{(.*?)\}", hdr, flags=re.S).group(1)
    assert re.findall(r"([a-z_0-9]+)\s*;", body) == [f[0] for f in K.EVArgs._fields_]
    assert C.sizeof(K.EVArgs) == 8 * 8 + 2 * 8 + 6 * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"
    full = open(os.path.join(ROOT, "include", "mi_eval.h")).read()
    for owner in ("mi_ddqn.h", "mi_pdd.h", "mi_qr.h", "mi_c51.h", "mi_rainbow.h", "mi_noisy.h"):
        assert owner in full, "the header points to %s" % owner
    assert "IQN is out of scope" in full and "Numerics contract" in full


def test_the_library_needs_no_symbol_of_the_others_and_exports_none(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved symbol of another library would fail the load (RTLD_NOW makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_ev_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_pg_version", "mi_c51_version", "mi_iqn_version", "mi_qr_version", "mi_ddqn_version",
                  "mi_pdd_version", "mi_ns_version", "mi_nz_version", "mi_rb_version", "mi_ddqn_forward", "mi_rb_forward"):
        assert not hasattr(L, other), other
    import shutil
    nm = subprocess.run(["nm", "-D", "--defined-only", K.SO_PATH], capture_output=True, text=True) if shutil.which("nm") else None
    if nm is not None and nm.returncode == 0:
        mine = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and ln.split()[-1].startswith("mi_")}
        assert mine == set(K.SIGNATURES), mine ^ set(K.SIGNATURES)


_ARG_PROBE = r"""
import ctypes as C, json, math, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_ev as K
L, out, text = K.lib(), {}, {}
A = 1 << 20   # an address-shaped number, 16-byte aligned: every call below must fail BEFORE anything could read it
def args(**kw):
    a = K.EVArgs(A, A, A, A, A, A, None, None, 1, 1 << 40, K.DUELING, 1, 0, -100.0, 100.0, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a
def ep(name, **kw):
    out[name] = L.mi_ev_episodes(C.byref(args(**kw)), None)
    text[name] = L.mi_ev_last_error().decode()
def fw(name, params=A, kind=K.DUELING, lo=-100.0, hi=100.0, obs=A, n=1, q=A):
    out[name] = L.mi_ev_forward(params, kind, lo, hi, obs, n, q, None)
    text[name] = L.mi_ev_last_error().decode()
out["episodes:NULL"] = L.mi_ev_episodes(None, None); text["episodes:NULL"] = L.mi_ev_last_error().decode()
ep("episodes:empty", params=None, lengths=None, n_episodes=0)
ep("episodes:params NULL", params=None)
ep("episodes:lengths NULL", lengths=None)
ep("episodes:params misaligned", params=A + 4)
ep("episodes:kind -1", kind=-1)
ep("episodes:kind 0", kind=0)
ep("episodes:kind 5", kind=5)
ep("episodes:E 0", n_episodes=0)
ep("episodes:E -3", n_episodes=-3)
ep("episodes:max_workgroups -1", max_workgroups=-1)
ep("episodes:forced_starts misaligned", forced_starts=A + 4)
ep("episodes:returns misaligned", returns=A + 2)
for kind in (K.C51, K.RAINBOW):
    for label, lo, hi in (("equal", 1.0, 1.0), ("reversed", 2.0, 1.0), ("inf", 0.0, math.inf), ("-inf", -math.inf, 0.0), ("nan", math.nan, 1.0), ("nan hi", 0.0, math.nan),
                          ("infinite span", -3e38, 3e38)):
        ep("episodes:%%s support %%s" %% (K.KIND_NAMES[kind], label), kind=kind, v_min=lo, v_max=hi)
        fw("forward:%%s support %%s" %% (K.KIND_NAMES[kind], label), kind=kind, lo=lo, hi=hi)
fw("forward:params NULL", params=None)
fw("forward:obs NULL", obs=None)
fw("forward:q NULL", q=None)
fw("forward:n 0", n=0)
fw("forward:n -1", n=-1)
fw("forward:kind -1", kind=-1)
fw("forward:kind 0", kind=0)
fw("forward:kind 5", kind=5)
fw("forward:params misaligned", params=A + 4)
fw("forward:obs misaligned", obs=A + 8)
print("RESULT", json.dumps(dict(out=out, text=text)))
"""


def test_every_bad_argument_is_an_error_before_any_hip_call(K):
    """NULL, zero, misaligned and out-of-range arguments: -1 and a message.  The pointers handed in are numbers no call may dereference; the process has no GPU to
    launch on, so any call that got past its checks would report MI_EV_EHIP (-2) instead"""
    p = subprocess.run([sys.executable, "-c", _ARG_PROBE % ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-800:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    assert len(res["out"]) == 13 + 2 * 2 * 7 + 10
    for name, rc in res["out"].items():
        assert rc == -1, (name, rc)   # MI_EV_EINVAL
        assert "invalid argument" in res["text"][name] and res["text"][name].startswith("mi_ev_" + name.split(":")[0]), (name, res["text"][name])
    assert "support" in res["text"]["episodes:C51 support nan"] and "kind" in res["text"]["episodes:kind 5"] and "kind" in res["text"]["episodes:kind 0"] and "n_episodes" in res["text"]["episodes:E 0"]
    assert "max_workgroups" in res["text"]["episodes:max_workgroups -1"] and "lengths" in res["text"]["episodes:lengths NULL"]


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_EVAL_SO"] = os.path.join(%r, "no_such_libmirl_eval.so")
import deep_rl_amd
assert "deep_rl_amd.evaluate" not in sys.modules and "deep_rl_amd._native_ev" not in sys.modules   # lazily, as the other optional paths
from deep_rl_amd import _native, _native_ev
assert _native.lib().mi_version() == _native.ABI_VERSION
assert "evaluate" in deep_rl_amd.__all__ and "EvalResult" in deep_rl_amd.__all__
assert callable(deep_rl_amd.evaluate) and deep_rl_amd.EvalResult is deep_rl_amd.evaluate.EvalResult
from deep_rl_amd.evaluate import evaluate, ENGINES_EVALUABLE
assert "IQNEngine" not in ENGINES_EVALUABLE and "DoubleDQNEngine" not in ENGINES_EVALUABLE and len(ENGINES_EVALUABLE) == 7
try:
    _native_ev.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_eleventh_library(K):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_unsupported_policies_raise_and_name_what_is_supported(K):
    import deep_rl_amd as D
    from deep_rl_amd import evaluate as EV

    class IQNEngine:   # what evaluate() sees of an IQN engine: `q` is no network of a supported class
        def __init__(self):
            self.q = D.FeaturesExtractor(type("E", (), {"observation_space": type("S", (), {"shape": (4,)}), "action_space": type("A", (), {"n": 2})})(), device="cpu")

    class DoubleDQNEngine:   # the plain QNetwork has no kind (its two owning forwards disagree): an error that says so, not a guess
        def __init__(self):
            self.q = D.QNetwork(E._Spec(), device="cpu")

    import _eval_ref as E
    with pytest.raises(K.MiError) as e:
        D.evaluate(DoubleDQNEngine(), 3)
    assert "plain QNetwork" in str(e.value) and "different bits" in str(e.value)
    for policy in (IQNEngine(), DoubleDQNEngine(), object(), None, D.CosineEmbeddingNetwork(64, 64, device="cpu")):
        with pytest.raises(K.MiError) as e:
            D.evaluate(policy, 3)
        for name in ("DuelingQNetwork", "QRQNetwork", "C51QNetwork", "RainbowQNetwork", "no torch fallback"):
            assert name in str(e.value), name
    assert inspect_signature(EV.evaluate) == ["policy", "episodes", "seed", "env_id_base", "forced_actions", "forced_starts", "trace", "max_workgroups", "stream"]
    import inspect
    sig = inspect.signature(EV.evaluate)
    assert (sig.parameters["episodes"].default, sig.parameters["seed"].default, sig.parameters["env_id_base"].default) == (100, 1, 1 << 40)
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("forced_actions", "forced_starts", "trace", "max_workgroups", "stream"))
    # a supported class on the CPU is an error too (the parameters must be on the device), never a torch evaluation
    with pytest.raises(K.MiError):
        D.evaluate(E.network_class("qr")(E._Spec(), device="cpu"), 3)
    for engine, net in EV.ENGINES_EVALUABLE.items():
        assert hasattr(D, engine) and hasattr(D, net), (engine, net)


def inspect_signature(fn):
    import inspect
    return list(inspect.signature(fn).parameters)


def test_parameter_counts_are_the_network_classes(K):
    """the floats a kind reads == flat.numel() of its class, the sigmas excluded"""
    import _eval_ref as E
    from deep_rl_amd import _native_nz, _native_rb

    n = {kind: E.network_class(kind)(E._Spec(), device="cpu").flat.numel() for kind in E.KINDS}
    assert n["qr"] == K.NPARAMS[K.QR] == 21644
    assert n["c51"] == K.NPARAMS[K.C51] == 27934
    assert n["dueling"] == _native_nz.NPARAMS == 11274 and n["dueling"] - 255 == K.NPARAMS[K.DUELING] == 11019      # NoisyDuelingQNetwork: 255 sigmas behind the means
    assert n["rainbow"] == _native_rb.NPARAMS == 36774 and n["rainbow"] - 13005 == K.NPARAMS[K.RAINBOW] == 23769    # 13,005 sigmas behind the means
    from deep_rl_amd import _native as N
    assert N.DUELING_NPARAMS == K.NPARAMS[K.DUELING]   # DuelingQNetwork's flat
    assert E.NREAD == {kind: K.NPARAMS[E.KIND_ID[kind]] for kind in E.KINDS}


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_every_kernel_has_no_scratch_and_no_vgpr_spill():
    """from the compiler's resource remarks: 4 forward kernels and 4 x 2 episode kernels (one instantiation per kind, forced and unforced apart)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_eval.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        seen[name] = dict(scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), spill=int(re.search(r"VGPRs Spill: (\d+)", b).group(1)),
                          lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    fwd = [n for n in seen if "ev_forward_kernel" in n]
    epi = [n for n in seen if "ev_episode_kernel" in n]
    assert len(fwd) == 4 and len(epi) == 8 and len(seen) == 12, sorted(seen)
    for name, r in seen.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["lds"] <= 8192, (name, r)


def test_eleven_distinct_source_ids_and_the_ten_older_ones_unchanged(K):
    import importlib

    from deep_rl_amd import _native as N

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    ids = [N.lib().mi_source_id().decode()]
    assert ids[0] == LIBMIRL_ID == json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json"))).get("source_id")
    for mod, files, pinned in OLDER:
        M = importlib.import_module("deep_rl_amd." + mod)
        assert M.source_id() == pinned == srcid(files), (mod, M.source_id(), srcid(files))
        ids.append(pinned)
    assert srcid(EV_ALLSRC) == K.source_id()
    ids.append(K.source_id())
    assert len(ids) == 11 == len(set(ids))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "EV_ALLSRC = " + " ".join(EV_ALLSRC) in mk and "$(OUT_EV)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_EV)" in mk.split("clean:")[1]
    assert "-DMI_EV_SOURCE_ID" in mk and "OUT_EV ?= ../libmirl_eval.so" in mk
    for rec in ("eval_bench.json", "eval_gpu_results.json"):
        path = os.path.join(ROOT, "profiles", rec)
        if os.path.exists(path):
            assert json.load(open(path))["eval_source_id"] == K.source_id(), rec
