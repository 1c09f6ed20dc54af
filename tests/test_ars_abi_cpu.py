"""CPU-only checks of the thirteenth library's boundary: libmirl_ars.so loads without a GPU, exports and binds every symbol include/mi_ars.h declares, lays its
struct out as the header does, refuses every invalid call before any HIP call, keeps every kernel out of scratch — and leaves the twelve older libraries what their
own sources give."""
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
ARS_ALLSRC = ["mi_ars.hip", "mi_common.h", S.INC + "mi_ars.h", S.INC + "mi_rl.h"]
# the ids of the twelve older libraries as their own sources gave them before this library existed (binding module -> 12 hex digits)
OLDER_IDS = {
    "_native_pg": "c30878346b6f", "_native_c51": "976edde66621", "_native_iqn": "e35a43ebf95c", "_native_qr": "8100cd09ac96", "_native_ddqn": "08f332993a59",
    "_native_pdd": "65d24581dff3", "_native_ns": "ffb74331a9c8", "_native_nz": "74e65f9c5f40", "_native_rb": "47a9b95b193c", "_native_md": "f25847e70b92",
}


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_ars

    if not all(os.path.exists(m.SO_PATH) for m in (_native_ars, _native)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_ars


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_ars.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_ars_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"mi_ars_" + n for n in ("version", "last_error", "source_id", "episodes", "update", "iterate")}
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_ars.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_ars_version() == K.ABI_VERSION == 1 == int(re.search(r"#define MI_ARS_VERSION (\d+)", hdr).group(1))
    for macro, value in (("MAX_STEPS", K.MAX_STEPS), ("MAX_DIRECTIONS", K.MAX_DIRECTIONS), ("DEFAULT_WORKGROUPS", K.DEFAULT_WORKGROUPS), ("NPARAMS", K.NPARAMS),
                         ("NSTATS", K.NSTATS), ("STREAM", K.STREAM)):
        assert int(re.search(r"#define MI_ARS_%s (\d+)" % macro, hdr).group(1)) == value, macro
    assert (K.MAX_STEPS, K.MAX_DIRECTIONS, K.STREAM) == (500, 4096, 15)
    assert "MIRL_ARS_SO" in open(os.path.join(ROOT, "deep_rl_amd", "_native_ars.py")).read()
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


def test_struct_layout_matches_the_header(K):
    body = re.search(r"typedef struct mi_ars_args_t \{(.*?)\}", _header(), flags=re.S).group(1)
    fields = re.findall(r"([a-z_0-9]+)\s*;", body)
    assert fields == [f[0] for f in K.ARSArgs._fields_]
    ctype = {"float*": C.c_void_p, "double*": C.c_void_p, "int64_t*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p, "uint64_t": C.c_uint64,
             "int32_t": C.c_int32, "float": C.c_float}
    types = [re.sub(r"\s+", "", t) for t in re.findall(r"([a-z_0-9]+\s*\*?)\s*[a-z_0-9]+\s*;", body)]
    assert [ctype[t] for t in types] == [f[1] for f in K.ARSArgs._fields_]
    assert C.sizeof(K.ARSArgs) == 10 * 8 + 2 * 8 + 8 * 4 and K.ARSArgs.seed.offset == 80 and K.ARSArgs.n_directions.offset == 96 and K.ARSArgs.noise.offset == 120


_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_ars as K
L, out = K.lib(), {}
inf, nan = float("inf"), float("nan")
# every pointer is set (never dereferenced on the host: every check comes before the launch) but the one under test
def args(**kw):
    a = K.ARSArgs(*([4096] * 10), 1, 0, 8, 4, 0, 0, 1, 0.02, 0.03, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a
calls = dict(episodes=lambda a: L.mi_ars_episodes(C.byref(a), None), update=lambda a: L.mi_ars_update(C.byref(a), None), iterate=lambda a: L.mi_ars_iterate(C.byref(a), 1, None))
def probe(key, who, **kw):
    out[key + ":" + who] = calls[who](args(**kw))
    out["text:" + key + ":" + who] = L.mi_ars_last_error().decode()
for who in calls:
    for key, kw in (("b_0", dict(n_top=0)), ("b_neg", dict(n_top=-1)), ("b_gt_N", dict(n_top=9)), ("N_0", dict(n_directions=0)), ("N_neg", dict(n_directions=-8)),
                    ("N_4097", dict(n_directions=4097, n_top=1)), ("noise_neg", dict(noise=-0.03)), ("noise_nan", dict(noise=nan)), ("noise_inf", dict(noise=inf)),
                    ("alpha_nan", dict(step_size=nan)), ("alpha_inf", dict(step_size=inf)),
                    ("null:policy", dict(policy=None)), ("null:stats", dict(stats=None)), ("null:norm", dict(norm=None)), ("null:iteration", dict(iteration=None)),
                    ("null:deltas", dict(deltas=None)), ("null:partials", dict(partials=None)), ("null:returns", dict(returns=None)),
                    ("misaligned:policy", dict(policy=4096 + 4)), ("misaligned:stats", dict(stats=4096 + 8)), ("misaligned:norm", dict(norm=4096 + 8)),
                    ("misaligned:iteration", dict(iteration=4096 + 8)), ("misaligned:deltas", dict(deltas=4096 + 4)), ("misaligned:partials", dict(partials=4096 + 4)),
                    ("misaligned:returns", dict(returns=4096 + 2))):
        probe(key, who, **kw)
for who in ("episodes", "iterate"):
    for key, kw in (("null:lengths", dict(lengths=None)), ("misaligned:lengths", dict(lengths=4096 + 2)), ("neg:max_workgroups", dict(max_workgroups=-1)),
                    ("neg:n_episodes", dict(n_episodes=-1))):
        probe(key, who, **kw)
probe("eval_with_noise", "episodes", n_episodes=5)
probe("eval_in_iterate", "iterate", n_episodes=5, noise=0.0)
out["null:args:episodes"] = L.mi_ars_episodes(None, None)
out["null:args:update"] = L.mi_ars_update(None, None)
out["null:args:iterate"] = L.mi_ars_iterate(None, 1, None)
out["zero:iterations"] = L.mi_ars_iterate(C.byref(args()), 0, None)
out["neg:iterations"] = L.mi_ars_iterate(C.byref(args()), -2, None)
out["empty:episodes"] = L.mi_ars_episodes(C.byref(K.ARSArgs()), None)
out["empty:update"] = L.mi_ars_update(C.byref(K.ARSArgs()), None)
out["empty:iterate"] = L.mi_ars_iterate(C.byref(K.ARSArgs()), 1, None)
out["version"] = L.mi_ars_version()
print("RESULT", json.dumps(out))
"""


def test_every_invalid_call_is_refused_before_hip(K):
    """no GPU here: a call that got as far as a launch would come back MI_ARS_EHIP (-2) or crash, never MI_ARS_EINVAL (-1)"""
    p = subprocess.run([sys.executable, "-c", _PROBE % ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-800:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    assert res.pop("version") == 1
    texts = {k[5:]: res.pop(k) for k in list(res) if k.startswith("text:")}
    assert len(res) >= 3 * 25 + 2 * 4 + 2 + 3 + 2 + 3
    for name, r in res.items():
        assert r == -1, (name, r)   # MI_ARS_EINVAL
    for who in ("episodes", "update", "iterate"):
        for key in ("b_0", "b_neg", "b_gt_N"):
            assert "n_top must be 1 .. n_directions" in texts[key + ":" + who], (key, who, texts[key + ":" + who])
        for key in ("N_0", "N_neg", "N_4097"):
            assert "n_directions must be 1 .. MI_ARS_MAX_DIRECTIONS" in texts[key + ":" + who], (key, who)
        for key in ("noise_neg", "noise_nan", "noise_inf"):
            assert "noise must be finite and >= 0" in texts[key + ":" + who], (key, who)
        for key in ("alpha_nan", "alpha_inf"):
            assert "step_size must be finite" in texts[key + ":" + who], (key, who)
        for key in ("misaligned:policy", "misaligned:stats", "misaligned:norm", "misaligned:iteration"):
            assert "16-byte aligned" in texts[key + ":" + who], (key, who)
    assert all("invalid argument" in t for t in texts.values())


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_ARS_SO"] = os.path.join(%r, "no_such_libmirl_ars.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_ars
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.ARSEngine is not None and "ARSEngine" in deep_rl_amd.__all__ and "LinearPolicy" in deep_rl_amd.__all__
try:
    _native_ars.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_thirteenth_library(K):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_thirteenth_library_needs_no_symbol_of_the_others(K):
    """ctypes loads the libraries RTLD_LOCAL: an unresolved mi_set_error / mi_ev_* would fail the load (RTLD_NOW here makes that immediate)"""
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_ars_version() == K.ABI_VERSION
    for other in ("mi_version", "mi_env_create", "mi_dqn_forward", "mi_pg_version", "mi_c51_version", "mi_iqn_version", "mi_qr_version", "mi_ddqn_version",
                  "mi_pdd_version", "mi_ns_version", "mi_nz_version", "mi_rb_version", "mi_ev_version", "mi_ev_episodes", "mi_md_version", "mi_set_error"):
        assert not hasattr(L, other), other
    src = open(os.path.join(CSRC, "mi_ars.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["mi_common.h", "../../include/mi_ars.h"] and "asm" not in re.sub(r"//.*", "", src)


FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]


def test_device_only_build_compiles_without_scratch():
    """every kernel of the library: no scratch, no spilled vector register, no LDS in the episode kernels (the figures DESIGN §27 quotes)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "mi_ars.hip"), "-o", os.path.join(d, "x.o")],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert len(names) == 3 and sum("ars_episode_kernel" in n for n in names) == 2 and sum("ars_update_kernel" in n for n in names) == 1
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * 3
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)] == [0] * 3
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out.stderr)) <= 256
    lds = dict(zip(names, (int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr))))
    assert all(v == 0 for n, v in lds.items() if "ars_episode_kernel" in n)


def test_thirteen_distinct_source_ids_and_the_twelve_older_ones_unchanged(K):
    import importlib

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    from deep_rl_amd import _native as N
    ids = {"_native": N.lib().mi_source_id().decode()}
    assert json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json"))).get("source_id") == ids["_native"] == srcid(S.SRCS + S.ALLSRC["_native"][1:])
    for mod, want in OLDER_IDS.items():
        ids[mod] = importlib.import_module("deep_rl_amd." + mod).source_id()
        assert ids[mod] == want == srcid(S.ALLSRC[mod]), mod
    ev = importlib.import_module("deep_rl_amd._native_ev")
    ids["_native_ev"] = ev.source_id()
    assert ids["_native_ev"] == srcid(S.ALLSRC["_native_ev"]) == json.load(open(os.path.join(ROOT, "profiles", "eval_bench.json")))["eval_source_id"]
    assert set(ids) == set(S.ALLSRC) and len(ids) == 12
    ids["_native_ars"] = K.source_id()
    assert srcid(ARS_ALLSRC) == K.source_id() and len(set(ids.values())) == 13
    bench = os.path.join(ROOT, "profiles", "ars_bench.json")
    if os.path.exists(bench):
        assert json.load(open(bench))["ars_source_id"] == K.source_id()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ARS_ALLSRC := " + " ".join(ARS_ALLSRC) in mk and "$(OUT_ARS)" in mk.split("all:")[1].splitlines()[0] and "$(OUT_ARS)" in mk.split("clean:")[1]
    assert "-DMI_ARS_SOURCE_ID" in mk and "OUT_ARS ?= ../libmirl_ars.so" in mk
    assert "_native_ars.lib().mi_ars_version() == _native_ars.ABI_VERSION" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_engine_surface():
    import inspect

    import deep_rl_amd as D
    from deep_rl_amd import checkpoint
    from deep_rl_amd._native import MiError

    sig = inspect.signature(D.ARSEngine.__init__)
    assert list(sig.parameters)[1:8] == ["n_directions", "n_top", "step_size", "noise", "normalize", "seed", "env_id_base"] and "device" in sig.parameters
    assert [sig.parameters[n].default for n in ("n_directions", "n_top", "step_size", "noise", "normalize", "seed", "env_id_base")] == [8, None, 0.02, 0.03, True, 1, 0]
    ev = inspect.signature(D.ARSEngine.evaluate)
    assert (ev.parameters["episodes"].default, ev.parameters["seed"].default, ev.parameters["env_id_base"].default) == (100, 1, 1 << 40)
    assert all(callable(getattr(D.ARSEngine, n)) for n in ("train", "evaluate", "drain_episodes"))
    # the checks of the constructor come before anything is allocated or loaded
    for kw in (dict(n_directions=0), dict(n_directions=4097), dict(n_top=0), dict(n_top=9), dict(noise=-1.0), dict(noise=float("nan")), dict(step_size=float("nan"))):
        with pytest.raises(MiError):
            D.ARSEngine(**kw)
    assert "ARSEngine" in inspect.getsource(checkpoint) and '"stats"' in inspect.getsource(checkpoint) and '"norm"' in inspect.getsource(checkpoint)
    script = open(os.path.join(ROOT, "deep_rl_amd", "ars.py")).read()
    for knob in ('"N_DIRECTIONS", "8"', '"N_TOP"', '"STEP_SIZE", "0.02"', '"NOISE", "0.03"', '"NORMALIZE", "1"', '"NUM_ITERATIONS", "40"', '"SEED", "1"', "ARSEngine("):
        assert knob in script, knob
    # deep_rl_amd.evaluate(ARSEngine) stays the error it was: the engine has no `q`, and the evaluation library no linear kind
    from deep_rl_amd import evaluate as E
    assert "ARSEngine" not in E.ENGINES_EVALUABLE and not hasattr(D.ARSEngine, "q")
