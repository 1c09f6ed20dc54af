"""CPU-only checks of the fourth library's boundary: libmirl_iqn.so loads without a GPU, exports and binds every symbol include/mi_iqn.h declares, reports errors
through return codes — and leaves libmirl.so, libmirl_pg.so and libmirl_c51.so what they were."""
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
IQN_ALLSRC = S.ALLSRC["_native_iqn"]
# the three other lists, as the Makefile states them (C51's holds mi_torso.h, the torso it shares with QR-DQN and Double DQN; IQN's does not)
OTHER_ALLSRC = {
    "ALLSRC": " ".join(S.ALLSRC["_native"]),
    "PG_ALLSRC": " ".join(S.ALLSRC["_native_pg"]),
    "C51_ALLSRC": " ".join(S.ALLSRC["_native_c51"]),
}


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native, _native_c51, _native_iqn, _native_pg

    if not all(os.path.exists(p) for p in (_native_iqn.SO_PATH, _native_c51.SO_PATH, _native_pg.SO_PATH, _native.SO_PATH)):
        import __graft_entry__

        __graft_entry__.build()
    return _native_iqn


def _header():
    hdr = open(os.path.join(ROOT, "include", "mi_iqn.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_symbols_all_exported_and_bound(K):
    hdr = _header()
    declared = set(re.findall(r"\b(mi_iqn_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 10
    L = C.CDLL(K.SO_PATH)
    for name in declared:
        assert hasattr(L, name), "libmirl_iqn.so does not export %s" % name
    assert declared == set(K.SIGNATURES), declared ^ set(K.SIGNATURES)
    assert K.lib().mi_iqn_version() == K.ABI_VERSION == int(re.search(r"#define MI_IQN_VERSION (\d+)", hdr).group(1))
    macros = dict(NPARAMS=K.NPARAMS, EMB=K.EMB, NCOS=K.NCOS, HID=K.HID, N_TAU=K.N_TAU, N_TAU_PRIME=K.N_TAU_PRIME, N_QUANT=K.N_QUANT, MAX_SLABS=K.MAX_SLABS,
                  SLAB_STRIDE=K.SLAB_STRIDE, MAX_STEPS_PER_CALL=K.MAX_STEPS_PER_CALL, **K.OFFSETS)
    for macro, value in macros.items():
        assert int(re.search(r"#define MI_IQN_%s (\d+)" % macro, hdr).group(1)) == value, macro


def test_offsets_sum_to_44898(K):
    order = ("FW1", "FB1", "FW2", "FB2", "FW3", "FB3", "CW", "CB", "QW1", "QB1", "QW2", "QB2")
    off = 0
    for k in order:
        assert K.OFFSETS[k] == off, k
        off += K.SIZES[k]
    assert off == K.NPARAMS == 44_898 == K.F_NPARAMS + K.C_NPARAMS + K.Q_NPARAMS
    assert K.SIZES["QW1"] == K.HID * K.EMB and K.SIZES["CW"] == K.EMB * K.NCOS and K.SLAB_STRIDE % 4 == 0 and K.SLAB_STRIDE >= K.NPARAMS + 1
    import _iqn_ref as R
    assert R.OFF == K.OFFSETS and R.NPARAMS == K.NPARAMS and all(int(__import__("numpy").prod(R.SHAPES[k])) == K.SIZES[k] for k in order)


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
    return re.findall(r"([a-z_0-9]+)\s*;", re.sub(r"\b(lr|beta1|beta2|slope),", r"\1;", body))


def test_struct_layouts_match_header(K):
    hdr = _header()
    assert _struct_fields(hdr, "mi_iqn_ring_t") == [f[0] for f in K.IQNRing._fields_]
    assert _struct_fields(hdr, "mi_iqn_act_t") == [f[0] for f in K.IQNAct._fields_]
    assert _struct_fields(hdr, "mi_iqn_batch_t") == [f[0] for f in K.IQNBatch._fields_]
    assert _struct_fields(hdr, "mi_iqn_adam_t") == [f[0] for f in K.IQNAdam._fields_]
    assert C.sizeof(K.IQNRing) == 4 * 8 + 8 + 4 + 4
    assert C.sizeof(K.IQNAct) == 8 * 8 + 2 * 8 + 2 * 8 + 4 + 4
    assert C.sizeof(K.IQNBatch) == 13 * 8 + 3 * 8 + 4 + 4 + 8
    assert C.sizeof(K.IQNAdam) == 2 * 8 + 8 + 4 * 8
    L = K.lib()
    assert L.mi_iqn_workspace_bytes(0) == 0 and L.mi_iqn_workspace_bytes(1) == K.SLAB_STRIDE * 4
    assert L.mi_iqn_workspace_bytes(64) == L.mi_iqn_workspace_bytes(4096) == K.MAX_SLABS * K.SLAB_STRIDE * 4
    sid = K.source_id()
    assert len(sid) == 12 and sid != "unknown"


_NULL_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from deep_rl_amd import _native_iqn as K
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
# structs that are there but empty are errors too, as are a ring of one slot and a batch of 0 rows
r, b, a, act = K.IQNRing(), K.IQNBatch(), K.IQNAdam(), K.IQNAct()
out["empty:act"] = L.mi_iqn_act_steps(None, C.byref(r), C.byref(act), None)
out["empty:target"] = L.mi_iqn_target(C.byref(r), C.byref(b), None)
out["empty:grad"] = L.mi_iqn_grad(C.byref(r), C.byref(b), None)
out["empty:update"] = L.mi_iqn_update(C.byref(r), C.byref(b), C.byref(a), None)
r.slots, r.n_envs = 1, 0
out["empty:ring"] = L.mi_iqn_grad(C.byref(r), C.byref(b), None)
out["text"] = L.mi_iqn_last_error().decode()
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
    harmless = {"mi_iqn_version", "mi_iqn_last_error", "mi_iqn_source_id", "mi_iqn_workspace_bytes"}   # (a batch of 0 rows needs 0 bytes)
    for name, r in res.items():
        if name in harmless:
            continue
        assert r == K.MI_IQN_EINVAL, (name, r)


_IMPORT_PROBE = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["MIRL_IQN_SO"] = os.path.join(%r, "no_such_libmirl_iqn.so")
import deep_rl_amd
from deep_rl_amd import _native, _native_iqn
assert _native.lib().mi_version() == _native.ABI_VERSION
assert deep_rl_amd.IQNEngine is not None and deep_rl_amd.QuantileNetwork is not None
try:
    _native_iqn.lib()
except _native.MiError as e:
    assert "missing" in str(e)
    print("OK")
"""


def test_package_imports_without_the_fourth_library(K):
    """libmirl_iqn.so loads lazily: with it absent `import deep_rl_amd` and libmirl.so work, and the first use of the IQN path is a loud error"""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([sys.executable, "-c", _IMPORT_PROBE % (ROOT, d)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stderr[-800:]


def test_fourth_library_needs_no_symbol_of_the_others(K):
    L = C.CDLL(K.SO_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert L.mi_iqn_version() == K.ABI_VERSION
    assert not hasattr(L, "mi_version") and not hasattr(L, "mi_env_create") and not hasattr(L, "mi_c51_version")


def test_the_other_libraries_keep_their_sources(K):
    """the feature changes no token of the three existing libraries: the Makefile's three *_ALLSRC lists are the parent's, their ids are what csrc/srcid.py gives
    for those lists (and what the committed profiles record), and the new library has an id of its own"""
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51 as C51
    from deep_rl_amd import _native_pg as PG

    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name, value in OTHER_ALLSRC.items():
        assert re.search(r"^%s = %s$" % (re.escape(name), re.escape(value)), mk, flags=re.M), name
    assert "IQN_ALLSRC = " + " ".join(IQN_ALLSRC) in mk and "$(OUT_IQN)" in mk and "IQN_SRCID" in mk

    def srcid(files):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "srcid.py")] + files, cwd=CSRC, capture_output=True, text=True, timeout=60)
        return out.stdout.strip()

    assert json.load(open(os.path.join(ROOT, "profiles", "latest_pmc.json"))).get("source_id") == N.lib().mi_source_id().decode()
    assert json.load(open(os.path.join(ROOT, "profiles", "c51_bench.json")))["c51_source_id"] == C51.source_id() == srcid(OTHER_ALLSRC["C51_ALLSRC"].split())
    assert srcid(OTHER_ALLSRC["PG_ALLSRC"].split()) == PG.source_id()
    assert srcid(IQN_ALLSRC) == K.source_id()
    assert len({N.lib().mi_source_id().decode(), PG.source_id(), C51.source_id(), K.source_id()}) == 4


def test_engine_surface_is_callable_where_it_must_be():
    import inspect

    from deep_rl_amd import IQNEngine

    methods = ("reset", "act", "drain_episodes", "sample", "target", "grad", "train_step", "sync_target")
    for name in methods:
        assert inspect.isfunction(getattr(IQNEngine, name)), name
    src = "".join(inspect.getsource(c.__init__) for c in IQNEngine.__mro__ if "__init__" in vars(c) and c is not object)   # the base class allocates the ring
    for name in methods:
        assert "self.%s =" % name not in src and "self.%s," % name not in src, name
    for name in ("observations", "actions", "rewards", "terminated", "batch_inds", "grads", "loss", "taus", "current_action_quantiles", "target_action_quantiles",
                 "next_actions", "episode_stats"):
        assert "self.%s = " % name in src, name


def test_modules_are_views_of_one_packed_buffer_on_the_cpu():
    """the reference's constructor signatures and forward shapes (iqn.py:156-158, :196-199) on CPU tensors; pack() joins the three modules in the optimizer's order"""
    import numpy as np
    import torch
    from types import SimpleNamespace

    import deep_rl_amd as M
    import _iqn_ref as R
    env = SimpleNamespace(observation_space=SimpleNamespace(shape=(4,)), action_space=SimpleNamespace(n=2), device="cpu")
    torch.manual_seed(3)
    fe = M.FeaturesExtractor(env)
    cn = M.CosineEmbeddingNetwork(num_cosines=64, embedding_dim=64, device="cpu")
    qn = M.QuantileNetwork(num_actions=2, embedding_dim=64, device="cpu")
    flat = M.pack(fe, cn, qn)
    assert flat.numel() == 44_898 and [tuple(p.shape) for p in (*fe.parameters(), *cn.parameters(), *qn.parameters())] == [R.SHAPES[k] for k in R.ORDER]
    assert all(p.data_ptr() == flat.data_ptr() + 4 * R.OFF[k] for p, k in zip((*fe.parameters(), *cn.parameters(), *qn.parameters()), R.ORDER))
    assert float(fe.net[0].bias.abs().max()) == 0.0 and float(cn.net[0].bias.abs().max()) > 0.0   # he-init zeroes the extractor's biases only
    obs, taus = torch.randn(3, 4), torch.rand(3, 32)
    with torch.no_grad():
        emb = fe(obs); te = cn(taus); quant = qn(emb, te)
    assert emb.shape == (3, 64) and te.shape == (3, 32, 64) and quant.shape == (3, 32, 2)
    r = R.forward(flat.numpy(), obs.numpy(), taus.numpy(), np.float64)
    assert np.abs(quant.numpy() - r["quantiles"]).max() <= 1e-5
