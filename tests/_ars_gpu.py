"""Device-side helpers of the ARS GPU tests — TEST INFRASTRUCTURE for libmirl_ars.so.  Every call goes into poisoned buffers with a guard band behind each (NaN for
the floats, 0xEE bytes for everything else), as the evaluation tests do: the guard bands must come back untouched, everything inside must be overwritten."""
import ctypes as C

import numpy as np
import torch

import _ars_ref as A

f32 = np.float32
GUARD = 64
EE32 = -286331154   # 0xEEEEEEEE as an int32
LIMIT = A.LIMIT


def to_np(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == f32 else np.uint64)


class DevState:
    """the four state tensors of a reference-style state dict"""

    def __init__(self, dev, st):
        self.dev = dev
        self.policy = torch.from_numpy(np.array(st["M"], f32)).to(dev)
        self.stats = torch.from_numpy(np.array(st["stats"], np.float64)).to(dev)
        self.norm = torch.from_numpy(np.array(st["norm"], np.float64)).to(dev)
        self.iteration = torch.tensor([int(st["k"])], dtype=torch.int64, device=dev)

    def read(self):
        torch.cuda.synchronize(self.dev)
        return dict(M=to_np(self.policy), stats=to_np(self.stats), norm=to_np(self.norm), k=int(self.iteration.item()))

    def raw(self):
        torch.cuda.synchronize(self.dev)
        return b"".join(to_np(t).tobytes() for t in (self.policy, self.stats, self.norm, self.iteration))


def _args(K, ds, buf, N, b, n_episodes, noise, seed, base, max_workgroups, normalize, step_size, trace=True, truncated=True):
    return K.ARSArgs(K.ptr(ds.policy), K.ptr(ds.stats), K.ptr(ds.norm), K.ptr(ds.iteration), K.ptr(buf["deltas"]), K.ptr(buf["returns"]), K.ptr(buf["lengths"]),
                     K.ptr(buf["truncated"]) if truncated else None, K.ptr(buf["actions"]) if trace else None, K.ptr(buf["partials"]), seed, base, N, b, n_episodes,
                     max_workgroups, int(normalize), float(step_size), float(noise), 0)


def buffers(dev, N, E, rows=1):
    """poisoned outputs: returns / lengths [rows * E + GUARD], truncated [E + GUARD], actions [E + 1][500], deltas [N + 8][8], partials [2 N + 8][9]"""
    return dict(returns=torch.full((rows * E + GUARD,), float("nan"), dtype=torch.float32, device=dev),
                lengths=torch.full((rows * E + GUARD,), EE32, dtype=torch.int32, device=dev),
                truncated=torch.full((E + GUARD,), 0xEE, dtype=torch.uint8, device=dev),
                actions=torch.full((E + 1, LIMIT), 0xEE, dtype=torch.uint8, device=dev),
                deltas=torch.full((N + 8, 8), float("nan"), dtype=torch.float32, device=dev),
                partials=torch.full((2 * N + 8, 9), float("nan"), dtype=torch.float64, device=dev))


def _collect(dev, buf, N, E, rows, train, trace=True):
    torch.cuda.synchronize(dev)
    out = {k: to_np(v) for k, v in buf.items()}
    n = rows * E
    assert np.isnan(out["returns"][n:]).all() and (out["lengths"][n:] == EE32).all() and (out["truncated"][E:] == 0xEE).all() and (out["actions"][E:] == 0xEE).all()
    assert not np.isnan(out["returns"][:n]).any() and ((out["lengths"][:n] >= 1) & (out["lengths"][:n] <= LIMIT)).all() and (out["truncated"][:E] <= 1).all()
    if train:
        assert np.isnan(out["deltas"][N:]).all() and np.isnan(out["partials"][2 * N:]).all()
        assert np.isfinite(out["deltas"][:N]).all() and np.isfinite(out["partials"][:2 * N]).all()
    else:
        assert np.isnan(out["deltas"]).all() and np.isnan(out["partials"]).all()
    if not trace:
        assert (out["actions"] == 0xEE).all()
    res = dict(returns=out["returns"][:n].reshape(rows, E), lengths=out["lengths"][:n].reshape(rows, E), truncated=out["truncated"][:E], actions=out["actions"][:E],
               deltas=out["deltas"][:N], partials=out["partials"][:2 * N])
    if rows == 1:
        res["returns"], res["lengths"] = res["returns"][0], res["lengths"][0]
    return res


def run_episodes(K, dev, ds, N, noise=A.NOISE, seed=A.SEED, base=A.TRAIN_BASE, max_workgroups=0, trace=True):
    """one training-mode mi_ars_episodes call -> numpy outputs"""
    buf = buffers(dev, N, 2 * N)
    a = _args(K, ds, buf, N, N, 0, noise, seed, base, max_workgroups, 1, A.STEP_SIZE, trace)
    K.check(K.lib().mi_ars_episodes(C.byref(a), K.stream_ptr(dev)), "mi_ars_episodes")
    return _collect(dev, buf, N, 2 * N, 1, True, trace)


def run_eval(K, dev, ds, E, seed=A.SEED, base=A.EVAL_BASE, max_workgroups=0, trace=True):
    """one evaluation-mode mi_ars_episodes call (N = 8 is passed and not read)"""
    buf = buffers(dev, 8, E)
    a = _args(K, ds, buf, 8, 8, E, 0.0, seed, base, max_workgroups, 1, A.STEP_SIZE, trace)
    K.check(K.lib().mi_ars_episodes(C.byref(a), K.stream_ptr(dev)), "mi_ars_episodes")
    return _collect(dev, buf, 8, E, 1, False, trace)


def run_update(K, dev, ds, returns, deltas, partials, b, step_size=A.STEP_SIZE, normalize=True):
    """one mi_ars_update call on placed inputs; the inputs must come back as they went in"""
    N = len(deltas)
    t = dict(returns=torch.from_numpy(np.ascontiguousarray(returns, f32)).to(dev), deltas=torch.from_numpy(np.ascontiguousarray(deltas, f32)).to(dev),
             partials=torch.from_numpy(np.ascontiguousarray(partials, np.float64)).to(dev), lengths=None, truncated=None, actions=None)
    before = {k: to_np(t[k]).tobytes() for k in ("returns", "deltas", "partials")}
    a = _args(K, ds, t, N, b, 0, A.NOISE, A.SEED, A.TRAIN_BASE, 0, normalize, step_size, trace=False, truncated=False)
    K.check(K.lib().mi_ars_update(C.byref(a), K.stream_ptr(dev)), "mi_ars_update")
    torch.cuda.synchronize(dev)
    assert all(to_np(t[k]).tobytes() == before[k] for k in before)


def run_iterate(K, dev, ds, N, b, iterations, normalize=True, noise=A.NOISE, seed=A.SEED, base=A.TRAIN_BASE, max_workgroups=0, step_size=A.STEP_SIZE):
    """one mi_ars_iterate call -> numpy outputs; returns / lengths [iterations][2 N]"""
    buf = buffers(dev, N, 2 * N, iterations)
    a = _args(K, ds, buf, N, b, 0, noise, seed, base, max_workgroups, normalize, step_size, trace=False)
    K.check(K.lib().mi_ars_iterate(C.byref(a), iterations, K.stream_ptr(dev)), "mi_ars_iterate")
    out = _collect(dev, buf, N, 2 * N, iterations, True, trace=False)
    if iterations == 1:
        out["returns"], out["lengths"] = out["returns"][None], out["lengths"][None]
    return out


def device_deltas(K, dev, N, k, seed=A.SEED):
    """the device's own deltas f32 [N][8] of iteration k: they are keyed (seed, i, k) and depend on nothing else, so a scratch state's episodes give them"""
    ds = DevState(dev, dict(A.fresh_state(), k=k))
    return run_episodes(K, dev, ds, N, seed=seed, trace=False)["deltas"]


def check_episodes(out, ref, train=True):
    """every output of every episode against the reference's, bit for bit, none left out"""
    assert len(ref) == len(out["lengths"])
    for e, r in enumerate(ref):
        n = r["length"]
        assert out["lengths"][e] == n and out["returns"][e] == r["ret"] and out["truncated"][e] == r["truncated"], (e, out["lengths"][e], n)
        assert np.array_equal(out["actions"][e, :n], r["actions"]), e
        assert (out["actions"][e, n:] == 0xEE).all(), e          # the bytes behind a trace row's end stay as they were
        if train:
            assert np.array_equal(bits(out["partials"][e]), bits(r["partial"])), (e, out["partials"][e], r["partial"])


def check_state(got, want, norm_rel=1e-9):
    """M, stats and k bit for bit; norm within relative 1e-9 of the float64 restatement"""
    assert np.array_equal(bits(np.asarray(got["M"], f32)), bits(np.asarray(want["M"], f32))), (got["M"], want["M"])
    assert np.array_equal(bits(got["stats"]), bits(np.asarray(want["stats"], np.float64))), (got["stats"], want["stats"])
    assert got["k"] == want["k"]
    w = np.asarray(want["norm"], np.float64)
    assert (np.abs(got["norm"] - w) <= norm_rel * np.abs(w)).all(), (got["norm"], w)
