"""Augmented Random Search on the MI355X (libmirl_ars.so, include/mi_ars.h, deep_rl_amd.ARSEngine) against the CPU restatement tests/_ars_ref.py.

Given the device's own deltas and norm, every output is the reference's BIT FOR BIT — lengths, returns, truncated, every traced action, the bytes behind a trace
row's end, the partial sums, M, stats, k and the per-iteration returns of whole chains — with no episode, step or case left out.  Two things carry a bound: the
deltas themselves against the float64 Box-Muller of the same Philox words (the bound tests/test_gpu_noisy_cases.py applies to the same construction,
_noisy_ref.BOUND_DRAW), and norm within relative 1e-9 (tests/test_ars_ref_cpu.py shows the conditioning that rests on).  Observed maxima go to
ars_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _ars_gpu as G
import _ars_ref as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native_ars
    return _native_ars


def record(key, value):
    from _c51_ref import results_dir
    from deep_rl_amd import _native_ars
    path = os.path.join(results_dir(), "ars_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d["ars_source_id"] = _native_ars.source_id()
    d[key] = value
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


# a state in mid-run: a normaliser that is neither 0 / 1 nor symmetric, and an iteration past 2^32 / 8 so that the high word of the draw's index is used
MID = dict(M=np.zeros(8, f32), stats=np.zeros(9), norm=np.array([0.01, -0.02, 0.003, 0.01, 2.0, 1.5, 8.0, 1.25]), k=(1 << 30) + 3)


@pytest.mark.parametrize("N", A.SHAPES)
@pytest.mark.parametrize("state", ["fresh", "mid"])
def test_training_episodes_of_random_policies_bit_for_bit(dev, R, K, N, state):
    st = A.fresh_state() if state == "fresh" else MID
    out = G.run_episodes(K, dev, G.DevState(dev, st), N)
    G.check_episodes(out, A.episodes(R, st, out["deltas"], A.NOISE))


@pytest.mark.parametrize("N", [n for n in A.SHAPES if n <= A.CONTROLLER_MAX_N])
def test_training_episodes_around_the_controller_bit_for_bit(dev, R, K, N):
    """M = the controller, the default noise: every lane runs to (or near) the limit"""
    st = dict(A.fresh_state(), M=np.array(A.controller()), k=2)
    out = G.run_episodes(K, dev, G.DevState(dev, st), N)
    G.check_episodes(out, A.episodes(R, st, out["deltas"], A.NOISE))
    assert out["truncated"].any() and (out["lengths"] == 500).any()


def test_mixed_case_a_waves_lanes_on_very_different_lengths(dev, R, K):
    m = A.mixed_case()
    st = dict(A.fresh_state(), M=np.array(A.controller()))
    out = G.run_episodes(K, dev, G.DevState(dev, st), 8, noise=m["noise"])
    ref = A.episodes(R, st, out["deltas"], m["noise"])
    G.check_episodes(out, ref)
    assert out["truncated"].any() and out["lengths"].min() < 100 and out["lengths"].max() == 500


def test_deltas_against_float64_and_the_prefix_property(dev, R, K):
    from _noisy_ref import BOUND_DRAW
    worst = 0.0
    for N, k in ((200, 0), (33, (1 << 30) + 3), (8, 1), (8, 5)):
        d = G.device_deltas(K, dev, N, k)
        worst = max(worst, float(np.abs(d.astype(np.float64) - A.normal64(R, A.SEED, N, k)).max()))
    print("device deltas against the float64 Box-Muller: %.3g (bound %.3g)" % (worst, BOUND_DRAW["z"]))
    record("deltas", {"max_abs": worst, "bound": BOUND_DRAW["z"]})
    assert worst <= BOUND_DRAW["z"]
    d8, d3 = G.device_deltas(K, dev, 8, 4), G.device_deltas(K, dev, 3, 4)
    assert np.array_equal(G.bits(d3), G.bits(d8[:3]))
    assert not np.array_equal(d8, G.device_deltas(K, dev, 8, 5)) and not np.array_equal(d8, G.device_deltas(K, dev, 8, 4, seed=A.SEED + 1))
    # both signs of a direction and every max_workgroups see the same deltas: the grid does not enter the key
    ds = G.DevState(dev, dict(A.fresh_state(), k=4))
    assert np.array_equal(G.bits(G.run_episodes(K, dev, ds, 200, max_workgroups=1)["deltas"][:8]), G.bits(d8))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("N,b", A.CHAIN_SHAPES)
def test_chain_of_iterations_bit_for_bit(dev, R, K, N, b, normalize):
    """mi_ars_iterate for 1, 2 and 5 iterations = the reference loop run on the device's deltas; one call of 5 = five calls of 1; max_workgroups 1, 2 and the
    default agree"""
    top = max(A.CHAIN_ITERATIONS)
    deltas = [G.device_deltas(K, dev, N, k) for k in range(top)]
    want, rows, st = {}, [], A.fresh_state()
    for t in range(top):
        st, ret, _ = A.iterate(R, st, N, b, deltas[t], normalize=normalize)
        rows.append(ret)
        want[t + 1] = (st, np.stack(rows))
    raw = {}
    for n in A.CHAIN_ITERATIONS:
        ds = G.DevState(dev, A.fresh_state())
        out = G.run_iterate(K, dev, ds, N, b, n, normalize)
        G.check_state(ds.read(), want[n][0])
        assert np.array_equal(G.bits(out["returns"]), G.bits(want[n][1])) and np.array_equal(out["lengths"], want[n][1].astype(np.int32))
        assert np.array_equal(G.bits(out["deltas"]), G.bits(deltas[n - 1]))
        raw[n] = (ds.raw(), out["returns"].tobytes())
        if not normalize:
            assert np.array_equal(ds.read()["norm"], A.fresh_state()["norm"])
    ds = G.DevState(dev, A.fresh_state())
    singles = [G.run_iterate(K, dev, ds, N, b, 1, normalize)["returns"] for _ in range(top)]
    assert ds.raw() == raw[top][0] and np.concatenate(singles).tobytes() == raw[top][1]
    for mw in (1, 2):
        ds = G.DevState(dev, A.fresh_state())
        out = G.run_iterate(K, dev, ds, N, b, top, normalize, max_workgroups=mw)
        assert ds.raw() == raw[top][0] and out["returns"].tobytes() == raw[top][1]


def test_max_workgroups_does_not_change_the_episodes_of_several_blocks(dev, K):
    """400 episodes are seven 64-lane blocks: one workgroup walks all of them, two take them alternately, the default takes one each"""
    outs = [G.run_episodes(K, dev, G.DevState(dev, MID), 200, max_workgroups=mw) for mw in (0, 1, 2, 5)]
    for o in outs[1:]:
        for name in ("returns", "lengths", "truncated", "actions", "deltas", "partials"):
            assert outs[0][name].tobytes() == o[name].tobytes(), name


def test_engine_matches_the_reference_and_a_second_engine_in_the_process(dev, R, K):
    import deep_rl_amd as D
    N, b, n = 8, 4, 5
    engines = [D.ARSEngine(n_directions=N, n_top=b, seed=A.SEED, env_id_base=A.TRAIN_BASE, device=dev) for _ in range(2)]
    ret = [G.to_np(e.train(n)) for e in engines]
    deltas = [G.device_deltas(K, dev, N, k) for k in range(n)]
    st, want = A.chain(R, N, b, n, deltas)
    for e, r in zip(engines, ret):
        assert np.array_equal(G.bits(r), G.bits(want)) and tuple(r.shape) == (n, 2 * N)
        G.check_state(dict(M=G.to_np(e.policy.flat), stats=G.to_np(e.stats), norm=G.to_np(e.norm), k=int(e.iteration.item())), st)
    count, eps = engines[0].drain_episodes()
    assert count == n * 2 * N and [x[0] for x in eps[:2 * N]] == list(range(2 * N)) and [x[2] for x in eps] == want.reshape(-1).tolist()
    assert all(x[1] == int(x[2]) for x in eps)
    assert np.array_equal(G.to_np(engines[0].policy.weight).reshape(-1), G.to_np(engines[0].policy.flat)) and tuple(engines[0].policy.weight.shape) == (2, 4)
    with pytest.raises(K.MiError, match="not supported"):
        D.evaluate(engines[0])   # the evaluation library has no linear kind: ARSEngine.evaluate is the engine's own


def test_nan_policy_every_launch_ends(dev, R, K):
    st = dict(A.fresh_state(), M=np.full(8, np.nan, f32), k=1)
    ds = G.DevState(dev, st)
    out = G.run_episodes(K, dev, ds, 8)
    ref = A.episodes(R, st, out["deltas"], A.NOISE)
    G.check_episodes(out, ref)                                   # lengths equal the reference's: a NaN score compares false, action 0 throughout
    assert all((out["actions"][e, :out["lengths"][e]] == 0).all() for e in range(16))
    ev = G.run_eval(K, dev, ds, 5)
    assert all((ev["actions"][e, :ev["lengths"][e]] == 0).all() for e in range(5))
    it = G.run_iterate(K, dev, ds, 8, 4, 2)
    got = ds.read()
    assert got["k"] == 3 and np.isfinite(it["returns"]).all() and np.isnan(got["M"]).all() and np.isfinite(got["stats"]).all()
    assert np.array_equal(it["returns"][0], np.array([e["ret"] for e in ref], f32))


@pytest.mark.parametrize("E", A.EVAL_EPISODES)
@pytest.mark.parametrize("net", ["controller", "trained"])
def test_evaluation_mode_exact_and_the_state_untouched(dev, R, K, E, net):
    if net == "controller":
        st = dict(A.fresh_state(), M=np.array(A.controller()), k=11)
    else:   # five iterations of the reference on its own draw: a normaliser in use and a policy that is neither good nor hopeless
        st, _ = A.chain(R, 8, 4, 5)
    ds = G.DevState(dev, st)
    before = ds.raw()
    out = G.run_eval(K, dev, ds, E)
    G.check_episodes(out, A.evaluate(R, st, E), train=False)
    assert ds.raw() == before
    if net == "controller":
        assert out["truncated"].all()
    if E == max(A.EVAL_EPISODES):
        for mw in (1, 2):
            o = G.run_eval(K, dev, ds, E, max_workgroups=mw)
            assert all(o[name].tobytes() == out[name].tobytes() for name in ("returns", "lengths", "truncated", "actions"))


def test_engine_evaluate_is_the_evaluation_mode(dev, R):
    import deep_rl_amd as D
    eng = D.ARSEngine(n_directions=8, n_top=4, seed=A.SEED, env_id_base=A.TRAIN_BASE, device=dev)
    eng.train(5)
    torch.cuda.synchronize(dev)
    st = dict(M=G.to_np(eng.policy.flat), stats=G.to_np(eng.stats), norm=G.to_np(eng.norm), k=int(eng.iteration.item()))
    res = eng.evaluate(5, trace=True)
    ref = A.evaluate(R, st, 5)
    from deep_rl_amd import _native_ars
    assert isinstance(res, D.EvalResult) and res.episodes == 5 and res.min_gap is None and res.source_id == _native_ars.source_id()
    assert G.to_np(res.returns).tolist() == [e["ret"] for e in ref] and G.to_np(res.lengths).tolist() == [e["length"] for e in ref]
    assert G.to_np(res.truncated).tolist() == [e["truncated"] for e in ref]
    assert res.mean == sum(e["ret"] for e in ref) / 5 and "mean_return=" in res.line()
    for e, r in enumerate(ref):
        assert np.array_equal(G.to_np(res.actions)[e, :r["length"]], r["actions"])


def test_checkpoint_resumes_bit_for_bit(dev, tmp_path):
    import deep_rl_amd as D
    from deep_rl_amd import checkpoint

    kw = dict(n_directions=8, n_top=4, seed=3, env_id_base=17, device=dev)
    straight = D.ARSEngine(**kw)
    r6 = G.to_np(straight.train(6))
    first = D.ARSEngine(**kw)
    r3 = G.to_np(first.train(3))
    path = checkpoint.save(str(tmp_path / "ars"), first)
    with np.load(path) as z:
        assert str(z["kind"]) == "ARSEngine" and {"params", "stats", "norm", "iteration"} <= set(z.files) and int(z["iteration"][0]) == 3
    resumed = checkpoint.load(path, D.ARSEngine(**kw))
    r3b = G.to_np(resumed.train(3))
    assert np.concatenate([r3, r3b]).tobytes() == r6.tobytes()
    for name in ("stats", "norm", "iteration"):
        assert G.to_np(getattr(resumed, name)).tobytes() == G.to_np(getattr(straight, name)).tobytes(), name
    assert G.to_np(resumed.policy.flat).tobytes() == G.to_np(straight.policy.flat).tobytes()
    with pytest.raises(D._native.MiError, match="written for"):
        checkpoint.load(path, D.ARSEngine(**dict(kw, seed=4)))
