"""Greedy policy evaluation on the MI355X (libmirl_eval.so, include/mi_eval.h, deep_rl_amd.evaluate): the action values against the owning libraries' forward
calls bit for bit, whole episodes against the CPU oracle's CartPole replayed under the device's own actions, teacher-forced endings on and around the 500-step
limit, independence of the grid, untouched training state, poisoned outputs, the public function and the CLI.

No tolerance appears here except the owning families' close-value distances (tests/_eval_ref.py `close`): a float32 device may pick the other action only where
the float64 values are closer than that.  Everything else is exact.  tests/test_eval_ref_cpu.py shows on the reference alone that the networks, the seed and the
episodes used here meet the conditions the comparisons rest on.  Observed figures go to eval_gpu_results.json in the tests' results directory."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _c51_ref as X5
import _eval_ref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GUARD = 64                       # elements of guard band behind every output buffer
EE32 = -286331154                # 0xEEEEEEEE as an int32


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
    from deep_rl_amd import _native_ev
    return _native_ev


@pytest.fixture(autouse=True)
def _fdlibm(R):
    R.set_sincos_mode("fdlibm")
    yield
    R.set_sincos_mode("libm")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def record(key, value):
    path = os.path.join(X5.results_dir(), "eval_gpu_results.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    from deep_rl_amd import _native_ev
    d["eval_source_id"] = _native_ev.source_id()
    d[key] = value
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


_PARAMS = {}


def params_of(dev, net, kind):
    """the device copy of a network's parameters ("controller" / "default" / "nan"), made once"""
    if (net, kind) not in _PARAMS:
        p = E.controller(kind) if net == "controller" else E.default_params(kind)
        if net == "nan":
            p = np.full_like(p, np.nan)
        _PARAMS[(net, kind)] = torch.from_numpy(np.array(p)).to(dev)
    return _PARAMS[(net, kind)]


def support_of(kind, support=None):
    return tuple(support or E.DEFAULT_SUPPORT.get(kind, (0.0, 1.0)))


def run(K, dev, kind, params, n, seed=E.SEED, base=E.ENV_BASE, forced_actions=None, forced_starts=None, trace=True, max_workgroups=0, support=None, stream=None,
        outputs=("returns", "truncated", "min_gap")):
    """one mi_ev_episodes call into poisoned buffers with a guard band behind each: NaN for the floats, 0xEE bytes for everything else.  The guard bands must come
    back untouched and everything inside n must be overwritten (the action rows up to lengths[e] only).  -> numpy arrays of the first n entries"""
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        buf = dict(returns=torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev),
                   lengths=torch.full((n + GUARD,), EE32, dtype=torch.int32, device=dev),
                   truncated=torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device=dev),
                   min_gap=torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev),
                   actions=torch.full((n + 1, E.LIMIT), 0xEE, dtype=torch.uint8, device=dev))
        fa = None if forced_actions is None else torch.from_numpy(np.ascontiguousarray(forced_actions, np.uint8)).to(dev)
        fs = None if forced_starts is None else torch.from_numpy(np.ascontiguousarray(forced_starts, np.float64)).to(dev)
        lo, hi = support_of(kind, support)
        a = K.EVArgs(K.ptr(params), K.ptr(buf["returns"]) if "returns" in outputs else None, K.ptr(buf["lengths"]),
                     K.ptr(buf["truncated"]) if "truncated" in outputs else None, K.ptr(buf["min_gap"]) if "min_gap" in outputs else None,
                     K.ptr(buf["actions"]) if trace else None, K.ptr(fa), K.ptr(fs), seed, base, E.KIND_ID[kind], n, max_workgroups, lo, hi, 0)
        K.check(K.lib().mi_ev_episodes(C.byref(a), s.cuda_stream), "mi_ev_episodes")
    s.synchronize()
    out = {k: _np(v) for k, v in buf.items()}
    written = set(outputs) | {"lengths"} | ({"actions"} if trace else set())
    # the guard bands, and every buffer the call was not given
    assert np.isnan(out["returns"][n:]).all() and np.isnan(out["min_gap"][n:]).all()
    assert (out["lengths"][n:] == EE32).all() and (out["truncated"][n:] == 0xEE).all() and (out["actions"][n:] == 0xEE).all()
    for name in set(out) - written:
        assert (np.isnan(out[name]) if out[name].dtype == f32 else (out[name] == (EE32 if name == "lengths" else 0xEE))).all(), name
    ln = out["lengths"][:n]
    assert ((ln >= 1) & (ln <= E.LIMIT)).all()
    if "returns" in written:
        assert np.array_equal(out["returns"][:n], ln.astype(f32))
    if "truncated" in written:
        assert np.isin(out["truncated"][:n], (0, 1)).all() and (out["truncated"][:n] <= (ln == E.LIMIT)).all()
    if trace:
        for e in range(n):
            assert np.isin(out["actions"][e, :ln[e]], (0, 1)).all() and (out["actions"][e, ln[e]:] == 0xEE).all(), e
    return {k: v[:n] for k, v in out.items()}


def ev_forward(K, dev, kind, params, obs, support=None):
    obs_t = torch.from_numpy(np.ascontiguousarray(obs, f32).reshape(-1, 4)).to(dev)
    q = torch.full((obs_t.shape[0], 2), float("nan"), dtype=torch.float32, device=dev)
    lo, hi = support_of(kind, support)
    K.check(K.lib().mi_ev_forward(K.ptr(params), E.KIND_ID[kind], lo, hi, K.ptr(obs_t), obs_t.shape[0], K.ptr(q), K.stream_ptr(dev)), "mi_ev_forward")
    return _np(q)


def owner_forwards(dev, kind, params, obs, support=None):
    """-> {name: q [n][2]} of every forward call of the libraries that own `kind`, on the same device vector"""
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_c51, _native_nz, _native_pdd, _native_qr, _native_rb
    obs_t = torch.from_numpy(np.ascontiguousarray(obs, f32).reshape(-1, 4)).to(dev)
    n, s = obs_t.shape[0], N.stream_ptr(dev)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)   # noqa: E731
    out = {}
    if kind == "dueling":
        q = new(n, 2); _native_pdd.check(_native_pdd.lib().mi_pdd_forward(N.ptr(params), N.ptr(obs_t), n, N.ptr(q), s), "mi_pdd_forward"); out["mi_pdd_forward"] = _np(q)
        if params.numel() == _native_nz.NPARAMS:   # an 11,274-float vector: the noisy library's mean network
            q = new(n, 2); _native_nz.check(_native_nz.lib().mi_nz_forward(N.ptr(params), N.ptr(obs_t), n, None, N.ptr(q), s), "mi_nz_forward"); out["mi_nz_forward"] = _np(q)
    elif kind == "qr":
        q = new(n, 2); _native_qr.check(_native_qr.lib().mi_qr_forward(N.ptr(params), N.ptr(obs_t), n, None, N.ptr(q), s), "mi_qr_forward"); out["mi_qr_forward"] = _np(q)
    elif kind == "c51":
        q, p = new(n, 2), new(n, 2, 101)
        _native_c51.check(_native_c51.lib().mi_c51_forward(N.ptr(params), N.ptr(obs_t), n, N.ptr(p), N.ptr(q), s), "mi_c51_forward")
        if support is None:
            out["mi_c51_forward"] = _np(q)
        else:
            # libmirl_c51.so's support is a compile-time constant: on another support the owner's values are its own PROBABILITIES under mi_c51.h's q expression
            # (lane i: fmaf(p_{i + 64}, z_{i + 64}, p_i * z_i), then the balanced tree) with the atoms of the support asked for — float32, exact
            pr, z = _np(p), E.atoms32(support, 101)
            lanes = (pr[..., :64] * z[:64]).astype(f32)
            lanes[..., :37] = X5.fma32(pr[..., 64:], z[64:], lanes[..., :37])
            out["mi_c51_forward probs, mi_c51.h's q on this support"] = X5.tree64(lanes)
    else:
        lo, hi = support_of(kind, support)
        q = new(n, 2); _native_rb.check(_native_rb.lib().mi_rb_forward(N.ptr(params), N.ptr(obs_t), n, None, lo, hi, None, N.ptr(q), s), "mi_rb_forward"); out["mi_rb_forward"] = _np(q)
    torch.cuda.synchronize(dev)
    return out


def replay(R, kind, params, got, n, forced_starts=None, base=E.ENV_BASE, seed=E.SEED):
    """the device's own actions replayed on the oracle -> the reference's episodes under them (with the float64 values at every observation met)"""
    return E.run_episodes(R, params, kind, seed, [base + e for e in range(n)], forced_actions=got["actions"], forced_starts=forced_starts)


# ---- 1. values -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_values_equal_the_owning_forward_bit_for_bit(K, dev, kind):
    box = E.reachable_box(np.random.default_rng([7, E.KIND_ID[kind]]), 300)
    traj = np.concatenate([o["obs"] for o in E.reference_run("default", kind)] + [o["obs"] for o in E.reference_run("controller", kind)[:2]])
    obs = np.concatenate([box, traj])
    compared = 0
    for net in ("default", "controller"):
        p = params_of(dev, net, kind)
        for support in (None,) + ((E.ALT_SUPPORT,) if kind in E.DEFAULT_SUPPORT else ()):
            q = ev_forward(K, dev, kind, p, obs, support)
            assert q.shape == (len(obs), 2) and np.isfinite(q).all()
            owners = owner_forwards(dev, kind, p, obs, support)
            assert owners
            for name, qo in owners.items():
                assert np.array_equal(_bits(q), _bits(qo)), (kind, net, support, name, float(np.abs(q - qo).max()))
                compared += 1
            if net == "default":
                assert np.unique(q[:, 0]).size > 100   # no constant network
    record("values_%s" % kind, dict(observations=int(len(obs)), owner_comparisons=compared))
    # dueling: mi_pdd_forward on both and mi_nz_forward on the 11,274-float one; the categorical kinds: two supports x two networks
    assert compared == dict(dueling=3, qr=2, c51=4, rainbow=4)[kind]


# ---- 2. default-init networks, unforced, traced ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.EPISODES)
@pytest.mark.parametrize("kind", E.KINDS)
def test_default_init_episodes_replay_exactly_on_the_oracle(K, dev, R, kind, n):
    p_host, p = E.default_params(kind), params_of(dev, "default", kind)
    got = run(K, dev, kind, p, n)
    ref = replay(R, kind, p_host, got, n)
    assert [o["length"] for o in ref] == got["lengths"].tolist()
    assert [o["ret"] for o in ref] == got["returns"].tolist() and [o["truncated"] for o in ref] == got["truncated"].tolist()
    assert got["lengths"].max() < E.SHORT
    steps, smallest = 0, np.inf
    for e, o in enumerate(ref):
        q = ev_forward(K, dev, kind, p, o["obs"])
        assert np.array_equal((q[:, 1] > q[:, 0]).astype(np.uint8), got["actions"][e, :o["length"]]), (kind, e)      # every step, none left out
        gap = np.abs(q[:, 1] - q[:, 0]).astype(f32)
        assert _bits(got["min_gap"][e:e + 1])[0] == _bits(gap.min(keepdims=True))[0], (kind, e, float(got["min_gap"][e]), float(gap.min()))
        steps += o["length"]; smallest = min(smallest, float(gap.min()))
    if n == E.E_MAX:
        assert set(np.concatenate([got["actions"][e, :got["lengths"][e]] for e in range(n)]).tolist()) == {0, 1}
    record("default_%s_E%d" % (kind, n), dict(episodes=n, steps_compared=steps, smallest_gap=smallest, longest=int(got["lengths"].max())))


# ---- 3. controllers, unforced ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.EPISODES)
@pytest.mark.parametrize("kind", E.KINDS)
def test_controllers_run_into_the_limit(K, dev, R, kind, n):
    p_host, p = E.controller(kind), params_of(dev, "controller", kind)
    got = run(K, dev, kind, p, n)
    assert (got["lengths"] == 500).all() and (got["truncated"] == 1).all() and (got["returns"] == f32(500)).all()
    ref = replay(R, kind, p_host, got, n)
    assert all(o["length"] == 500 and o["truncated"] == 1 for o in ref)
    acts = np.stack([o["actions"] for o in ref]); greedy = np.stack([o["greedy"] for o in ref]); gaps = np.stack([o["gaps"] for o in ref])
    far = gaps >= E.close(kind)
    assert np.array_equal(acts[far], greedy[far])
    assert (~far).mean() <= E.MAX_EXCLUDED, (kind, n, float((~far).mean()))
    record("controller_%s_E%d" % (kind, n), dict(episodes=n, steps_compared=int(far.sum()), left_out=int((~far).sum()), smallest_gap_f64=float(gaps.min()),
                                                  smallest_gap_device=float(got["min_gap"].min()), disagreements_inside_close=int((acts != greedy).sum())))


# ---- 4. forced actions -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_forced_actions_end_where_the_oracle_ends(K, dev, kind):
    """the scripts of tests/_timelimit_cases.py on twelve env ids each: truncated at 500; the pole falling on step 498, 499 and exactly on step 500 (truncated = 0,
    length 500); short random episodes.  The same with a NaN-filled parameter vector: the episode is the actions', whatever the network holds"""
    seen = set()
    for name, _ in E.SCRIPTS:
        acts, want = E.scripts(name)
        for net in ("default", "nan"):
            got = run(K, dev, kind, params_of(dev, net, kind), E.SCRIPT_EPISODES, forced_actions=acts)
            assert got["lengths"].tolist() == [w["length"] for w in want], (kind, name, net)
            assert got["returns"].tolist() == [w["ret"] for w in want] and got["truncated"].tolist() == [w["truncated"] for w in want], (kind, name, net)
            for e, w in enumerate(want):
                assert np.array_equal(got["actions"][e, :w["length"]], acts[e, :w["length"]])
            if net == "nan":
                assert np.isposinf(got["min_gap"]).all()      # a NaN gap never enters the minimum
            else:
                assert np.isfinite(got["min_gap"]).all()      # the network is evaluated under forced actions too
        seen |= {(w["length"], w["truncated"]) for w in want}
    assert {(500, 1), (500, 0), (499, 0)} <= seen
    # unforced, a NaN network takes action 0 at every step (a NaN comparison is false) and the launch ends
    got = run(K, dev, kind, params_of(dev, "nan", kind), 5)
    assert all((got["actions"][e, :got["lengths"][e]] == 0).all() for e in range(5)) and (got["lengths"] < 20).all() and np.isposinf(got["min_gap"]).all()
    record("forced_%s" % kind, dict(endings=sorted([list(s) for s in seen if s[0] >= 490])))


# ---- 5. forced starts ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_forced_starts(K, dev, R, kind):
    """a start one step from the x threshold and moving out: length 1; a start on which the controller never drops the pole: 500"""
    starts = np.array([[2.39, 1.0, 0.0, 0.0], [0.0, 0.0, 0.01, 0.0], [-2.39, -1.0, 0.0, 0.0]])
    got = run(K, dev, kind, params_of(dev, "controller", kind), 3, forced_starts=starts)
    assert got["lengths"].tolist() == [1, 500, 1] and got["truncated"].tolist() == [0, 1, 0] and got["returns"].tolist() == [1.0, 500.0, 1.0]
    ref = replay(R, kind, E.controller(kind), got, 3, forced_starts=starts)
    assert [o["length"] for o in ref] == [1, 500, 1] and [o["truncated"] for o in ref] == [0, 1, 0]
    with E.T._Mode(R):
        s, term = R.cartpole_step(starts[0], int(got["actions"][0, 0]))
    assert term and s[0] > 2.4
    # the starts are read as given: the first observation is their float32 rounding
    q = ev_forward(K, dev, kind, params_of(dev, "controller", kind), starts.astype(f32))
    assert np.array_equal((q[:, 1] > q[:, 0]).astype(np.uint8), got["actions"][:, 0])


# ---- 6. independence -------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, n=None):
    for k in ("returns", "lengths", "truncated", "min_gap", "actions"):
        x, y = a[k][:n], b[k][:n]
        assert np.array_equal(x.view(np.uint32) if x.dtype == f32 else x, y.view(np.uint32) if y.dtype == f32 else y), k


@pytest.mark.parametrize("kind", E.KINDS)
def test_results_do_not_depend_on_the_grid_the_count_or_the_neighbours(K, dev, kind):
    other = E.KINDS[(E.KINDS.index(kind) + 1) % len(E.KINDS)]
    for net in ("default", "controller"):
        p = params_of(dev, net, kind)
        base = run(K, dev, kind, p, E.E_MAX)
        for g in (1, 2, 3):
            _same(base, run(K, dev, kind, p, E.E_MAX, max_workgroups=g))
        _same(base, run(K, dev, kind, p, 5), 5)              # E = 5 is the prefix of E = 37
        _same(base, run(K, dev, kind, p, 1), 1)
        _same(base, run(K, dev, kind, p, E.E_MAX))           # a second call: nothing is carried
    # two kinds on two streams at once
    alone = {k: run(K, dev, k, params_of(dev, "controller", k), E.E_MAX) for k in (kind, other)}
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    from deep_rl_amd import evaluate as EV
    nets = {}
    for k in (kind, other):   # through evaluate(): bare networks of the project's classes holding the controller's parameters
        import deep_rl_amd as D
        env = D.make("CartPole-v1", num_envs=1, device=dev)
        cls = E.network_class(k) if k != "dueling" else D.DuelingQNetwork
        nets[k] = cls(env)
        nets[k].flat[:E.NREAD[k]].copy_(params_of(dev, "controller", k)[:E.NREAD[k]])
    torch.cuda.synchronize(dev)
    r1 = EV.evaluate(nets[kind], E.E_MAX, seed=E.SEED, trace=True, stream=s1)
    r2 = EV.evaluate(nets[other], E.E_MAX, seed=E.SEED, trace=True, stream=s2)
    torch.cuda.synchronize(dev)
    for k, r in ((kind, r1), (other, r2)):
        got = dict(returns=_np(r.returns), lengths=_np(r.lengths), truncated=_np(r.truncated), min_gap=_np(r.min_gap))
        for name, v in got.items():
            assert np.array_equal(v.view(np.uint32) if v.dtype == f32 else v, alone[k][name].view(np.uint32) if v.dtype == f32 else alone[k][name]), (k, name)
        ln = got["lengths"]
        assert all(np.array_equal(_np(r.actions)[e, :ln[e]], alone[k]["actions"][e, :ln[e]]) for e in range(E.E_MAX))


# ---- 7. training is undisturbed --------------------------------------------------------------------------------------------------------------------------
def make_engine(dev, name, n_envs=4, slots=64, seed=3, **kw):
    """an engine of class `name` as its script builds it, small"""
    import deep_rl_amd as D
    from deep_rl_amd.evaluate import ENGINES_EVALUABLE
    env = D.make("CartPole-v1", num_envs=n_envs, device=dev, seed=seed, env_id_base=100)
    torch.manual_seed(seed)
    cls = getattr(D, ENGINES_EVALUABLE[name])
    q, tq = cls(env), cls(env)
    tq.load_state_dict(q.state_dict())
    opt = D.ClipAdam(q, lr=2.5e-4, eps=1e-8) if name == "DuelingDQNEngine" else D.Adam(q, lr=2.5e-4)
    if name not in ("C51Engine", "QRDQNEngine"):
        kw.setdefault("learning_starts", 0)
    return getattr(D, name)(env, q, tq, opt, slots=slots, batch_size=32, max_episodes_logged=256, **kw)


def _train(dev, name, with_eval, **kw):
    import deep_rl_amd as D
    from deep_rl_amd import checkpoint
    eng = make_engine(dev, name, **kw)
    eng.reset()
    log, evals = [], []
    for _ in range(3):
        eng.act(16)
        log.append(eng.drain_episodes())
        if with_eval:
            evals.append(D.evaluate(eng, 5))
    for _ in range(3):
        eng.train_step()
        if with_eval:
            evals.append(D.evaluate(eng, 5))
    eng.act(16)
    log.append(eng.drain_episodes())
    torch.cuda.synchronize(dev)
    return checkpoint.state_dict(eng), log, evals, eng


@pytest.mark.parametrize("name,kw", [("PDDDQNEngine", dict(prioritized=True)), ("RainbowEngine", dict(prioritized=True)), ("QRDQNEngine", {}), ("C51Engine", {})])
def test_training_is_undisturbed_by_evaluation(dev, name, kw):
    """3 acting chunks and 3 updates with evaluate(engine, 5) after each, against the same run without, for an engine of every kind: ring, parameters, target, moments, priorities, env state,
    counters and the episode log are equal bit for bit (checkpoint.state_dict holds all of them)"""
    # (DoubleDQNEngine is not among them: the plain QNetwork has no kind, include/mi_eval.h; QR-DQN and C51 stand beside the two prioritized engines)
    a, log_a, evals, eng = _train(dev, name, True, **kw)
    b, log_b, _none, _ = _train(dev, name, False, **kw)
    assert set(a) == set(b) and {"params", "target", "env_blob", "observation", "observations", "actions", "opt_exp_avg", "opt_exp_avg_sq"} <= set(a)
    if kw.get("prioritized"):
        assert "priorities" in a and "max_priority" in a
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    assert log_a == log_b
    assert len(evals) == 6 and all(r.episodes == 5 and 1 <= r.min <= r.max <= 500 for r in evals)
    assert not np.array_equal(_np(evals[2].min_gap), _np(evals[5].min_gap))   # the parameters moved between them: the evaluation read the live vector
    record("undisturbed_%s" % name, dict(keys=len(a), evaluations=len(evals), mean_returns=[r.mean for r in evals]))


# ---- 8. poison -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_poisoned_outputs_and_nullable_buffers(K, dev, kind):
    """run() pre-fills every buffer (NaN / 0xEE) and checks the guard bands and the buffers the call was not given after EVERY launch of this file; here each
    nullable output is left out in turn and the rest must not change"""
    p = params_of(dev, "default", kind)
    full = run(K, dev, kind, p, 5)
    assert not np.isnan(full["returns"]).any() and not np.isnan(full["min_gap"]).any()
    for outputs, trace in ((("returns", "truncated", "min_gap"), False), (("truncated", "min_gap"), True), (("returns", "min_gap"), True), (("returns", "truncated"), True), ((), False)):
        got = run(K, dev, kind, p, 5, trace=trace, outputs=outputs)
        assert np.array_equal(got["lengths"], full["lengths"])
        for name in outputs:
            assert np.array_equal(_bits(got[name]) if got[name].dtype == f32 else got[name], _bits(full[name]) if full[name].dtype == f32 else full[name]), name


# ---- 9. evaluate() and the CLI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_evaluate_statistics_equal_numpys(K, dev, kind):
    import deep_rl_amd as D
    env = D.make("CartPole-v1", num_envs=1, device=dev)
    net = (E.network_class(kind) if kind != "dueling" else D.DuelingQNetwork)(env)
    net.flat[:E.NREAD[kind]].copy_(params_of(dev, "default", kind)[:E.NREAD[kind]])
    before = net.flat.clone()
    res = D.evaluate(net, E.E_MAX, seed=E.SEED, trace=True)
    assert isinstance(res, D.EvalResult) and res.source_id == K.source_id() and res.episodes == E.E_MAX
    assert torch.equal(net.flat, before)
    direct = run(K, dev, kind, params_of(dev, "default", kind), E.E_MAX)
    r, tr = _np(res.returns).astype(np.float64), _np(res.truncated).astype(np.float64)
    assert np.array_equal(_np(res.returns), direct["returns"]) and np.array_equal(_np(res.lengths), direct["lengths"]) and np.array_equal(_bits(_np(res.min_gap)), _bits(direct["min_gap"]))
    assert res.returns.dtype == torch.float32 and res.lengths.dtype == torch.int32 and res.truncated.dtype == torch.uint8 and res.actions.shape == (E.E_MAX, 500)
    assert res.mean == np.mean(r) and res.min == np.min(r) and res.max == np.max(r) and res.truncated_fraction == np.mean(tr)
    # the returns are whole numbers, so n * sum r^2 - (sum r)^2 is exact in float64: numpy gives the same two roundings
    n = float(len(r))
    assert res.std == np.sqrt((n * np.sum(r * r) - np.sum(r) ** 2) / (n * n))
    assert D.evaluate(net, 3, trace=False).actions is None
    # evaluate.forward: mi_ev_forward on the network's own vector
    from deep_rl_amd.evaluate import forward
    obs = E.reachable_box(np.random.default_rng(5), 33)
    assert np.array_equal(_bits(_np(forward(net, torch.from_numpy(obs)))), _bits(ev_forward(K, dev, kind, params_of(dev, "default", kind), obs)))
    # the default env ids are disjoint from a training env's: another base gives other episodes, the same base the same
    assert not np.array_equal(_np(D.evaluate(net, E.E_MAX, env_id_base=0).min_gap), _np(res.min_gap))
    with pytest.raises(K.MiError):
        D.evaluate(net, 0)
    with pytest.raises(K.MiError):
        D.evaluate(net, 3, forced_actions=torch.zeros((2, 500), dtype=torch.uint8, device=dev))


def test_cli_prints_what_evaluate_returns(dev, tmp_path):
    """a checkpoint of each supported engine class, evaluated through the CLI in ONE fresh child process (a line per checkpoint), against evaluate(engine)"""
    import deep_rl_amd as D
    from deep_rl_amd import checkpoint
    from deep_rl_amd.evaluate import ENGINES_EVALUABLE
    paths, want = [], []
    for name in sorted(ENGINES_EVALUABLE):
        eng = make_engine(dev, name, n_envs=2, slots=16)
        eng.reset()
        eng.act(8)
        paths.append(checkpoint.save(str(tmp_path / name), eng, include_replay=False))
        want.append(D.evaluate(eng, 7, seed=3).line())
    torch.cuda.synchronize(dev)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "deep_rl_amd.evaluate"] + paths + ["--episodes", "7", "--seed", "3"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("episodes=")]
    assert lines == want, (lines, want)
    assert len(lines) == 7 and all(ln.split()[0] == "episodes=7" and [f.split("=")[0] for f in ln.split()] == ["episodes", "mean_return", "std", "min", "max", "truncated"] for ln in lines)
    # the three engines on a DuelingQNetwork were built under one torch seed: the same parameters, hence the same line (nothing says the other classes' lines differ)
    by_name = dict(zip(sorted(ENGINES_EVALUABLE), lines))
    assert by_name["DuelingDQNEngine"] == by_name["PDDDQNEngine"] == by_name["NStepDQNEngine"]
    record("cli", dict(checkpoints=len(lines), lines=lines))
