"""The kernels of libmirl_pg.so (deep_rl_amd/csrc/mi_reinforce.hip) on synthetic inputs, against float64 — what tests/test_gpu_reinforce.py cannot reach because
it drives them through real CartPole episodes under trained or freshly initialised parameters: every tail of the slab sum and the grid stride of the gradient
kernel (one-hot env probe, by value), the gradient at env counts / episode lengths / parameter scales nobody picked, the returns kernel at the lane-ownership
boundaries of its rows and at other gammas, forward and log-probs under saturated softmax and degenerate masks, the keyed RNG streams past the first episode
(step counters off the 4-step block boundary, high key / counter words in use) and mi_pg_adam away from n = 898 and the default hyper-parameters.

Every input comes from tests/_reinforce_cases.py; tests/test_reinforce_cases_cpu.py validates those inputs without a GPU and measures the tolerances: a device
bound is 8 x the error of the f32 numpy restatement against float64 on the same inputs (K.*_REST).  MIRL_FUZZ_CASES (default 4) and MIRL_FUZZ_SEED (default 1)
choose the cases as in tests/test_gpu_fuzz.py; a failing assert names the case's shape.  Observed maxima go to reinforce_gpu_maxima.json (docs/LEDGER.md)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _reinforce_cases as K      # noqa: E402
import _reinforce_ref as P        # noqa: E402
import test_gpu_reinforce as T    # noqa: E402  (_make, _np, _record, LP_BOUND)
from oracle import cpu_ref as R   # noqa: E402
from test_gpu_fuzz import _log   # noqa: E402  (a line per passed case, in the fuzz families' file)

F = K.DEVICE_FACTOR
_make, _np, _record = T._make, T._np, T._record


@pytest.fixture(scope="module", autouse=True)
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int32))


def _poison_storage(eng):
    eng.observations.fill_(float("nan")); eng.b_returns.fill_(float("nan")); eng.actions.fill_(K.POISON_ACTION); eng.mask_bits.fill_(-1)


def _poisoned_grad(eng):
    eng.workspace.fill_(0xFF)       # every slab NaN: a slab that is summed without having been written shows
    eng.grad()
    return _np(eng.grads).copy()


# ---- 1. slab sum and grid stride: one-hot env probe ------------------------------------------------------------
def _load_probe(eng, k, ep):
    dev = eng.device
    n = K.PROBE_LEN
    eng.observations[k, :n] = torch.from_numpy(ep["X"]).to(dev); eng.actions[k, :n] = torch.from_numpy(ep["A"]).to(dev)
    eng.mask_bits[k, :n] = _words(ep["W"]).to(dev); eng.b_returns[k, :n] = torch.from_numpy(ep["Rn"]).to(dev)
    eng.lengths[k] = n


@pytest.fixture(scope="module")
def probe():
    """the probe episode and its gradient from an N = 1 engine (one slab), itself checked against float64"""
    ep = K.probe_episode()
    eng = _make(1, params=ep["params"])
    _poison_storage(eng)
    _load_probe(eng, 0, ep)
    g = _poisoned_grad(eng)
    g64 = P.grad(ep["params"], ep["X"], ep["A"], ep["M"], ep["Rn"], np.float64)
    err = float(np.abs(g - g64).max() / np.abs(g64).max())
    _record("kernels_probe_n1", {"grad_err_of_max": err, "bound": F * K.GRAD_REST})
    assert np.isfinite(g).all() and err <= F * K.GRAD_REST, err
    return ep, g


@pytest.mark.parametrize("n", K.PROBE_NS)
def test_pg_grad_one_hot_env_probe(probe, n):
    """all lengths 0 but env k's: the sum over min(n, 1024) slabs must be the one slab that is not zero — by value (adding zero slabs is exact; +0 + -0 may turn a
    sign bit, so no bit views).  n = 49 / 33 / 81 reach the s2 / s1 tails of pg_reduce_kernel, n > 1024 gives workgroups a second env."""
    ep, want = probe
    eng = _make(n, params=ep["params"])
    _poison_storage(eng)
    for k in K.probe_envs(n):
        eng.lengths.zero_()
        _load_probe(eng, k, ep)
        got = _poisoned_grad(eng)
        bad = np.flatnonzero(~(got == want))
        assert np.array_equal(got, want), "pg probe: envs %d, the episode in env %d: %d of 898 elements differ, first %d: %r against %r" % (
            n, k, len(bad), bad[0], got[bad[0]], want[bad[0]])
    _log("pg probe: envs %d, probed %s ok" % (n, K.probe_envs(n)))


# ---- 2. gradient at any shape ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(K.CASES))
def test_pg_grad_any_shape(case):
    c = K.grad_case(case)
    shape = c["shape"]
    eng = _make(c["n"], params=c["params"])
    dev = eng.device
    eng.observations.copy_(torch.from_numpy(c["obs"]).to(dev)); eng.actions.copy_(torch.from_numpy(c["act"]).to(dev))
    eng.mask_bits.copy_(_words(c["words"]).to(dev)); eng.b_returns.copy_(torch.from_numpy(c["brn"]).to(dev))
    eng.log_probs.fill_(float("inf")); eng.lengths.copy_(torch.from_numpy(c["lengths"]).to(dev))
    g = _poisoned_grad(eng)
    g64 = P.grad(c["params"], c["X"], c["A"], c["M"], c["Rn"], np.float64)
    assert np.isfinite(g).all(), shape
    err = float(np.abs(g - g64).max() / np.abs(g64).max())
    print(shape, "grad err of max |g| %.3g (bound %.3g)" % (err, F * K.GRAD_REST))
    _record("kernels_grad_case%d" % case, {"shape": shape, "grad_err_of_max": err, "bound": F * K.GRAD_REST})
    assert err <= F * K.GRAD_REST, "%s: %.3g of max |g|" % (shape, err)
    again = _poisoned_grad(eng)
    assert np.array_equal(again.view(np.uint32), g.view(np.uint32)), shape + ": a second grad() gives other bits"
    _log(shape + " ok")


# ---- 3. returns kernel ---------------------------------------------------------------------------------------------
_ret64 = {}


def _returns64(L, gamma):
    if (L, gamma) not in _ret64:
        _ret64[(L, gamma)] = P.returns_normalised64(L, gamma)
    return _ret64[(L, gamma)]


@pytest.mark.parametrize("n", K.RETURNS_NS)
def test_pg_returns_chosen_lengths_and_gammas(n):
    eng = _make(n)
    raw = norm = 0.0
    for gamma in K.GAMMAS:
        eng.gamma = gamma
        for lens in K.returns_launches(n):
            shape = "pg returns: envs %d, gamma %g, lengths %s" % (n, gamma, lens.tolist())
            eng.lengths.copy_(torch.from_numpy(lens).to(eng.device))
            eng.returns.fill_(float("nan")); eng.b_returns.fill_(float("nan"))
            eng.compute_returns()
            Rd, Nd = _np(eng.returns), _np(eng.b_returns)
            for e, L in enumerate(int(x) for x in lens):
                R64, N64 = _returns64(L, gamma)
                assert np.all(Rd[e, L:] == 0) and np.all(Nd[e, L:] == 0), shape + ": rows behind the end of env %d are not 0" % e
                er, en = float((np.abs(Rd[e, :L] - R64) / np.abs(R64)).max()), float(np.abs(Nd[e, :L] - N64).max())
                assert er <= F * K.RETURNS_RAW_REST, "%s: env %d raw returns %.3g of the value" % (shape, e, er)
                assert en <= F * K.RETURNS_NORM_REST, "%s: env %d normalised returns %.3g absolute" % (shape, e, en)
                if gamma == 0.0:
                    assert np.all(Rd[e, :L] == 1) and np.all(Nd[e, :L] == 0), shape + ": gamma 0 gives R = 1 and exactly 0 after normalisation"
                raw, norm = max(raw, er), max(norm, en)
    _record("kernels_returns_n%d" % n, {"raw_rel_err": raw, "raw_bound": F * K.RETURNS_RAW_REST, "normalised_abs_err": norm, "normalised_bound": F * K.RETURNS_NORM_REST})
    _log("pg returns: envs %d, %d lengths x %d gammas ok" % (n, len(K.RETURNS_LENGTHS), len(K.GAMMAS)))


def test_pg_returns_edge_lengths():
    """len 1: R = 1 and NaN after normalisation (include/mi_reinforce.h); len 0 and below: every row 0, no NaN; above 500: as 500"""
    lens = np.array(K.RETURNS_EDGE_LENGTHS, np.int32)
    assert lens.tolist() == [1, 0, -3, 501, 10 ** 6, 500, 2]
    eng = _make(len(lens))
    eng.lengths.copy_(torch.from_numpy(lens).to(eng.device))
    eng.returns.fill_(float("nan")); eng.b_returns.fill_(float("nan"))
    eng.compute_returns()
    Rd, Nd = _np(eng.returns), _np(eng.b_returns)
    assert Rd[0, 0] == 1 and np.isnan(Nd[0, 0]) and np.all(Rd[0, 1:] == 0) and np.all(Nd[0, 1:] == 0)
    for e in (1, 2):
        assert np.all(Rd[e] == 0) and np.all(Nd[e] == 0), "len %d" % lens[e]
    R64, N64 = _returns64(500, 0.99)
    assert float((np.abs(Rd[5, :500] - R64) / R64).max()) <= F * K.RETURNS_RAW_REST and float(np.abs(Nd[5, :500] - N64).max()) <= F * K.RETURNS_NORM_REST
    for e in (3, 4):
        assert np.array_equal(Rd[e].view(np.uint32), Rd[5].view(np.uint32)) and np.array_equal(Nd[e].view(np.uint32), Nd[5].view(np.uint32)), "len %d" % lens[e]
        assert Rd[e, 500] == 0 and Nd[e, 500] == 0
    R2, N2 = _returns64(2, 0.99)
    assert np.all(np.abs(Rd[6, :2] - R2) / R2 <= F * K.RETURNS_RAW_REST) and np.all(np.abs(Nd[6, :2] - N2) <= F * K.RETURNS_NORM_REST) and np.all(Rd[6, 2:] == 0)
    assert int(np.isnan(Rd).sum()) == 0 and int(np.isnan(Nd).sum()) == 1
    # the gradient kernel clamps the same way: nothing behind row 500 or in front of row 0 is read, an empty env adds nothing
    _poison_storage(eng)
    eng.b_returns[:, :500] = 0.0; eng.observations[:, :500] = 0.25; eng.actions[:, :500] = 1; eng.mask_bits[:, :500] = 0x55555555
    g = _poisoned_grad(eng)
    assert np.isfinite(g).all() and np.all(g == 0)


# ---- 4. forward and log-probs at extreme parameters ----------------------------------------------------------------
def test_pg_forward_extreme_parameters_and_masks():
    agent = _make(1).agent
    worst = {}
    for name, params in K.forward_param_sets():
        agent.load_flat(params)
        b2 = params[896:898].astype(np.float64)
        soft_b2 = np.exp(b2 - b2.max()) / np.exp(b2 - b2.max()).sum()
        w = 0.0
        for n in K.FORWARD_NS:
            for i, (X, M) in enumerate(K.forward_launches(n)):
                shape = "pg forward: %s, rows %d, launch %d" % (name, n, i)
                for mode, Mm in (("masks", M), ("eval", None)):
                    p = _np(agent.forward(torch.from_numpy(X), None if Mm is None else _words(P.mask_words(Mm))))
                    p64 = P.forward64(params, X, Mm)[0]
                    assert p.shape == (n, 2) and np.isfinite(p).all(), shape + " " + mode
                    err = float(np.abs(p - p64).max())
                    w = max(w, err)
                    assert err <= F * K.PROBS_REST, "%s %s: probabilities %.3g absolute" % (shape, mode, err)
                    assert float(np.abs(p.astype(np.float64).sum(1) - 1).max()) <= 1e-6, shape + " " + mode
                    if name.startswith("gap"):
                        assert np.all(np.sort(p, axis=1) == [0, 1]), shape + " " + mode + ": saturated softmax is exactly (0, 1)"
                dropped = np.flatnonzero(M.sum(1) == 0)
                p = _np(agent.forward(torch.from_numpy(X), _words(P.mask_words(M))))
                assert float(np.abs(p[dropped] - soft_b2).max(initial=0.0)) <= F * K.PROBS_REST, shape + ": all units dropped, p is not softmax(b2)"
        worst[name] = w
    _record("kernels_forward", {"probs_abs_err": worst, "bound": F * K.PROBS_REST})


def test_pg_log_probs_teacher_forced_extreme_parameters():
    worst = {}
    for r in K.log_prob_rollouts():
        eng = _make(3, params=r["params"])
        eng.rollout(torch.from_numpy(r["resets"]), torch.from_numpy(r["actions"]), _words(r["words"]))
        lens = _np(eng.lengths)
        shape = "pg log-probs: %s, lengths %s" % (r["name"], r["lengths"].tolist())
        assert np.array_equal(lens, r["lengths"]), shape + ": device lengths %s" % lens.tolist()
        w, lowest = 0.0, 0.0
        for e, (X, A, M) in enumerate(r["rows"]):
            L = int(lens[e])
            obs, mb, lp = _np(eng.observations[e, :L]), _np(eng.mask_bits[e, :L]), _np(eng.log_probs[e])
            assert np.array_equal(obs, X) and np.array_equal(P.words_to_masks(mb), M) and np.array_equal(_np(eng.actions[e, :L]), A), shape
            _p64, lp64, L64, _Z = P.forward64(r["params"], obs, P.words_to_masks(mb))
            assert np.isfinite(lp[:L]).all() and np.all(lp[L:] == 0), shape + ": env %d" % e
            err = float((np.abs(lp[:L] - lp64[np.arange(L), A]) / np.maximum(1.0, np.abs(L64).max(axis=1))).max())
            assert err <= F * K.LOG_PROBS_REST, "%s: env %d log-probs %.3g of max(1, |l0|, |l1|)" % (shape, e, err)
            w, lowest = max(w, err), min(lowest, float(lp[:L].min()))
        if r["name"].startswith("gap"):
            assert lowest < -100, shape + ": a forced action of probability 0 has log-prob %g" % lowest        # finite (above), large and negative
        worst[r["name"]] = {"log_prob_err": w, "lowest_log_prob": lowest}
    _record("kernels_log_probs", {"rollouts": worst, "bound": F * K.LOG_PROBS_REST})


# ---- 5. RNG continuation ---------------------------------------------------------------------------------------------
def test_pg_rng_continues_over_three_episodes():
    """seed 2**33 + 11 and env_id_base 2**32 + 7 (mi_env_create takes both as they are: 64-bit).  Episode j of env e starts at step counter c0 = the sum of its
    earlier lengths — mostly off the 4-step boundary of the action uniforms' Philox block — and at episode counter j."""
    n, seed, base = K.RNG_N, K.RNG_SEED, K.RNG_BASE
    params = K.rng_params()
    eng = _make(n, seed=seed, env_id_base=base, params=params)
    eps = []
    for j in range(K.RNG_EPISODES):
        eng.rollout()
        lens = _np(eng.lengths).copy()
        eps.append((lens, [(_np(eng.observations[e, :lens[e] + 1]).copy(), _np(eng.actions[e, :lens[e]]).astype(np.int64), _np(eng.mask_bits[e, :lens[e]]).copy())
                           for e in range(n)]))
    lengths = np.array([l for l, _ in eps]).T                       # (env, episode)
    c0 = K.start_counters(lengths)
    assert lengths.min() >= 1 and lengths.max() <= 500
    assert {1, 2, 3} <= {int(x) for x in (c0 % 4).ravel()}, "choose another seed: start counters mod 4 are %s" % (c0 % 4).tolist()
    boundary = rows = 0
    R.set_sincos_mode("fdlibm")
    try:
        for j, (lens, envs) in enumerate(eps):
            for e, (obs, A, W) in enumerate(envs):
                E, L = base + e, int(lens[e])
                ctrs = int(c0[e, j]) + np.arange(L)
                shape = "pg rng: env %d (id %d), episode %d, length %d, first step counter %d" % (e, E, j, L, c0[e, j])
                assert np.array_equal(P.words_to_masks(W), P.keyed_masks(seed, E, ctrs)), shape + ": masks"
                s0 = R.reset_noise(seed, E, j)
                assert np.array_equal(obs[0], s0.astype(np.float32)), shape + ": reset noise"
                p0 = _np(eng.agent.forward(torch.from_numpy(obs[:L]), torch.from_numpy(W)))[:, 0]
                u = P.action_uniforms(seed, E, ctrs)
                differ = (u >= p0).astype(np.int64) != A
                assert np.all(np.abs(u[differ] - p0[differ]) <= T.LP_BOUND), shape + ": an action differs from the draw away from the boundary"
                boundary += int(differ.sum()); rows += L
                o_obs, _t, o_done, _tr = P.replay_episode(s0, A)
                assert len(o_obs) == L and o_done[-1], shape + ": oracle length %d" % len(o_obs)
                assert np.array_equal(obs[1:], o_obs), shape + ": observations"
    finally:
        R.set_sincos_mode("libm")
    _record("kernels_rng_continuation", {"lengths": lengths.tolist(), "start_counters_mod4": (c0 % 4).tolist(), "rows": rows, "boundary_actions": boundary})


# ---- 6. Adam ---------------------------------------------------------------------------------------------------------
def test_pg_adam_any_size_step_and_hyperparameters(dev):
    from deep_rl_amd import _native as N
    from deep_rl_amd import _native_pg as PG

    worst = 0.0
    for c in K.adam_cases():
        n, (lr, b1, b2, eps) = c["n"], c["hp"]
        p, g, m, v = [torch.from_numpy(c[k].copy()).to(dev) for k in "pgmv"]
        PG.check(PG.lib().mi_pg_adam(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, c["step"], lr, b1, b2, eps, N.stream_ptr(dev)), "mi_pg_adam")
        p64, m64, v64 = [c[k][:n].astype(np.float64) for k in "pmv"]
        P.adam_step64(p64, c["g"][:n], m64, v64, c["step"], lr, b1, b2, eps)
        pd = _np(p)
        for k, t in zip("pgmv", (p, g, m, v)):
            assert np.array_equal(_np(t)[n:].view(np.uint32), c[k][n:].view(np.uint32)), c["shape"] + ": %s is written behind n" % k
        assert np.array_equal(_np(g).view(np.uint32), c["g"].view(np.uint32)) and np.isfinite(pd).all(), c["shape"]
        err = float((np.abs(pd[:n] - p64) / np.maximum(np.abs(p64), lr)).max())
        assert err <= F * K.ADAM_REST, "%s: %.3g of max(|p|, lr)" % (c["shape"], err)
        worst = max(worst, err)
    _record("kernels_adam", {"param_err_of_max_p_lr": worst, "bound": F * K.ADAM_REST})
