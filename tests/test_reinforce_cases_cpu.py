"""The inputs of tests/test_gpu_reinforce_kernels.py (tests/_reinforce_cases.py) checked without a GPU: that they reach the paths they are meant to reach, that
the ReLU-kink rule switches off at most 1 % of a case's rows (float64 alone), that the RNG-continuation seed is predicted to start episodes at every residue of
the step counter mod 4, and — the tolerances — that the f32 numpy restatement stays at or below each *_REST constant against float64 on every case list.  The
GPU tests allow the device 8 x those constants.  Every figure is printed before it is asserted (`pytest -s`)."""
import numpy as np
import pytest

import _reinforce_cases as K
import _reinforce_ref as P

f32 = np.float32


@pytest.fixture(autouse=True, scope="module")
def _default_seed():
    """the constants were measured at the default seed and case count, whatever the environment asks of the GPU run"""
    seed, cases = K.SEED, K.CASES
    K.SEED, K.CASES = 1, 4
    yield
    K.SEED, K.CASES = seed, cases


def test_probe_covers_every_tail_of_the_slab_sum():
    """pg_reduce_kernel: groups of 16 slabs on four accumulators; the tails s0 / s1 / s2 run for n_slabs mod 64 in 1-16 / 17-32 / 33-48"""
    tails = {(min(n, 1024) % 64 + 15) // 16 for n in K.PROBE_NS}
    assert {1, 2, 3, 4} <= tails                              # 2 and 3: the s1 and s2 tails
    assert any(n > 1024 for n in K.PROBE_NS)                  # a workgroup with two envs
    for n in K.PROBE_NS:
        ks = K.probe_envs(n)
        assert ks[0] == 0 and ks[-1] == n - 1 and all(0 <= k < n for k in ks)
        if n > 1024:
            assert {1023, 1024} <= set(ks)
    ep = K.probe_episode()
    g = P.grad(ep["params"], ep["X"], ep["A"], ep["M"], ep["Rn"], np.float64)
    assert len(ep["A"]) == K.PROBE_LEN and np.isfinite(g).all() and (g != 0).sum() > 400      # a dropped slab cannot hide behind a zero gradient


@pytest.fixture(scope="module")
def grad_cases():
    return [K.grad_case(c) for c in range(K.CASES)]


def test_grad_cases_shapes_poison_and_kink_cap(grad_cases):
    buckets, residues, sigmas = set(), set(), set()
    for c in grad_cases:
        n, L = c["n"], c["lengths"]
        print(c["shape"])
        buckets.add([lo <= n < hi for lo, hi in K.N_BUCKETS].index(True))
        residues |= {int(x) % 8 for x in L if 0 < x < 25}
        sigmas.add(c["sigma"])
        rows = int(L.sum())
        assert 0 < rows <= 25000 and n <= 1100, c["shape"]
        assert int((L > 24).sum()) <= 2 and all(493 <= x <= 500 for x in L[L > 24]), c["shape"]
        assert int(c["kink"].sum()) <= K.KINK_SHARE * rows, c["shape"]                 # float64 alone
        assert np.all(c["Rn"][c["kink"]] == 0)
        if rows >= 2:
            assert (c["M"].sum(1) == 0).any() and (c["M"].sum(1) == 128).any(), c["shape"]
        for e in range(n):
            assert np.isnan(c["obs"][e, L[e]:]).all() and np.isnan(c["brn"][e, L[e]:]).all() and np.all(c["act"][e, L[e]:] == K.POISON_ACTION)
            assert np.all(c["words"][e, L[e]:] == K.POISON_WORD) and np.isfinite(c["obs"][e, :L[e]]).all() and np.isfinite(c["brn"][e, :L[e]]).all()
        assert np.array_equal(P.words_to_masks(np.concatenate([c["words"][e, :L[e]] for e in range(n)])), c["M"])
    if K.CASES >= 4:
        assert buckets == {0, 1, 2, 3} and residues == set(range(8)), (buckets, residues)


def test_grad_restatement_error(grad_cases):
    worst = 0.0
    for c in grad_cases:
        g64 = P.grad(c["params"], c["X"], c["A"], c["M"], c["Rn"], np.float64)
        g32 = P.grad(c["params"], c["X"], c["A"], c["M"], c["Rn"]).astype(np.float64)
        err = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        print("%s: f32 restatement %.3g of max |g|" % (c["shape"], err))
        worst = max(worst, err)
    print("GRAD_REST measured", worst)
    assert worst <= K.GRAD_REST


def test_returns_cases_and_restatement_error():
    for n in K.RETURNS_NS:
        launches = K.returns_launches(n)
        assert all(len(v) == n for v in launches) and set(K.RETURNS_LENGTHS) <= {int(x) for v in launches for x in v}
    raw = norm = 0.0
    at = None
    for g in K.GAMMAS:
        for L in K.RETURNS_LENGTHS:
            R32, N32 = P.returns_normalised(L, g)
            R64, N64 = P.returns_normalised64(L, g)
            raw = max(raw, float((np.abs(R32 - R64) / np.abs(R64)).max()))
            e = float(np.abs(N32 - N64).max())
            if e > norm:
                norm, at = e, (g, L)
            if g == 0.0:
                assert np.all(R32 == 1) and np.all(N32 == 0) and np.all(N64 == 0)       # variance 0: the denominator is exp(-5)
    print("RETURNS_RAW_REST measured", raw, " RETURNS_NORM_REST measured", norm, "at (gamma, len)", at)
    assert raw <= K.RETURNS_RAW_REST and norm <= K.RETURNS_NORM_REST
    R1, N1 = P.returns_normalised64(1)
    assert R1[0] == 1 and np.isnan(N1[0]) and np.isnan(P.returns_normalised(1)[1][0])


def test_forward_cases_and_restatement_error():
    sets = K.forward_param_sets()
    special = K.one_bit_masks()
    assert len(special) == 10 and special[0].sum() == 0 and special[1].sum() == 128 and all(m.sum() == 1 for m in special[2:])
    worst, worst_eval, sat = 0.0, 0.0, 0
    for n in K.FORWARD_NS:
        launches = K.forward_launches(n)
        seen = {tuple(np.flatnonzero(m)) for _X, M in launches for m in M}
        assert {tuple(np.flatnonzero(m)) for m in special} <= seen, n                   # every special mask row passes at every n
        for name, params in sets:
            for X, M in launches:
                p32 = P.forward(params, X, M)[0]
                p64, _lp, L64, _Z = P.forward64(params, X, M)
                worst = max(worst, float(np.abs(p32 - p64).max()))
                worst_eval = max(worst_eval, float(np.abs(P.forward(params, X, None)[0] - P.forward64(params, X, None)[0]).max()))
                assert np.isfinite(p32).all()
                if name.startswith("gap"):
                    assert np.all(np.abs(L64[:, 0] - L64[:, 1]) > 100), name
                    assert np.all(np.sort(p32, axis=1) == [0, 1])
                    sat += len(X)
    assert sat > 0
    print("PROBS_REST measured: masked", worst, "eval", worst_eval)
    assert max(worst, worst_eval) <= K.PROBS_REST


def _log_prob_error(lp, lp64, L64, A):
    i = np.arange(len(A))
    return np.abs(lp[i, A] - lp64[i, A]) / np.maximum(1.0, np.abs(L64).max(axis=1))


def test_log_prob_rollouts_and_restatement_error():
    worst = 0.0
    ros = K.log_prob_rollouts()
    assert [r["name"] for r in ros] == ["sigma3", "gap+"]
    lens = np.concatenate([r["lengths"] for r in ros])
    assert lens.max() == 500 and lens.min() < 20, lens
    for r in ros:
        zero_prob = 0
        for X, A, M in r["rows"]:
            assert M[0].sum() == 0 and (len(A) < 2 or M[1].sum() == 128)
            _p, lp32, _h = P.forward(r["params"], X, M)
            p64, lp64, L64, _Z = P.forward64(r["params"], X, M)
            worst = max(worst, float(_log_prob_error(lp32, lp64, L64, A).max()))
            assert np.isfinite(lp32).all()
            zero_prob += int((p64[np.arange(len(A)), A] < 1e-40).sum())
        print(r["name"], "lengths", r["lengths"].tolist(), "forced actions of probability ~ 0:", zero_prob)
        if r["name"] == "gap+":
            assert zero_prob > 0
    print("LOG_PROBS_REST measured", worst)
    assert worst <= K.LOG_PROBS_REST


def test_rng_seed_is_predicted_to_start_episodes_at_every_residue():
    lens = K.predicted_rng_lengths()
    c0 = K.start_counters(lens)
    print("predicted lengths", lens.tolist(), "start counters mod 4", (c0 % 4).tolist())
    assert lens.shape == (K.RNG_N, K.RNG_EPISODES) and np.all(c0[:, 0] == 0)
    assert {1, 2, 3} <= {int(x) for x in (c0 % 4).ravel()}
    assert K.RNG_SEED >> 32 and K.RNG_BASE >> 32                                        # the high key and counter words are in use


def test_adam_cases_and_restatement_error():
    cases = K.adam_cases()
    assert len(cases) == len(K.ADAM_NS) * len(K.ADAM_STEPS) * len(K.ADAM_HPS) * 2
    worst = 0.0
    zeros = 0
    for c in cases:
        n, (lr, b1, b2, eps) = c["n"], c["hp"]
        g = c["g"][:n]
        mag = np.abs(g[g != 0])
        zeros += int((g == 0).sum())
        assert len(c["p"]) == n + K.ADAM_PAD and (mag.size == 0 or (mag.min() >= 0.99e-12 and mag.max() <= 1.01e3)) and np.all(c["v"] >= 0)
        p32, m32, v32 = c["p"][:n].copy(), c["m"][:n].copy(), c["v"][:n].copy()
        p64, m64, v64 = [a[:n].astype(np.float64) for a in (c["p"], c["m"], c["v"])]
        P.adam_step(p32, g, m32, v32, c["step"], lr, b1, b2, eps)
        P.adam_step64(p64, g, m64, v64, c["step"], lr, b1, b2, eps)
        assert np.isfinite(p32).all() and np.isfinite(p64).all(), c["shape"]
        worst = max(worst, float((np.abs(p32 - p64) / np.maximum(np.abs(p64), lr)).max()))
    assert zeros > 100
    print("ADAM_REST measured", worst)
    assert worst <= K.ADAM_REST
