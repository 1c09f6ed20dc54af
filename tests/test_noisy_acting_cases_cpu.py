"""tests/_noisy_acting_cases.py on the CPU: the batched float64 forwards are the ref modules'; the two controllers decide as tests/_timelimit_cases.rule under the
mean network; the predicted live runs hold their edges (every condition the GPU tests assert again on the device's own trajectory: an env truncated twice, actions
the noise chose against the mean network, at most 1 % of the decisions inside CLOSE_Q); and each wrong reading of the noise key (VARIANTS) changes at least one
expected action of the live, the shared-workgroup or the epsilon run at a decision outside CLOSE_Q, so the GPU comparison would fail for it."""
import numpy as np
import pytest

import _noisy_acting_cases as A
import _noisy_ref as Z
import _rainbow_ref as RZ
import _timelimit_cases as T


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


@pytest.mark.parametrize("algo", A.ALGOS)
def test_batched_forwards_are_the_ref_modules(algo):
    """q64 over many rows, each under its own sample, against _noisy_ref.forward / _rainbow_ref.forward row by row: two float64 evaluations of the same formulas, which
    differ by their summation order alone (1e-11 of values up to 100, six orders below the smallest CLOSE_Q)"""
    rng = np.random.default_rng(0)
    obs = rng.uniform(-0.3, 0.3, (9, 4)).astype(np.float32)
    for p in (A.live_params(algo, 1), A.CONTROLLERS[algo](), A.random_params(algo)):
        assert p.dtype == np.float32 and p.size == A.NPARAMS[algo] and p[A.REF[algo].SIGMA:].all()
        xi = A.xi32(algo, A.BASE + np.arange(9), 7, A.STREAM_ACT)
        assert xi.shape == (9, A.NXI[algo]) and xi.dtype == np.float32
        q, qm = A.q64(algo, p, obs, xi), A.q64(algo, p, obs)
        for r in range(9):
            if algo == "noisy":
                ref, refm = Z.forward(p, obs[r], xi[r])[0], Z.forward(p, obs[r])[0]
            else:
                assert np.array_equal(A._rb_eps_rows(xi[r:r + 1])[0].view(np.uint32), RZ.eps_of(*RZ.factors(xi[r])).view(np.uint32))
                ref, refm = RZ.forward(p, obs[r], A.SUPPORT, RZ.eps_of(*RZ.factors(xi[r])))[1][0], RZ.forward(p, obs[r], A.SUPPORT)[1][0]
            assert np.abs(q[r] - ref).max() <= 1e-11 and np.abs(qm[r] - refm).max() <= 1e-11, (r, q[r], ref)
        assert not np.array_equal(q, qm)


@pytest.mark.parametrize("algo", A.ALGOS)
def test_controllers_decide_as_the_rule_under_the_mean_network(algo):
    """on random observations and on the 5,500 observations of the mean network's own run, which holds what the GPU test asserts of it"""
    p = A.CONTROLLERS[algo]()
    assert np.array_equal(p[A.REF[algo].SIGMA:], A.REF[algo].default_sigma(A.SIGMA_SCALE)) and p[A.REF[algo].SIGMA:].all()
    if algo == "noisy":
        assert np.array_equal(p[:Z.NP_MEAN], T.controller_dueling(A.CONTROLLER_K))
    else:
        assert not p[RZ.HEAD:RZ.WA].any() and np.count_nonzero(p[RZ.WA:RZ.SIGMA]) == 2                      # the value stream is zero; two advantage weights
    c = A.close_q(algo, "off")
    r = A.live_run(algo, False)
    case = r["case"]
    rng = np.random.default_rng(1)
    for obs in (rng.uniform(-0.2, 0.2, (4096, 4)).astype(np.float32), case.obs[:-1].reshape(-1, 4)):
        q = A.q64(algo, p, obs)
        far = A.gaps(q) >= c
        assert (~far).mean() <= 0.01 and np.array_equal((q[:, 1] > q[:, 0]).astype(np.int64)[far], T.rule(obs)[far])
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2 and set(np.unique(case.actions).tolist()) == {0, 1}, k


@pytest.mark.parametrize("algo", A.ALGOS)
def test_the_predicted_noisy_run_holds_its_edges(algo):
    r = A.live_run(algo, True)
    case, p = r["case"], A.CONTROLLERS[algo]()
    assert case.steps == A.LIVE_STEPS == 1100 and case.n == 5 and r["call_list"][:2] == [49, 50]
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    gap = A.gaps(r["q"])
    excluded = gap < A.close_q(algo)
    assert excluded.mean() <= 0.01
    qm = A.q64(algo, p, case.obs[:-1]).reshape(case.steps, case.n, 2)
    flips = ((qm[..., 1] > qm[..., 0]).astype(np.int64) != case.actions) & ~excluded & (A.gaps(qm) >= A.close_q(algo))
    print(algo, k, "noise-chosen", int(flips.sum()), "excluded", int(excluded.sum()), "smallest gap %.3g" % gap.min())
    assert flips.sum() >= 100                                        # the noise is what chose, hundreds of times
    # elapsed and the step counter coincide until the first episode ends and differ afterwards: what elapsed_for_ctr needs
    assert (case.elapsed[:500] == np.arange(500)[:, None]).all() and (case.elapsed[501] == 1).all()


@pytest.mark.parametrize("algo", A.ALGOS)
def test_the_shared_workgroup_case(algo):
    assert len(A.SHARED_COMPARED) == 12 + 128 and set(T.SHARED_1030) <= set(A.SHARED_COMPARED) and A.SHARED_N > A.GRID and sum(A.SHARED_CALLS) == 8
    assert all(A.partner(A.partner(i)) == i and A.partner(i) in T.SHARED_1030 for i in T.SHARED_1030)
    r = A.shared_run(algo)
    k = A.shared_conditions(algo, r, A.live_params(algo, A.SHARED_PARAM_SEED[algo]))
    assert k["excluded"] <= 0.01 and len(k["told_apart"]) >= 1, k
    assert set(np.unique(r["actions"][:, list(A.SHARED_COMPARED)]).tolist()) == {0, 1}
    # env w and env 1,024 + w draw different samples
    x = r["xi"]
    for w in range(6):
        assert not np.array_equal(x[:, w], x[:, A.GRID + w]) and abs(np.corrcoef(x[0, w], x[0, A.GRID + w])[0, 1]) < 0.3


@pytest.mark.parametrize("algo", A.ALGOS)
def test_the_epsilon_case(algo, R):
    r = A.explore_run(algo)
    assert r["call_list"] == [7] * 8 + [4] and A.EXPLORE_STARTS % A.EXPLORE_CALL != 0          # learning_starts falls inside a call
    k = A.explore_conditions(algo, r, A.live_params(algo, A.EXPLORE_PARAM_SEED[algo]))
    assert k["both_branches"] and k["greedy_after_exploring"] and k["exploring_after_greedy"] and k["excluded"] <= 0.01 and len(k["greedy_count_caught"]) >= 1, k
    ex, ra = r["explores"], r["random"]
    assert ex[:A.EXPLORE_STARTS].all() and not ex[A.EXPLORE_STARTS:].all() and np.array_equal(r["actions"][ex], ra[ex])
    # the exploration draw is the oracle's, and the table is constant at 0.5
    assert (A.eps_table(64, 0.5, 0.5) == 0.5).all() and A.eps_table(3, 1.0, 0.05, 0.5, 400).tolist() == [1.0, 1.0 + (0.05 - 1.0) / 200.0, 1.0 + (0.05 - 1.0) / 200.0 * 2.0]
    for e in range(A.EXPLORE_N):
        for g in (0, 12, 13, 14, 37, 59):
            u, a = R.dqn_explore_draw(A.SEED, A.BASE + e, g)
            assert int(a) == int(ra[g, e]) and bool(ex[g, e]) == (g < A.EXPLORE_STARTS or float(u) < 0.5)


_RUNS = {"live": lambda algo: (A.live_run(algo, True), A.CONTROLLERS[algo]()),
         "shared": lambda algo: (A.shared_run(algo), A.live_params(algo, A.SHARED_PARAM_SEED[algo])),
         "explore": lambda algo: (A.explore_run(algo), A.live_params(algo, A.EXPLORE_PARAM_SEED[algo]))}
# where each reading must show at the least (it may show elsewhere too)
_SHOWS_IN = {"workgroup_index_for_env_id": "shared", "env_index_without_base": "live", "step_in_launch_for_ctr": "live", "elapsed_for_ctr": "live",
             "greedy_count_for_ctr": "explore", "stream_14_for_13": "live"}


@pytest.mark.parametrize("variant", A.VARIANTS)
@pytest.mark.parametrize("algo", A.ALGOS)
def test_each_wrong_reading_of_the_key_changes_an_expected_action(algo, variant):
    assert set(_SHOWS_IN) == set(A.VARIANTS)
    r, p = _RUNS[_SHOWS_IN[variant]](algo)
    aw, gw = A.expected(algo, p, r, variant)
    ar, gr = A.expected(algo, p, r, None)
    greedy = ~r["explores"]
    assert np.array_equal(ar[greedy], r["actions"][greedy]) and np.abs(gr - A.gaps(r["q"])).max() <= 1e-11   # the right reading is the run itself (summed in another order)
    envs = [i for i in A.SHARED_COMPARED] if _SHOWS_IN[variant] == "shared" else None
    got = A.caught(r["actions"], gr, aw, gw, greedy, A.close_q(algo), envs)
    print(algo, variant, "first changed decision outside CLOSE_Q in envs", got)
    assert len(got) >= 1
    if variant == "workgroup_index_for_env_id":
        assert all(e >= A.GRID for e in got)                          # only the second env of a workgroup can tell
    if variant == "elapsed_for_ctr":                                  # identical until the first episode ends: nothing before step 500 may differ
        assert np.array_equal(aw[:500], ar[:500])


def test_the_keys():
    a, b, s = A.keys(None, 3, [2, 3])
    assert s == 13 and a.tolist() == [[300, 301, 302]] * 5 and b[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert A.keys("step_in_launch_for_ctr", 3, [2, 3])[1][:, 1].tolist() == [0, 1, 0, 1, 2]
    assert A.keys("env_index_without_base", 3, [2, 3])[0][0].tolist() == [0, 1, 2]
    assert A.keys("workgroup_index_for_env_id", 1030, [1])[0][0, [0, 1023, 1024, 1029]].tolist() == [300, 1323, 300, 305]
    ex = np.array([[True, False], [False, False], [True, True], [False, False]])
    assert A.keys("greedy_count_for_ctr", 2, [4], explores=ex)[1].tolist() == [[0, 0], [0, 1], [1, 2], [1, 2]]
    assert A.keys("stream_14_for_13", 1, [1])[2] == 14
    with pytest.raises(AssertionError):
        A.keys("no such reading", 1, [1])
