"""tests/_pdd_cases.py and tests/_pdd_ref.py validated on the CPU, before tests/test_gpu_pdd_cases.py leans on them: every case meets its conditions with no row
left out (wrapping and repeated rows, terminated successors, a live row on which the two networks prefer different actions, a* taking both values, online action
values far enough apart at EVERY successor, NaN-poisoned rings, the placed weights); the float32 torch evaluation picks the same a* on every row of every case and is
MEASURED against float64 per family and figure, with _pdd_ref.MEASURED tied to that measurement; each deliberately wrong reading leaves its bound; the restatement
agrees with tests/_dqn_cases.py's dueling reference and with tests/_ddqn_ref.py where the three algorithms coincide; and the 51-update weighted chain is measured the
same way."""
import numpy as np
import pytest
import torch

import _ddqn_ref as DD
import _dqn_cases as D
import _pdd_cases as K
import _pdd_ref as X

f32 = np.float32
CASES = range(len(K.SPECS))
_case = lambda name: K.make_case(K.NAMES.index(name))   # noqa: E731


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    cpu_ref.lib().ref_set_num_threads(8)
    return cpu_ref


@pytest.fixture
def one_thread():
    """the measured float32 figures are torch's on ONE thread: how a BLAS splits a product over threads must not move them"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def f32_eval():
    """the float32 torch evaluation of every case, computed once (on one thread, see one_thread)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return [X.evaluate(K.make_case(i), torch.float32) for i in CASES]
    finally:
        torch.set_num_threads(n)


def test_families_sizes_and_seeds():
    by = lambda fam: [(s["mb"], s["ring"]) for s in K.SPECS if s["family"] == fam]   # noqa: E731
    assert by("plain") == [(1, (1, 2)), (5, (3, 7)), (K.MAX_SLABS + 1, (2, 30)), (300, (129, 40))] and 300 > 2 * K.MAX_SLABS
    assert [(s["mb"], s["wkind"]) for s in K.SPECS if s["family"] == "weights"] == [(17, "one"), (17, "span"), (300, "span")]
    assert all(s["wkind"] is None for s in K.SPECS if s["family"] != "weights") and [K.SPECS[i]["family"] for i in K.UNIFORM].count("weights") == 0
    assert by("synced") == [(17, (2, 30))] and by("online_tie") == [(9, (3, 7))] and by("terminal") == [(9, (3, 7)), (17, (2, 30))]
    assert by("gamma") == [(17, (2, 30))] * 2 and by("scale") == [(17, (2, 30))] and by("adv_tie") == [(17, (2, 30))] and by("kink_placed") == [(8, (3, 7))]
    assert [s["gamma"] for s in K.SPECS if s["family"] == "gamma"] == [0.0, 1.0] and [s["head_scale"] for s in K.SPECS if s["family"] == "scale"] == [30.0]
    assert set(X.FAMILIES) == set(X.MEASURED) == {s["family"] for s in K.SPECS} and len(K.SEEDS) == len(K.SPECS)
    from deep_rl_amd import _native_pdd
    assert K.MAX_SLABS == _native_pdd.MAX_SLABS and X.NP == _native_pdd.NPARAMS == 11019
    for i in CASES:
        assert K.find_seed(i, tries=K.SEEDS[i] + 1) == K.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_case_meets_its_conditions_with_no_row_left_out(i):
    c = K.make_case(i)
    k, (N, S), idx, mb, e, fam = c["cond"], c["ring"], c["idx"], c["mb"], c["exp"], c["family"]
    cap = N * S
    print(c["name"], k)
    assert K.conditions_met(c)
    assert idx.dtype == np.int64 and idx.shape == (mb,) and idx.min() >= 0 and idx.max() < cap
    nx = D.successor(idx, N, S)
    assert np.array_equal(nx, ((idx // N + 1) % S) * N + idx % N) and np.array_equal(nx[idx // N == S - 1], idx[idx // N == S - 1] % N)   # the wrap lands in slot 0
    live = e["live"] > 0
    if mb >= 5:
        assert k["wraps"] >= 2 and k["repeats"] >= 1
        if fam != "terminal":
            assert k["terminated"] >= 1
        if fam not in ("synced", "adv_tie") and c["name"] != "terminal_all_9":
            assert ((e["q_next"].argmax(1) != e["q_target"].argmax(1)) & live).sum() == k["live_differ"] >= 1
        if fam not in K.TIES and c["name"] != "terminal_all_9":
            assert set(e["next_actions"][live].tolist()) == {0, 1}                                   # a* is not a constant
    if mb == 1:
        assert k["wraps"] == 1 and idx[0] // N == S - 1
    rows, succ = np.zeros(cap, bool), np.zeros(cap, bool)
    rows[idx] = True; succ[nx] = True
    obs, rew = c["observations"].reshape(cap, 4), c["rewards"].reshape(cap)
    act, term = c["actions"].reshape(cap), c["terminated"].reshape(cap)
    assert obs.dtype == f32 and rew.dtype == f32 and term.dtype == np.uint8 and act.dtype == np.int64
    # the poison: NaN / 2 / 1 wherever the batch references nothing; a sampled row's OWN reward is NaN and its own flag 1 unless it is another sampled row's successor
    assert np.isnan(obs[~(rows | succ)]).all() and np.isfinite(obs[rows | succ]).all()
    assert np.isnan(rew[~succ]).all() and np.isfinite(rew[succ]).all() and len(np.unique(rew[succ])) == succ.sum()
    assert (term[~succ] == 1).all() and (act[~rows] == 2).all() and set(np.unique(act[rows])) <= {0, 1}
    assert np.array_equal(np.isnan(rew[idx]), ~succ[idx])
    # nothing excluded: the expectation covers every row and is finite
    for key in ("grads", "target", "current", "td_abs", "q_next", "q_target", "q_row"):
        assert np.isfinite(e[key]).all(), key
    assert e["target"].shape == e["current"].shape == e["td_abs"].shape == e["next_actions"].shape == (mb,) and e["grads"].shape == (X.NP,) and np.abs(e["grads"]).max() > 0
    assert np.array_equal(e["td_abs"], np.abs(e["target"] - e["current"]))                           # unweighted, whatever the weights are
    assert abs(e["loss"]) >= K.LOSS_FLOOR and k["zero_gap"] > K.NEAR_ZERO
    gap = np.abs(e["q_next"][:, 0] - e["q_next"][:, 1])
    if fam in K.TIES:
        assert (gap == 0).all() and (e["next_actions"] == 0).all() and live.sum() >= 1
    else:
        assert gap.min() >= X.CLOSE_Q[fam] == 2 * X.BOUND[fam]["q"]                                  # every successor, the terminated ones included: the share left out is 0
    if fam == "online_tie":
        assert (e["q_target"][live, 1] > e["q_target"][live, 0]).sum() * 2 >= live.sum()            # the target's own max would take action 1's value there
    a, b = D.DUEL["Wa"]
    tied = lambda v: np.array_equal(v[a:a + D.H2], v[a + D.H2:b]) and v[D.DUEL["ba"][0]] == v[D.DUEL["ba"][0] + 1]   # noqa: E731
    assert tied(c["params"]) == (fam in K.TIES) and tied(c["target"]) == (fam == "adv_tie")
    if fam == "adv_tie":                                                                             # the advantage term vanishes: Q is the value head alone
        assert np.array_equal(e["q_row"][:, 0], e["q_row"][:, 1]) and np.array_equal(e["q_target"][:, 0], e["q_target"][:, 1])
    if fam == "synced":
        assert np.array_equal(c["params"], c["target"]) and c["params"] is not c["target"]
    else:
        assert np.abs(c["params"].astype(np.float64) - c["target"]).mean() > 0.02                    # an independent draw, not a near-copy
    if fam == "terminal":
        assert (~live).sum() == (mb if c["p_term"] == 1.0 else 0)
    if fam == "kink_placed":
        assert len(c["units"]["1"]) == 4 and len(c["units"]["2"]) == 4 and (e["grads"] == 0).sum() >= 4 * 4 + 4 + 4 * D.H1 + 4
    w = c["weights"]
    if c["wkind"] is None:
        assert w is None
    else:
        assert w.dtype == f32 and w.shape == (mb,)
        if c["wkind"] == "one":
            assert (w == 1).all()
        else:
            assert (w == 0).sum() == 1 and (w == 1).sum() >= 1 and w.max() == 1 and w[w > 0].min() >= 1e-3 and (w[w > 0] < 0.01).any() and e["td_abs"][w == 0].min() > 0


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_f32_picks_the_same_action_and_relu_side_on_every_row(i, f32_eval):
    c, g = K.make_case(i), f32_eval[i]
    e = c["exp"]
    assert np.array_equal(g["next_actions"], e["next_actions"])
    m1, m2 = np.ones(D.H1, bool), np.ones(D.H2, bool)
    m1[c["units"]["1"]] = False; m2[c["units"]["2"]] = False
    assert np.array_equal(g["z1"][:, m1] > 0, e["z1"][:, m1] > 0) and np.array_equal(g["z2"][:, m2] > 0, e["z2"][:, m2] > 0)
    assert not g["z1"][:, ~m1].any() and not g["z2"][:, ~m2].any()                                   # the placed units: exactly 0 in every precision


def test_measured_is_what_float32_torch_gives_against_float64(f32_eval):
    worst = {}
    for i in CASES:
        c = K.make_case(i)
        fig = X.figures(c["exp"], f32_eval[i], c["family"])
        print("%-18s" % c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
        assert set(fig) == set(X.FIGURES)
        w = worst.setdefault(c["family"], {})
        for k, v in fig.items():
            w[k] = max(w.get(k, 0.0), v)
    assert X.BAR == dict(loss=2e-5, grad=1e-5)
    for fam, w in worst.items():
        print("%-12s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
        for k, v in w.items():
            assert v <= X.MEASURED[fam][k], (fam, k, v)                          # the stored values cover the measurement
            assert X.MEASURED[fam][k] <= 1.25 * v, (fam, k, v)                   # and the table cannot drift loose
            assert X.BOUND[fam][k] == max(8 * X.MEASURED[fam][k], X.BAR.get(k, 0.0))
        assert set(X.BOUND[fam]) == set(X.FIGURES) and all(X.BOUND[fam][k] == 8 * X.MEASURED[fam][k] for k in ("q", "target", "current", "td_abs"))   # no bar on these


@pytest.mark.parametrize("variant", X.VARIANTS)
def test_a_wrong_reading_leaves_its_bound(variant):
    """every wrong reading of the target, the head or the weights moves the gradient out of its bound on at least one of the cases that can show it; td_abs_weighted
    moves no gradient (|td| is an output beside the loss), so it is the td_abs figure that must leave its bound"""
    weighted = variant in ("weights_ignored", "weight_squared", "td_abs_weighted")
    names = tuple(n for n in K.NAMES if n.startswith("weights_span" if weighted else "plain"))
    figure = "td_abs" if variant == "td_abs_weighted" else "grad"
    out = {}
    for name in names:
        c = _case(name)
        wrong = X.evaluate(c, variant=variant)
        out[name] = X.figures(c["exp"], wrong, c["family"])[figure] / X.BOUND[c["family"]][figure]
        if variant == "td_abs_weighted":
            assert np.array_equal(wrong["grads"], c["exp"]["grads"])
    print(variant, figure, out)
    assert len(names) >= 2 and max(out.values()) > 1
    if weighted or variant == "mean_over_batch":
        assert min(out[n] for n in names if _case(n)["mb"] > 1) > 1                # every case with weights (with more than one row) tells it


def test_the_restatement_agrees_with_the_older_references_where_the_algorithms_coincide():
    """synced: the double target is the plain maximum, so tests/_dqn_cases.py's dueling reference (kind "dueling": dueling_dqn.py in float64) gives the same gradient;
    adv_tie: Q is the value head alone and every a* is 0, so the target is r + gamma v'(obs[nx])"""
    c = _case("synced_17")
    e = c["exp"]
    plain = X.evaluate(c, variant="dqn_max")
    assert np.array_equal(plain["target"], e["target"]) and np.array_equal(plain["grads"], e["grads"])
    dc = dict(c, kinds=("dueling",), dparams=c["params"], dtarget=c["target"], placed_weights=None)
    old = D.evaluate(dc, "dueling")
    assert np.abs(old["grads"] - e["grads"]).max() <= 1e-12 * np.abs(e["grads"]).max() and abs(old["loss"] - e["loss"]) <= 1e-12 * abs(e["loss"])
    t = _case("adv_tie_17")
    et = t["exp"]
    nx = D.successor(t["idx"], *t["ring"])
    with torch.no_grad():
        h2, _, _ = D.features(torch.tensor(t["target"], dtype=torch.float64), torch.tensor(t["observations"].reshape(-1, 4)[nx], dtype=torch.float64))
    v = h2.numpy() @ t["target"][D.DUEL["Wv"][0]:D.DUEL["Wv"][1]].astype(np.float64) + float(t["target"][D.DUEL["bv"][0]])
    want = t["rewards"].reshape(-1)[nx].astype(np.float64) + float(f32(t["gamma"])) * v * et["live"]
    assert np.abs(want - et["target"]).max() <= 1e-12 * np.abs(want).max()
    a, b = D.DUEL["Wa"]
    assert np.abs(et["grads"][a:a + D.H2] + et["grads"][a + D.H2:b]).max() <= 1e-15     # dWa[0] = -dWa[1]: the two advantage rows pull against each other


def test_terminal_all_does_not_see_the_target_network():
    c = _case("terminal_all_9")
    other = np.random.default_rng(99).normal(0, 1, X.NP).astype(f32)
    again = X.evaluate(c, target=other)
    assert np.array_equal(again["grads"], c["exp"]["grads"]) and again["loss"] == c["exp"]["loss"] and np.array_equal(again["target"], c["exp"]["target"])


def test_weights_of_one_are_no_weights():
    c = _case("weights_one_17")
    none = X.evaluate(dict(c, weights=None))
    assert np.array_equal(none["grads"], c["exp"]["grads"]) and none["loss"] == c["exp"]["loss"]


def test_chain_of_51_weighted_updates_is_measured(R, one_thread):
    ring, indices, weights, params, target = X.chain_data(R)
    assert indices.shape == weights.shape == (X.CHAIN_UPDATES, X.CHAIN_BATCH) and indices.min() >= 0 and indices.max() < X.CHAIN_STEPS
    assert weights.dtype == f32 and (weights.max(axis=1) == 1).all() and weights.min() >= 0.05 and params.shape == target.shape == (X.NP,)
    l64, p64 = X.chain(ring, indices, weights, params, target)
    l32, p32 = X.chain(ring, indices, weights, params, target, torch.float32)
    fl, fp = float((np.abs(l32 - l64) / np.abs(l64)).max()), float(np.abs(p32 - p64).max())
    print("chain: loss rel %.3g, params abs %.3g; losses %.4f .. %.4f" % (fl, fp, l64[0], l64[-1]))
    assert np.abs(p64 - params).max() > 20 * X.LR                                 # the parameters moved: 51 steps of about lr each
    for v, key in ((fl, "loss"), (fp, "params")):
        assert v <= X.MEASURED_CHAIN[key] <= 1.25 * v, (key, v)
    assert X.BOUND_CHAIN == dict(loss=max(8 * X.MEASURED_CHAIN["loss"], X.BAR["loss"]), params=8 * X.MEASURED_CHAIN["params"])
    assert DD.CHAIN_UPDATES == 51
