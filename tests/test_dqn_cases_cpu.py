"""tests/_dqn_cases.py validated on the CPU: every case meets its conditions with no row left out and reaches what it claims (wrapping and repeated rows, NaN-poisoned
rings with the sampled rows' OWN rewards poisoned, exact-zero pre-activations, dead layers, bit-for-bit target ties, placed weights, priorities over 15 decades); f32
evaluations put every online ReLU on the same side as float64; the f32 oracle (oracle/cpu_ref.c: ref_dqn_td_grads, ref_per_td_grads, ref_per_weights,
ref_per_update_priorities, ref_dueling_td_grads) is measured against the float64 autograd reference per family and figure and _dqn_cases.MEASURED is tied to that
measurement; each of the seven known-wrong variants of the reference leaves the bound of a named case; and a torch FLOAT32 run of the same formulas stays within the
device bounds — so when tests/test_gpu_dqn_cases.py fails, a reader knows whether oracle or device is the outlier."""
import numpy as np
import pytest
import torch

import _dqn_cases as K

f32 = np.float32
CASES = range(len(K.SPECS))
_case = lambda name: K.make_case(K.NAMES.index(name))   # noqa: E731


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    cpu_ref.lib().ref_set_num_threads(8)
    return cpu_ref


@pytest.fixture(scope="module")
def oracle(R):
    """the oracle's results on every (kind, case), computed once: {(kind, name): got}"""
    return {(kind, K.SPECS[i]["name"]): K.oracle_eval(R, K.make_case(i), kind) for kind, i in K.RUNS}


def _tensor(g, kind, key):
    s, e = K.LAYOUT[kind][key]
    return g[s:e]


# ---- conditions and reach -----------------------------------------------------------------------------------------------------------
def test_families_sizes_and_seeds():
    by = lambda fam: [s for s in K.SPECS if s["family"] == fam]   # noqa: E731
    assert [s["mb"] for s in by("plain")] == [1, 7, 8, 9, 17, 504, 505, 2048, 2049, 4113]
    assert [s["mb"] for s in by("plain") if "dueling" in s["kinds"]] == [1, 9, 17, 505, 2049]
    assert [(s["mb"], s["p_term"]) for s in by("terminal")] == [(9, 1.0), (17, 0.0)] and [(s["mb"], s["gamma"]) for s in by("gamma")] == [(17, 0.0), (17, 1.0)]
    assert [(s["mb"], s["head_scale"], s["r_std"]) for s in by("scale")] == [(17, 30.0, 10.0), (40, 300.0, 100.0)]
    assert [s["mb"] for s in by("kink_placed")] == [8, 24] and [s["mb"] for s in by("dead")] == [5, 17] and [s["mb"] for s in by("target_tie")] == [9]
    assert [s["mb"] for s in by("weights_placed")] == [8, 17] and [s["mb"] for s in by("converged")] == [17] and [s["mb"] for s in by("dueling_heads")] == [17, 17]
    pw = by("per_weights")
    assert {(s["mb"], s["ring"]) for s in pw} == {(17, (2, 30)), (40, (129, 40))} and {s["alpha"] for s in pw} == {0.6, 1.0}
    assert {s["beta"] for s in pw} >= {"beta0", "one"} and {s["mp"] for s in pw} == {"above", "below"} and any(s["prio"] == "same" for s in pw)
    for fam in ("weights_placed", "per_weights"):
        assert all(s["kinds"] == ("per",) for s in by(fam))
    for fam in ("terminal", "scale", "kink_placed"):
        assert all(s["kinds"] == K.KINDS for s in by(fam))
    assert all(s["kinds"] == ("dueling",) for s in by("dueling_heads"))
    assert {s["ring"] for s in K.SPECS} == set(K.RINGS) and all(s["ring"] == (1, 2) for s in K.SPECS if s["mb"] == 1)
    assert set(K.FAMILIES) == set(K.MEASURED) and len(K.SEEDS) == len(K.SPECS)
    # the kernel's forms: 8-row groups up to 256 of them, the reduce kernels switch at 64 slabs, 16-row groups beyond, 258 of them on 256 workgroups
    assert [(-(-mb // K.row_group(mb)), K.row_group(mb)) for mb in (504, 505, 2048, 2049, 4113)] == [(63, 8), (64, 8), (256, 8), (129, 16), (258, 16)]
    for i in CASES:
        assert K.find_seed(i, tries=K.SEEDS[i] + 1) == K.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_case_meets_its_conditions_with_no_row_left_out(i):
    c = K.make_case(i)
    k, (N, S), idx, mb = c["cond"], c["ring"], c["idx"], c["mb"]
    cap = N * S
    print(c["name"], k)
    assert K.conditions_met(c)
    assert idx.dtype == np.int64 and idx.shape == (mb,) and idx.min() >= 0 and idx.max() < cap
    nx = K.successor(idx, N, S)
    assert np.array_equal(nx, ((idx // N + 1) % S) * N + idx % N) and np.array_equal(nx[idx // N == S - 1], idx[idx // N == S - 1] % N)   # the wrap lands in slot 0
    if mb >= 5:
        assert k["wraps"] >= 2 and k["repeats"] >= 1
    if mb == 1:
        assert k["wraps"] == 1
    rows, succ = np.zeros(cap, bool), np.zeros(cap, bool)
    rows[idx] = True; succ[nx] = True
    obs, rew = c["observations"].reshape(cap, 4), c["rewards"].reshape(cap)
    act, term = c["actions"].reshape(cap), c["terminated"].reshape(cap)
    assert obs.dtype == f32 and rew.dtype == f32 and term.dtype == np.uint8 and act.dtype == np.int64
    # the poison: NaN / 2 / 1 wherever the batch references nothing; a sampled row's OWN reward is NaN and its own flag 1 unless it is another sampled row's successor
    assert np.isnan(obs[~(rows | succ)]).all() and np.isfinite(obs[rows | succ]).all() and (np.abs(obs[rows | succ]) <= np.array(K.OBS_RANGE, f32)).all()
    assert np.isnan(rew[~succ]).all() and np.isfinite(rew[succ]).all() and len(np.unique(rew[succ])) == succ.sum()
    assert (term[~succ] == 1).all() and (act[~rows] == 2).all() and set(np.unique(act[rows])) <= {0, 1}
    own = np.isnan(rew[idx])
    assert np.array_equal(own, ~succ[idx]) and own.mean() == k["poisoned"] >= K.POISON_SHARE
    assert not (rew[idx] == rew[nx]).any()                                                      # r[i] != r[nx] in every row
    # nothing excluded: the expectation covers every row and is finite
    for kind, e in c["exp"].items():
        assert e["td"].shape == (mb,) and np.isfinite(e["grads"]).all() and np.isfinite(e["td"]).all() and np.abs(e["grads"]).max() > 0
        assert e["grads"].shape == (K.DNP if kind == "dueling" else K.NP,)
        if c["family"] not in K.LOOSE:
            assert abs(e["loss"]) >= K.LOSS_FLOOR
    assert k["zero_gap"] > K.NEAR_ZERO
    if "per" in c["kinds"]:
        assert (c["priorities"] >= 0).all() and (c["priorities"].reshape(-1)[idx] > 0).all()
    if c["prio"] == "wide":
        p = c["priorities"].reshape(-1)
        assert 0.1 < (p == 0).mean() < 0.3 and 1e-12 <= p[p > 0].min() and p.max() <= 1e3 and (cap < 1000 or (p[p > 0].min() < 1e-11 and p.max() > 1e2))


def _sequential_f32_preacts(params, x):
    """the pre-activations in float32 in the oracle's summation order (dqn_fwd: k ascending, the bias last), one rounding per operation"""
    p = params.astype(f32)
    s = lambda k, shape: p[K.DQN[k][0]:K.DQN[k][1]].reshape(shape)   # noqa: E731
    W1, W2 = s("W1", (K.H1, 4)), s("W2", (K.H2, K.H1))
    acc = np.zeros((len(x), K.H1), f32)
    for k in range(4):
        acc = acc + W1[None, :, k] * x[:, None, k]
    z1 = acc + s("b1", (K.H1,))
    h1 = np.maximum(z1, f32(0))
    acc = np.zeros((len(x), K.H2), f32)
    for k in range(K.H1):
        acc = acc + W2[None, :, k] * h1[:, None, k]
    return z1, acc + s("b2", (K.H2,))


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_f32_puts_every_online_relu_on_the_side_float64_does(i):
    """the NEAR_ZERO margin does its work: torch's float32 evaluation and a float32 evaluation in the oracle's own summation order give every online pre-activation of every
    sampled row the sign float64 gives it; the placed units of kink_placed are exactly 0 in all three.  No row needs an exclusion."""
    c = K.make_case(i)
    kind = c["kinds"][0]
    e = c["exp"][kind]
    cap = c["ring"][0] * c["ring"][1]
    t32 = K.evaluate(c, kind, torch.float32)
    s1, s2 = _sequential_f32_preacts(c["params"], c["observations"].reshape(cap, 4)[c["idx"]])
    worst = 0.0
    for z64, zt, zs, placed in ((e["z1"], t32["z1"], s1, c["units"]["1"]), (e["z2"], t32["z2"], s2, c["units"]["2"])):
        assert np.array_equal(zt > 0, z64 > 0) and np.array_equal(zs > 0, z64 > 0)
        assert (z64[:, placed] == 0).all() and (zt[:, placed] == 0).all() and (zs[:, placed] == 0).all()
        live = z64 > -100                                   # (a dead layer sits at -1e3, where an f32 ulp is 6e-5 and no sign is in question)
        worst = max(worst, np.abs(zt - z64)[live].max(initial=0.0), np.abs(zs - z64)[live].max(initial=0.0))
    print(c["name"], "zero gap", c["cond"]["zero_gap"], "f32 off by", worst)
    assert worst < c["cond"]["zero_gap"]
    if c["family"] == "kink_placed":
        assert len(c["units"]["1"]) == 4 and len(c["units"]["2"]) == 4 and {0, K.H1 - 1} <= set(c["units"]["1"]) and {0, K.H2 - 1} <= set(c["units"]["2"])
    else:
        assert not len(c["units"]["1"]) and not len(c["units"]["2"])


def test_terminal_all_does_not_see_the_target_net(R):
    """every successor terminated: the expectation and the oracle's bits are the same under a second, unrelated target vector"""
    c = _case("terminal_all_9")
    other = np.random.default_rng(99).normal(0, 1, K.DNP).astype(f32)
    for kind in c["kinds"]:
        e, e2 = c["exp"][kind], K.evaluate(c, kind, target=other[:len(c["exp"][kind]["grads"])])
        assert (e["live"] == 0).all() and np.array_equal(e["grads"], e2["grads"]) and e["loss"] == e2["loss"] and not np.array_equal(e["tmax"], e2["tmax"])
    g1 = K.oracle_eval(R, c, "dqn")
    g2 = K.oracle_eval(R, dict(c, target=other[:K.NP]), "dqn")
    assert np.array_equal(g1["grads"], g2["grads"]) and g1["loss"] == g2["loss"]
    none = _case("terminal_none_17")
    assert (none["exp"]["dqn"]["live"] == 1).all() and (none["terminated"].reshape(-1)[none["idx"]][np.isnan(none["rewards"].reshape(-1)[none["idx"]])] == 1).all()


def test_gamma_cases():
    c0, c1 = _case("gamma_0_17"), _case("gamma_1_17")
    e0, e1 = c0["exp"]["dqn"], c1["exp"]["dqn"]
    r0 = c0["rewards"].reshape(-1)[K.successor(c0["idx"], *c0["ring"])].astype(np.float64)
    assert np.array_equal(e0["td"], r0 - e0["old"])                                            # gamma 0: the target is the reward alone
    r1 = c1["rewards"].reshape(-1)[K.successor(c1["idx"], *c1["ring"])].astype(np.float64)
    assert np.array_equal(e1["td"], (r1 + 1.0 * e1["tmax"] * e1["live"]) - e1["old"]) and (e1["live"] == 1).sum() >= 5


def test_scale_reaches_late_training_magnitudes():
    for name, lo, hi in (("scale_30_17", 3.0, 100.0), ("scale_300_40", 30.0, 1000.0)):
        e = _case(name)["exp"]["dqn"]
        print(name, np.abs(e["old"]).max(), np.abs(e["tmax"]).max(), e["td_abs"].max())
        assert lo < np.abs(e["old"]).max() < hi and lo < np.abs(e["tmax"]).max() < hi


@pytest.mark.parametrize("name", ["kink_placed_8", "kink_placed_24"])
def test_kink_placed_zero_patterns(name, oracle):
    """pre-activation exactly 0 in placed units: the float64 autograd gradient and the oracle's are exactly 0 in dW1[u], db1[u], dW2[j], db2[j], the head's column j and the
    W2[:, u] column — and the oracle is exactly 0 wherever float64 is"""
    c = _case(name)
    u1, u2 = c["units"]["1"], c["units"]["2"]
    for kind in c["kinds"]:
        for g in (c["exp"][kind]["grads"], oracle[(kind, name)]["grads"]):
            assert not _tensor(g, kind, "W1").reshape(K.H1, 4)[u1].any() and not _tensor(g, kind, "b1")[u1].any()
            W2 = _tensor(g, kind, "W2").reshape(K.H2, K.H1)
            assert not W2[u2].any() and not W2[:, u1].any() and not _tensor(g, kind, "b2")[u2].any()
            for key, n in (("W3", 2),) if kind != "dueling" else (("Wv", 1), ("Wa", 2)):
                assert not _tensor(g, kind, key).reshape(n, K.H2)[:, u2].any()
            keep = np.ones(K.H2, bool); keep[u2] = False
            assert np.abs(_tensor(g, kind, "b2")[keep]).max() > 0 and np.abs(W2[keep]).max() > 0
        assert not oracle[(kind, name)]["grads"][K.zero_mask(c["exp"][kind])].any()
    if name == "kink_placed_24":                           # the target net's placed units: a third of each layer, exactly 0 there
        t = c["target"]
        assert (t[K.DQN["b1"][0]:K.DQN["b1"][1]] == 0).sum() == 40 and (t[K.DQN["b2"][0]:K.DQN["b2"][1]] == 0).sum() == 28


def test_dead_layers_zero_patterns(oracle):
    for kind in ("dqn", "per"):
        c = _case("dead_l2_5")
        for g in (c["exp"][kind]["grads"], oracle[(kind, "dead_l2_5")]["grads"]):
            assert not g[:K.DQN["b3"][0]].any() and np.abs(g[K.DQN["b3"][0]:]).max() > 0          # h2 == 0: exactly 0 everywhere except b3
        assert (c["exp"][kind]["z2"] < -900).all()
        c = _case("dead_l1_17")
        for g in (c["exp"][kind]["grads"], oracle[(kind, "dead_l1_17")]["grads"]):
            assert not g[:K.DQN["b2"][0]].any()                                                    # W1, b1, W2
            assert all(np.abs(_tensor(g, kind, key)).max() > 0 for key in ("b2", "W3", "b3"))
        assert (c["exp"][kind]["z1"] < -900).all()
        for name in ("dead_l2_5", "dead_l1_17"):
            assert not oracle[(kind, name)]["grads"][K.zero_mask(_case(name)["exp"][kind])].any()


def test_target_tie_is_bit_for_bit():
    c = _case("target_tie_9")
    cap = c["ring"][0] * c["ring"][1]
    x = c["observations"].reshape(cap, 4)[K.successor(c["idx"], *c["ring"])]
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            q = K.q_values(K._t(c["target"], dtype), K._t(x, dtype), "dqn")[0].numpy()
        assert np.array_equal(q[:, 0], q[:, 1]) and np.abs(q).max() > 0
    assert np.array_equal(c["exp"]["dqn"]["tmax"], q[:, 0]) and len(q) == 9                      # the max of a tie is the value itself


def test_placed_weights_do_not_move_td(oracle):
    for name in ("weights_placed_8", "weights_placed_17"):
        c = _case(name)
        e = c["exp"]["per"]
        w = c["placed_weights"]
        assert w.dtype == f32 and set(np.unique(w)) == set(np.array(K.PLACED_WEIGHTS, f32)) and np.array_equal(e["weights"], w.astype(np.float64))
        plain = K.evaluate(dict(c, placed_weights=None), "per")
        assert np.array_equal(plain["td_abs"], e["td_abs"]) and not np.array_equal(plain["grads"], e["grads"])
        o = oracle[("per", name)]
        assert K.figures(e, o, "per")["weights"] == 0 and (e["td_abs"][w == 0] > 0.01).all()        # a zero-weight row still has its |td| and its priority
        assert np.array_equal(o["prio"][c["idx"]], o["td_abs"])


def test_per_weights_reach(oracle):
    for s in (s for s in K.SPECS if s["family"] == "per_weights"):
        c = _case(s["name"])
        e, o = c["exp"]["per"], oracle[("per", s["name"])]
        w = e["weights"]
        print(s["name"], "beta", c["beta"], "weights", w.min(), w.max(), "max |td|", e["td_abs"].max(), "max_priority", float(c["max_priority"]), "->", e["max_priority"])
        assert w.max() == 1.0 and (w > 0).all() and np.float32(w.min()) > np.finfo(f32).tiny
        if s["beta"] == "beta0":
            assert c["beta"] == float(f32(K.BETA_0))
        if s["beta"] == "one":
            assert c["beta"] == 1.0
        if s["prio"] == "same":
            assert (w == 1.0).all() and (o["weights"] == 1.0).all()
        else:
            assert w.min() < 1e-2
        if s["mp"] == "above":                             # stays bit for bit
            assert e["max_priority"] == float(c["max_priority"]) == o["max_priority"] > e["td_abs"].max()
        else:
            assert e["max_priority"] == e["td_abs"].max() > float(c["max_priority"]) and o["max_priority"] == o["td_abs"].max()
        untouched = np.ones(len(e["prio"]), bool); untouched[c["idx"]] = False
        assert np.array_equal(e["prio"][untouched], c["priorities"].reshape(-1)[untouched].astype(np.float64)) and np.array_equal(o["prio"][untouched], e["prio"][untouched])


def test_converged_is_illconditioned_by_construction():
    c = _case("converged_17")
    e = c["exp"]["dqn"]
    print(np.abs(e["old"]).max(), e["td_abs"].max(), e["loss"])
    assert c["family"] in K.LOOSE and 30 < np.abs(e["old"]).max() < 1000 and e["td_abs"].max() < 5e-3 * np.abs(e["old"]).max()
    assert all(K.BOUND[kind]["converged"][k] == 8 * K.MEASURED["converged"][k] for kind in ("dqn", "per") for k in K.BOUND[kind]["converged"] if k != "weights")
    assert K.BOUND["per"]["converged"]["weights"] == K.BAR["per"]["weights"]


def test_dueling_heads(oracle):
    c = _case("dueling_heads_tie_17")
    e = c["exp"]["dueling"]
    d = c["dparams"]
    Wa, ba = _tensor(d, "dueling", "Wa").reshape(2, K.H2), _tensor(d, "dueling", "ba")
    assert np.array_equal(Wa[0], Wa[1]) and ba[0] == ba[1]
    cap = c["ring"][0] * c["ring"][1]
    with torch.no_grad():
        p, x = K._t(d, torch.float64), K._t(c["observations"].reshape(cap, 4)[c["idx"]], torch.float64)
        value = K.features(p, x)[0] @ p[K.DUEL["Wv"][0]:K.DUEL["Wv"][1]] + p[K.DUEL["bv"][0]]
    assert np.array_equal(e["old"], value.numpy())                                               # the advantage cancels exactly: Q is the value head alone
    for g in (e["grads"], oracle[("dueling", c["name"])]["grads"]):
        gWa, gba = _tensor(g, "dueling", "Wa").reshape(2, K.H2), _tensor(g, "dueling", "ba")
        assert np.array_equal(gWa[0], -gWa[1]) and gba[0] == -gba[1] and np.abs(gWa).max() > 0
    c = _case("dueling_heads_value_1e3_17")
    d = c["dparams"]
    ratio = np.abs(_tensor(d, "dueling", "Wv")).mean() / np.abs(_tensor(d, "dueling", "Wa")).mean()
    assert 300 < ratio < 3000


# ---- the bounds are tied to the measurement -----------------------------------------------------------------------------------------
def test_oracle_against_float64_pins_the_bounds(oracle):
    worst = {}
    for kind, i in K.RUNS:
        c = K.make_case(i)
        fig = K.figures(c["exp"][kind], oracle[(kind, c["name"])], kind)
        print("%-8s %-32s" % (kind, c["name"]), {k: float("%.3g" % v) for k, v in fig.items()})
        assert set(fig) == set(K.BAR[kind])
        w = worst.setdefault(c["family"], {})
        for k, v in fig.items():
            w[k] = max(w.get(k, 0.0), v)
    assert set(worst) == set(K.MEASURED)
    assert K.BAR == dict(dqn=dict(loss=2e-5, grad=1e-5, tensor=1e-3), per=dict(loss=3e-5, td=2e-5, grad=1e-5, tensor=1e-3, weights=3e-5, prio=2e-5),
                         dueling=dict(loss=3e-5, grad=1e-5, tensor=1e-3))
    for fam, w in worst.items():
        print("%-14s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
        assert set(w) == set(K.MEASURED[fam])
        for k, v in w.items():
            assert v <= K.MEASURED[fam][k], (fam, k, v)                          # the stored values cover the measurement
            assert K.MEASURED[fam][k] <= 1.25 * v, (fam, k, v)                   # and the table cannot drift loose
            for kind in K.KINDS:
                if k in K.BAR[kind]:
                    loose = fam in K.LOOSE and k != "weights"
                    assert K.BOUND[kind][fam][k] == (8 * K.MEASURED[fam][k] if loose else max(8 * K.MEASURED[fam][k], K.BAR[kind][k]))
        if fam not in K.LOOSE:
            assert max(w.values()) <= 2e-6, fam                                  # the issue's feasibility figures: the bar, not 8 x the oracle, is the bound
            assert all(K.BOUND[kind][fam][k] == K.BAR[kind][k] for kind in K.KINDS for k in K.BOUND[kind][fam])


def test_a_stray_read_is_visible(R):
    """an index outside the case's rows pulls the poison into the result, and figures() reports it as inf"""
    c = dict(_case("plain_17"))
    cap = c["ring"][0] * c["ring"][1]
    free = np.flatnonzero(np.isnan(c["observations"].reshape(cap, 4)[:, 0]))
    c["idx"] = c["idx"].copy()
    c["idx"][16] = free[0]
    c["actions"] = c["actions"].copy()
    c["actions"].reshape(-1)[free[0]] = 0                 # (the unreferenced action 2 would index outside the oracle's two-action head)
    got = K.oracle_eval(R, c, "dqn")
    assert np.isnan(got["grads"]).any()
    assert K.figures(_case("plain_17")["exp"]["dqn"], got, "dqn")["grad"] == np.inf


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,kind,name,figure", [
    ("reward_at_row", "dqn", "plain_17", "grad"), ("reward_at_row", "dueling", "plain_1", "loss"), ("reward_at_row", "per", "plain_4113", "td"),
    ("terminated_at_row", "dqn", "terminal_none_17", "grad"), ("terminated_at_row", "per", "plain_505", "td"),
    ("no_wrap", "dqn", "plain_9", "grad"), ("no_wrap", "dqn", "plain_1", "loss"), ("no_wrap", "dueling", "plain_2049", "grad"),
    ("relu_one_at_zero", "dqn", "kink_placed_8", "tensor"), ("relu_one_at_zero", "dueling", "kink_placed_24", "tensor"),
    ("weight_inside_square", "per", "weights_placed_8", "grad"), ("weight_inside_square", "per", "weights_placed_17", "loss"),
    ("mean_over_padded", "dqn", "plain_9", "grad"), ("mean_over_padded", "dqn", "plain_2049", "grad"), ("mean_over_padded", "per", "plain_4113", "loss"),
    ("dueling_no_mean", "dueling", "plain_17", "grad"), ("dueling_no_mean", "dueling", "dueling_heads_tie_17", "loss")])
def test_teeth(variant, kind, name, figure):
    """a wrong reading lies >= 10 x the bound away from the right one on the named case, in the named figure"""
    c = _case(name)
    fig = K.figures(c["exp"][kind], K.evaluate(c, kind, variant=variant), kind)
    print(variant, kind, name, {k: float("%.3g" % v) for k, v in fig.items()}, "bound", K.BOUND[kind][c["family"]][figure])
    assert fig[figure] >= 10 * K.BOUND[kind][c["family"]][figure] and K.within(fig, c["family"], kind)
    assert set(K.VARIANTS) == {"reward_at_row", "terminated_at_row", "no_wrap", "relu_one_at_zero", "weight_inside_square", "mean_over_padded", "dueling_no_mean"}


def test_the_own_reward_poison_is_what_shows_a_read_at_the_row():
    """reward_at_row on a row whose own reward is poisoned is a NaN, on the others a wrong number: both are outside the bound"""
    c = _case("plain_17")
    w = K.evaluate(c, "dqn", variant="reward_at_row")
    own = np.isnan(c["rewards"].reshape(-1)[c["idx"]])
    assert np.array_equal(np.isnan(w["td"]), own) and 0 < own.sum() < 17
    assert (np.abs(w["td"][~own] - c["exp"]["dqn"]["td"][~own]) > 1e-3).all()


# ---- the float32 run of the reference -----------------------------------------------------------------------------------------------
def test_torch_float32_stays_within_the_device_bounds():
    """the same formulas evaluated by torch in float32 (its own summation orders) against float64, under the DEVICE bounds, on every case and kind: the bounds leave room
    for an honest f32 evaluation that is neither the oracle nor the kernel"""
    for kind, i in K.RUNS:
        c = K.make_case(i)
        e32 = K.evaluate(c, kind, torch.float32)
        fig = K.figures(c["exp"][kind], e32, kind)
        print("%-8s %-32s" % (kind, c["name"]), {k: float("%.3g" % v) for k, v in fig.items()})
        assert not K.within(fig, c["family"], kind), (kind, c["name"], K.within(fig, c["family"], kind))
        assert not e32["grads"][K.zero_mask(c["exp"][kind])].any()
