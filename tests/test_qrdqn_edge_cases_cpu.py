"""tests/_qrdqn_edge_cases.py validated on the CPU, before tests/test_gpu_qrdqn_edge_cases.py leans on it: every case meets its conditions with no row left out
(wrapping and repeated rows, NaN / 2 / 1 poison around the batch, target action values far enough apart, pre-activations clear of 0); each family has the property it
is named for, in float64; the autograd expectation agrees with the hand-written derivations of tests/_qrdqn_ref.py; the f32 restatement picks the same a* and the
same ReLU side on every row and is MEASURED against float64 per family and figure, with _qrdqn_edge_cases.MEASURED tied to that measurement; and each deliberately
wrong reading of the formula leaves the device bound, gives NaN, picks another a* or raises on a named case."""
import numpy as np
import pytest
import torch

import _dqn_cases as D
import _qrdqn_cases as K0
import _qrdqn_edge_cases as K
import _qrdqn_ref as X

f32 = np.float32
CASES = range(len(K.SPECS))
_case = lambda name: K.make_case(K.NAMES.index(name))   # noqa: E731
PLAIN = tuple(n for n in K.NAMES if n.startswith("plain"))
PLAIN_5_UP = tuple(n for n in PLAIN if n != "plain_1")


@pytest.fixture(scope="module")
def f32_eval():
    """the f32 restatement of every case, computed once"""
    return [K.restate32(K.make_case(i)) for i in CASES]


def test_families_sizes_and_seeds():
    by = lambda fam: [(s["mb"], s["ring"]) for s in K.SPECS if s["family"] == fam]   # noqa: E731
    assert [mb for mb, _ in by("plain")] == [1, 5, 16, 17, 48, 49, 64, 65, 127, 129, 300]
    assert [r for _, r in by("plain")] == [(1, 2), (3, 7), (2, 30), (2, 30)] + [(129, 40)] * 7
    # the slab sum's tails (rg_reduce: group k adds slabs k, k + 16, ... on four interleaved accumulators): 16 / 17, 48 / 49, 64 / 65 and 127 slabs, all below MAX_SLABS
    assert {16, 17, 48, 49, 64, 65, 127} <= {mb for mb, _ in by("plain") if mb < K.MAX_SLABS} and 300 > 2 * K.MAX_SLABS
    assert by("target_tie") == [(9, (3, 7))] and by("terminal") == [(9, (3, 7)), (17, (2, 30))] and by("gamma") == [(17, (2, 30))] * 2
    assert by("huber_placed") == [(9, (3, 7))] and by("linear") == by("quadratic") == [(17, (2, 30))] and by("kink_placed") == by("dead") == [(8, (3, 7))]
    assert by("single_action") == [(9, (3, 7))] * 2 and by("bad_index") == [(5, (3, 7))]
    assert [s["gamma"] for s in K.SPECS if s["family"] == "gamma"] == [0.0, 1.0]
    assert [s["head_scale"] for s in K.SPECS if s["family"] in ("linear", "quadratic")] == [30.0, 2.0 ** -8]
    assert [s["place"] for s in K.SPECS if s["family"] == "single_action"] == ["single_action0", "single_action1"]
    assert K.NAMES[11:] == ("target_tie_9", "terminal_all_9", "terminal_none_17", "gamma_0_17", "gamma_1_17", "huber_placed_9", "linear_17", "quadratic_17",
                            "kink_placed_8", "dead_8", "single_action0_9", "single_action1_9", "bad_index_5")
    eps = 2.0 ** -20
    assert set(K.HUBER_U) == {0.0, 1.0, -1.0, 1 + eps, -(1 + eps), 1 - eps, -(1 - eps), 0.25, -0.25, 1000.0, -1000.0}
    assert all(float(f32(v)) == v for v in K.HUBER_U) and K.QUAD_REWARDS.tolist() == [0, 0.25, -0.25, 0.5] and K0.REWARDS.tolist() == [1, -3, 5, 0.5, 0]
    assert set(K.FAMILIES) == set(K.MEASURED) == set(K.BOUND) and len(K.SEEDS) == len(K.SPECS) == 24
    from deep_rl_amd import _native_qr
    assert K.MAX_SLABS == _native_qr.MAX_SLABS and K.NP == _native_qr.NPARAMS and K.NQ == _native_qr.N_QUANT
    assert np.array_equal(X.TAUS.astype(np.float64), (2 * np.arange(64) + 1) / 128)
    for i in CASES:
        assert K.find_seed(i, tries=K.SEEDS[i] + 1) == K.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_case_meets_its_conditions_with_no_row_left_out(i):
    c = K.make_case(i)
    k, (N, S), idx, raw, mb, e, fam = c["cond"], c["ring"], c["eidx"], c["idx"], c["mb"], c["exp"], c["family"]
    cap = N * S
    print(c["name"], k)
    assert K.conditions_met(c)
    assert raw.dtype == np.int64 and raw.shape == (mb,) and idx.min() >= 0 and idx.max() < cap
    if fam == "bad_index":
        assert sorted(raw[raw != idx].tolist()) == [-1, cap] and 0 in idx and cap - 1 in idx and np.array_equal(idx, np.clip(raw, 0, cap - 1))
    else:
        assert np.array_equal(raw, idx)
    nx = D.successor(idx, N, S)
    assert np.array_equal(nx, ((idx // N + 1) % S) * N + idx % N) and np.array_equal(nx[idx // N == S - 1], idx[idx // N == S - 1] % N)   # the wrap lands in slot 0
    live = e["live"] > 0
    if mb >= 5:
        assert k["wraps"] >= 2 and k["repeats"] >= 1
        if fam not in ("terminal", "huber_placed"):
            assert (~live).any() and live.any()
    if mb == 1:
        assert k["wraps"] == 1 and idx[0] // N == S - 1 and c["ring"] == (1, 2)
    if mb >= 16:
        assert set(e["next_actions"].tolist()) == {0, 1}
    rows, succ = np.zeros(cap, bool), np.zeros(cap, bool)
    rows[idx] = True; succ[nx] = True
    obs, rew = c["observations"].reshape(cap, 4), c["rewards"].reshape(cap)
    act, term = c["actions"].reshape(cap), c["terminated"].reshape(cap)
    assert obs.dtype == f32 and rew.dtype == f32 and term.dtype == np.uint8 and act.dtype == np.int64 and c["params"].dtype == f32 and c["target"].dtype == f32
    # the poison: NaN / 2 / 1 wherever the batch references nothing; a sampled row's OWN reward is NaN and its own flag 1 unless it is another sampled row's successor
    assert np.isnan(obs[~(rows | succ)]).all() and np.isfinite(obs[rows | succ]).all()
    assert np.isnan(rew[~succ]).all() and np.isfinite(rew[succ]).all()
    assert (term[~succ] == 1).all() and (act[~rows] == 2).all() and set(np.unique(act[rows])) <= {0, 1}
    assert np.array_equal(np.isnan(rew[idx]), ~succ[idx]) and k["poisoned"] > 0                     # (every case here has a row that is nobody's successor)
    # nothing excluded: the expectation covers every row and is finite
    for key in ("grads", "target", "current", "q"):
        assert np.isfinite(e[key]).all(), key
    assert e["target"].shape == e["current"].shape == (mb, K.NQ) and e["next_actions"].shape == (mb,) and e["grads"].shape == (K.NP,) and np.abs(e["grads"]).max() > 0
    assert e["loss"] > 0 and k["zero_gap"] > K.NEAR_ZERO
    gap = np.abs(e["q"][:, 0] - e["q"][:, 1])
    if fam == "target_tie":
        assert (gap == 0).all() and (e["next_actions"] == 0).all()
        t = c["target"]
        assert np.array_equal(t[K.W3:K.W3 + K.NQ * K.H2], t[K.W3 + K.NQ * K.H2:K.B3]) and np.array_equal(t[K.B3:K.B3 + K.NQ], t[K.B3 + K.NQ:])
    else:
        assert gap.min() >= K.CLOSE_Q[fam] == 2 * K.BOUND[fam]["q"] > 0                              # every successor, the terminated ones included
    assert np.abs(c["params"].astype(np.float64) - c["target"]).mean() > 0.02 or fam == "quadratic"  # an independent draw, not a near-copy
    assert not np.array_equal(c["params"][:K.W3], c["target"][:K.W3])
    # ---- what the family is named for, in float64
    u = K.pairs(e)
    r_next = rew[nx].astype(np.float64)
    zero = e["grads"] == 0
    g3 = zero[K.W3:K.B3].reshape(2, K.NQ, K.H2)
    gb3 = zero[K.B3:].reshape(2, K.NQ)
    if fam == "plain":
        assert c["p_term"] == 1 / 3 and (mb < 48 or 0.2 < (~live).mean() < 0.47)                    # about a third of the successors terminated
        if mb >= 5:
            assert (u < 0).any() and (u > 0).any() and (np.abs(u) < 1).any() and (np.abs(u) > 1).any()
        if mb >= 16:
            assert set(rew[nx].tolist()) == set(K0.REWARDS.tolist())                                # _qrdqn_cases.REWARDS dealt in turn
    if fam == "terminal":
        assert (~live).sum() == (mb if c["p_term"] == 1.0 else 0)
    if c["name"] in ("terminal_all_9", "gamma_0_17", "huber_placed_9"):
        assert np.array_equal(e["target"], np.repeat(r_next[:, None], K.NQ, axis=1))                # the reward in all 64 places
    if c["name"] == "gamma_0_17":
        assert live.any()                                                                           # on live rows too
    if fam == "huber_placed":
        assert not live.any() and not c["params"][K.W3:K.B3].any()
        b3 = c["params"][K.B3:].reshape(2, K.NQ).astype(np.float64)
        assert np.array_equal(e["current"], b3[act[idx]])                                           # current is b3 of the stored action
        assert np.array_equal(np.ldexp(b3, 20), np.round(np.ldexp(b3, 20))) and np.array_equal(r_next * 4, np.round(r_next * 4))   # dyadic
        for v in K.HUBER_U:
            assert (u == v).any(), v                                                                # each edge of the loss is reached, exactly
        assert (u.astype(f32) == u).all()                                                           # and f32 forms the same u: target - current is exact
        assert zero[:K.W3].all() and zero[:K.W3].sum() == 10_764 and not zero[K.W3:].all()
    if fam == "linear":
        assert (np.abs(u) > 1).mean() >= K.LINEAR_SHARE == 0.95
    if fam == "quadratic":
        assert np.abs(u).max() < 1 and set(rew[nx].tolist()) <= set(K.QUAD_REWARDS.tolist())
    if fam == "kink_placed":
        u1, u2 = c["units"]["1"], c["units"]["2"]
        assert len(u1) == 4 and len(u2) == 4 and {0, K.H1 - 1} <= set(u1.tolist()) and {0, K.H2 - 1} <= set(u2.tolist())
        assert not e["z1"][:, u1].any() and not e["z2"][:, u2].any()
        assert zero[0:480].reshape(K.H1, 4)[u1].all() and zero[480:600][u1].all() and zero[600:10680].reshape(K.H2, K.H1)[u2].all() and zero[10680:10764][u2].all()
        assert zero[600:10680].reshape(K.H2, K.H1)[:, u1].all() and g3[:, :, u2].all()
        assert zero.sum() >= 4 * 4 + 4 + 4 * K.H1 + 4
    if fam == "dead":
        assert (e["z2"] < -100).all() and zero[:K.B3].all() and not zero[K.B3:].all()
    if fam == "single_action":
        a = int(c["place"][-1])
        assert (act[idx] == a).all() and g3[1 - a].all() and gb3[1 - a].all() and not g3[a].all() and not gb3[a].any()
        assert zero.sum() >= K.NQ * K.H2 + K.NQ
    elif mb >= 5:
        assert set(act[idx].tolist()) == {0, 1}


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_autograd_agrees_with_the_hand_written_derivations(i):
    """float64 against float64: _qrdqn_ref.forward64 / target / loss_grad derive forward, targets and backward by hand, this file's reference by autograd"""
    c = K.make_case(i)
    e, mb = c["exp"], c["mb"]
    Xb, A, Xn, Rw, Tm = K.batch_of(c)
    th64, q64 = X.forward64(c["target"], Xn)[:2]
    assert np.abs(q64 - e["q"]).max() <= 1e-12
    na, tgt, _q = X.target(c["target"], Xn, Rw, Tm, gamma=c["gamma"], dtype=np.float64)
    if c["family"] != "target_tie":                                                                 # (one 128-column product need not tie bit for bit)
        assert np.array_equal(na, e["next_actions"])
    assert np.abs(tgt - e["target"]).max() <= 1e-12
    loss, g, cur = X.loss_grad(c["params"], Xb, A, e["target"], dtype=np.float64)
    assert abs(loss - e["loss"]) <= 1e-12 * abs(e["loss"]) and np.abs(cur - e["current"]).max() <= 1e-12
    assert np.abs(X.forward64(c["params"], Xb)[0][np.arange(mb), A] - e["current"]).max() <= 1e-12
    assert np.abs(g - e["grads"]).max() <= 1e-11 * np.abs(e["grads"]).max()
    assert np.array_equal(g == 0, e["grads"] == 0)                                                  # the exact zeros are the same elements


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_f32_picks_the_same_action_and_relu_side_on_every_row(i, f32_eval):
    c, g = K.make_case(i), f32_eval[i]
    e = c["exp"]
    assert np.array_equal(g["next_actions"], e["next_actions"])                                     # no row excluded
    Xb = K.batch_of(c)[0]
    h1, h2 = X.torso(c["params"], Xb)
    assert np.array_equal(h1 > 0, e["z1"] > 0) and np.array_equal(h2 > 0, e["z2"] > 0)              # (a placed unit is exactly 0 in every precision: not > 0)
    e32 = K.evaluate(c, dtype=torch.float32)                                                        # the reference itself in float32: the same a*, the same sides
    assert np.array_equal(e32["next_actions"], e["next_actions"]) and np.array_equal(e32["z1"] > 0, e["z1"] > 0) and np.array_equal(e32["z2"] > 0, e["z2"] > 0)
    if c["family"] == "target_tie":
        q = g["q"].astype(f32)
        assert np.array_equal(q[:, 0].view(np.uint32), q[:, 1].view(np.uint32)) and not g["next_actions"].any()
        assert np.array_equal(e32["q"][:, 0], e32["q"][:, 1])
    if c["name"] in ("terminal_all_9", "gamma_0_17", "huber_placed_9"):                             # r + 0 * theta is r, bit for bit
        Rw = K.batch_of(c)[3]
        assert np.array_equal(g["target"].astype(f32).view(np.uint32), np.repeat(Rw[:, None], K.NQ, axis=1).view(np.uint32))
    if c["family"] == "huber_placed":
        assert np.array_equal(g["current"], e["current"])


def test_measured_is_what_the_f32_restatement_gives_against_float64(f32_eval):
    worst = {}
    for i in CASES:
        c = K.make_case(i)
        fig = K.figures(c["exp"], f32_eval[i])
        print("%-18s" % c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
        assert set(fig) == set(K.FIGURES)
        w = worst.setdefault(c["family"], {})
        for k, v in fig.items():
            w[k] = max(w.get(k, 0.0), v)
    assert K.SHIPPED == dict(target=X.BOUND_TARGET_ABS, current=X.BOUND_QUANT_ABS, loss=X.BOUND_LOSS_REL, grad=X.BOUND_GRAD_REL, q=X.BOUND_Q_ABS)
    assert K.NO_FLOOR == (("quadratic", "q"),)
    for fam, w in worst.items():
        print("%-14s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
        for k, v in w.items():
            assert v <= K.MEASURED[fam][k], (fam, k, v)                          # the stored values cover the measurement
            assert K.MEASURED[fam][k] <= 1.25 * v, (fam, k, v)                   # and the table cannot drift loose
            if (fam, k) in K.NO_FLOOR:                                           # narrower than the rule: 8 x MEASURED alone, below the shipped bound
                assert K.BOUND[fam][k] == 8 * K.MEASURED[fam][k] < K.SHIPPED[k]
            else:
                assert K.BOUND[fam][k] == max(8 * K.MEASURED[fam][k], K.SHIPPED[k])  # never below what tests/test_gpu_qrdqn_cases.py holds the kernel to
        assert K.CLOSE_Q[fam] == 2 * K.BOUND[fam]["q"]
    # linear: quantiles of several hundred carry their f32 error at full weight — more than ten times the plain family's, and still inside 1 / 8 of the shipped bounds
    assert worst["linear"]["target"] > 10 * worst["plain"]["target"] and worst["linear"]["current"] > 10 * worst["plain"]["current"]
    assert 8 * K.MEASURED["linear"]["target"] <= X.BOUND_TARGET_ABS and 8 * K.MEASURED["linear"]["current"] <= X.BOUND_QUANT_ABS
    # quadratic: under the shipped q bound no seed could keep every successor's action values CLOSE_Q apart (the reason for NO_FLOOR)
    gap = np.abs(np.diff(_case("quadratic_17")["exp"]["q"], axis=1))
    assert gap.max() < 2 * X.BOUND_Q_ABS and gap.min() >= K.CLOSE_Q["quadratic"]


def test_the_f32_loss_stage_reaches_the_placed_edges(f32_eval):
    """huber_placed in f32: the restatement's u are the placed values exactly, so the device's loss stage runs on both sides of every edge"""
    c = _case("huber_placed_9")
    g = f32_eval[K.NAMES.index("huber_placed_9")]
    u = (g["target"].astype(f32)[:, None, :] - g["current"].astype(f32)[:, :, None]).astype(f32)
    for v in K.HUBER_U:
        assert (u == f32(v)).any(), v
    assert np.array_equal(u.astype(np.float64), K.pairs(c["exp"]))


# variant -> the named cases; "all": the wrong reading must show on every one of them, "any": on at least one
TEETH = {
    "reward_at_row": (PLAIN, "all"),
    "terminated_at_row": (PLAIN, "any"),
    "no_wrap": (PLAIN, "all"),
    "tie_takes_last": (("target_tie_9",), "all"),
    "relu_one_at_zero": (("kink_placed_8",), "all"),
    "stray_action_as_1": (PLAIN, "any"),
    "slab_left_out": (("plain_17", "plain_49", "plain_65"), "all"),
    "mean_over_128": (PLAIN + ("terminal_none_17",), "all"),
    "pairs_transposed": (PLAIN_5_UP, "all"),
    "taus_from_zero": (PLAIN_5_UP, "all"),
    "dh2_last_quantile_left_out": (PLAIN_5_UP, "all"),
    "greedy_by_online_net": (tuple(n for n in PLAIN_5_UP if n != "plain_5"), "all"),
    "other_action_rows_touched": (("single_action0_9", "single_action1_9"), "all"),
}


def _wrong(c, variant):
    """-> ("raise", text) | ("nan", None) | ("actions", rows that differ) | ("figures", the largest figure over its device bound)"""
    try:
        w = K.evaluate(c, variant=variant)
    except (RuntimeError, IndexError) as err:
        return "raise", str(err)[:60]
    if not (np.isfinite(w["grads"]).all() and np.isfinite(w["loss"]) and np.isfinite(w["target"]).all()):
        return "nan", None
    if not np.array_equal(w["next_actions"], c["exp"]["next_actions"]):
        return "actions", int((w["next_actions"] != c["exp"]["next_actions"]).sum())
    fig = K.figures(c["exp"], w)
    return "figures", max(fig[k] / K.BOUND[c["family"]][k] for k in K.FIGURES)


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_a_wrong_reading_leaves_the_device_bound(variant):
    assert set(TEETH) == set(K.VARIANTS)
    names, mode = TEETH[variant]
    out = {name: _wrong(_case(name), variant) for name in names}
    print(variant, out)
    shows = {name: kind in ("raise", "nan") or (kind == "actions" and v > 0) or (kind == "figures" and v > 1) for name, (kind, v) in out.items()}
    assert all(shows.values()) if mode == "all" else any(shows.values())
    kinds = {kind for kind, _ in out.values()}
    if variant in ("reward_at_row", "no_wrap"):
        assert kinds == {"nan"}                                                  # the poison: a NaN reward
    if variant == "tie_takes_last":
        assert out["target_tie_9"] == ("actions", 9)
    if variant == "greedy_by_online_net":
        assert kinds == {"actions"}
    if variant == "relu_one_at_zero":
        c = _case("kink_placed_8")
        assert K.evaluate(c, variant=variant)["grads"][c["exp"]["grads"] == 0].any()
    if variant == "other_action_rows_touched":                                   # non-zero exactly where float64 has the other action's exact zeros
        for name in names:
            c = _case(name)
            a = int(c["place"][-1])
            w = K.evaluate(c, variant=variant)
            assert w["grads"][K.W3:K.B3].reshape(2, K.NQ, K.H2)[1 - a].any() and w["grads"][K.B3:].reshape(2, K.NQ)[1 - a].all()
            assert w["loss"] == c["exp"]["loss"] and np.array_equal(w["grads"][:K.W3], c["exp"]["grads"][:K.W3])   # and nowhere else


def test_the_right_reading_has_no_teeth_marks():
    """the helper itself: the right reading, evaluated again, is bit for bit the expectation"""
    for name in ("plain_5", "kink_placed_8", "huber_placed_9", "linear_17"):
        c = _case(name)
        again = K.evaluate(c)
        assert np.array_equal(again["grads"], c["exp"]["grads"]) and again["loss"] == c["exp"]["loss"] and np.array_equal(again["target"], c["exp"]["target"])
        assert _wrong(c, None)[0] == "figures" and _wrong(c, None)[1] == 0.0
    assert torch.get_default_dtype() == torch.float32
