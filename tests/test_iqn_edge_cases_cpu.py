"""tests/_iqn_edge_cases.py validated on the CPU, before tests/test_gpu_iqn_edge_cases.py leans on it: every case meets its conditions with no row left out
(wrapping and repeated rows, NaN / 2 / 1 poison around the batch, the placed taus, target action values far enough apart, pre-activations clear of 0, td errors clear
of kappa); each family has the property it is named for, in float64; the autograd expectation agrees with the hand-written backward of tests/_iqn_ref.py; the f32
restatement picks the same a* and the same ReLU side on every row and is MEASURED against float64 per family and figure, with _iqn_edge_cases.MEASURED tied to that
measurement; and each deliberately wrong reading of the formula leaves the device bound, gives NaN or picks another a* on a named case (TEETH: the table)."""
import numpy as np
import pytest
import torch

import _dqn_cases as D
import _iqn_edge_cases as K
import _iqn_ref as R
import _qrdqn_edge_cases as QK
import _qrdqn_ref as QX

f32 = np.float32
CASES = range(len(K.SPECS))
_case = lambda name: K.make_case(K.NAMES.index(name))   # noqa: E731
PLAIN = tuple(n for n in K.NAMES if n.startswith("plain"))
TAILS = tuple(n for n in K.NAMES if n.startswith("tails"))
RELU = tuple("relu_one_at_zero_" + s for s in K.SITES)


@pytest.fixture(scope="module")
def f32_eval():
    """the f32 restatement of every case, computed once"""
    return [K.restate32(K.make_case(i)) for i in CASES]


def test_families_sizes_and_seeds():
    by = lambda fam: [(s["mb"], s["ring"]) for s in K.SPECS if s["family"] == fam]   # noqa: E731
    assert by("plain") == [(1, (1, 2)), (5, (3, 7)), (17, (2, 30))]
    assert [mb for mb, _ in by("tails")] == [16, 32, 33, 48, 49, 63, 64, 65, 127, 129] and [r for _, r in by("tails")] == [(2, 30)] * 3 + [(129, 40)] * 7
    # the slab sum's tails (rg_reduce: group k adds slabs k, k + 16, ... on four interleaved accumulators): 16 / 17, 32 / 33, 48 / 49 and 64 slabs; two and three rows a workgroup
    sizes = {s["mb"] for s in K.SPECS}
    assert {16, 17, 32, 33, 48, 49, 63, 64} <= sizes and {65, 127} <= sizes and 129 > 2 * K.MAX_SLABS
    assert by("tau_bands") == [(17, (2, 30))] and by("target_tie") == [(9, (3, 7))] and by("terminal") == [(9, (3, 7)), (17, (2, 30))] and by("gamma") == [(17, (2, 30))] * 2
    assert by("huber_placed") == [(13, (2, 30))] and by("kink_placed") == by("dead_emb") == by("dead_te") == by("dead_head") == [(8, (3, 7))]
    assert by("single_action") == [(9, (3, 7))] * 2 and by("bad_index") == [(5, (3, 7))]
    assert [s["gamma"] for s in K.SPECS if s["family"] == "gamma"] == [0.0, 1.0]
    assert [s["head_scale"] for s in K.SPECS if s["family"] == "tails"] == [2.0 ** -6] * 10 and all(s["head_scale"] == 1.0 for s in K.SPECS if s["family"] != "tails")
    assert [s["place"] for s in K.SPECS if s["family"] == "single_action"] == ["single_action0", "single_action1"]
    assert K.HUBER_U is QK.HUBER_U and all(float(f32(v)) == v and float(f32(v + 0.5)) == v + 0.5 for v in K.HUBER_U)
    eps = 2.0 ** -20
    assert set(K.HUBER_U) == {0.0, 1.0, -1.0, 1 + eps, -(1 + eps), 1 - eps, -(1 - eps), 0.25, -0.25, 1000.0, -1000.0}
    assert sorted(K.TAIL_REWARDS.tolist()) == [-3, -2.5, -0.25, 0, 0.25, 0.5, 2.5, 3] and set(K.REWARDS.tolist()) != {1.0} and K.REWARDS.min() < 0 < K.REWARDS.max()
    assert np.array_equal(K.REWARDS * 2, np.round(K.REWARDS * 2)) and np.array_equal(K.TAIL_REWARDS * 4, np.round(K.TAIL_REWARDS * 4))   # dyadic
    assert K.KINK_UNITS == dict(h1=(0, 31), h2=(0, 63), emb=(0, 20, 63), te=(0, 41, 63), head=(0, 39, 480, 511)) and K.KINK_ZEROS == 2 * 5 + 2 * 33 + 3 * 65 + 3 * 65 + 4 * 65
    assert set(K.FAMILIES) == set(K.MEASURED) == set(K.BOUND) and len(K.SEEDS) == len(K.SPECS) == 27 and len(K.VARIANTS) == 22
    assert float(K.TAU_TOP) == 1 - 2.0 ** -24 and K.NEAR_ZERO == R.NEAR_ZERO
    from deep_rl_amd import _native_iqn as N
    assert K.MAX_SLABS == N.MAX_SLABS and K.NP == N.NPARAMS and (K.NT, K.NQ) == (N.N_TAU, N.N_QUANT) and N.N_TAU_PRIME == K.NT and K.OFF == N.OFFSETS and K.SIZE == N.SIZES
    for i in CASES:
        assert K.find_seed(i, tries=K.SEEDS[i] + 1) == K.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


def test_the_slab_order_is_the_sibling_files_at_64():
    """sum_rows_slabs restates SUMROWS for MI_IQN_MAX_SLABS = 64; at 128 it is _qrdqn_ref.sum_rows_slabs bit for bit, and on values that add exactly it is the plain sum"""
    rng = np.random.default_rng(3)
    for n in (1, 5, 16, 17, 33, 49, 64, 65, 129, 300):
        v = rng.normal(0, 3, n).astype(f32)
        assert K.sum_rows_slabs(v, 128) == QX.sum_rows_slabs(v)
        ints = rng.integers(-1000, 1000, n).astype(f32)
        assert K.sum_rows_slabs(ints) == ints.sum()
    v = np.zeros(129, f32)                                 # workgroup 0 of 64 adds rows 0, 64, 128 in that order; of 128, rows 0 and 128, and row 64 joins in the slab sum
    v[0], v[64], v[128] = 2.0 ** 24, -2.0 ** 24, 1.0
    assert K.sum_rows_slabs(v) == 1.0 and K.sum_rows_slabs(v, 128) == 0.0


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
    assert np.array_equal(nx, (idx + N) % cap)                                                      # ... which is _iqn_ref.batch_of's rule
    live = e["live"] > 0
    if mb >= 5:
        assert k["wraps"] >= 2 and k["repeats"] >= 1 and k["poisoned"] >= 1
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
    assert np.array_equal(np.isnan(rew[idx]), ~succ[idx]) and k["poisoned"] >= 1                    # (every case here has a row that is nobody's successor)
    # the taus: f32 on the 2^-24 grid inside [0, 1); with >= 5 rows one is exactly 0, one 1 - 2^-24, and one batch row holds the same tau twice
    for name, n in (("taus", K.NT), ("next_taus", K.NQ), ("tau_dashes", K.NT)):
        t = c[name]
        assert t.dtype == f32 and t.shape == (mb, n) and t.min() >= 0 and t.max() < 1 and np.array_equal(t * 16777216.0, np.round(t * 16777216.0))
    if mb >= 5:
        assert (c["taus"] == 0).any() and (c["taus"] == K.TAU_TOP).any() and any(len(np.unique(r)) < K.NT for r in c["taus"])
    if fam == "tau_bands":
        assert c["next_taus"].max() < 0.125 and c["tau_dashes"].min() >= 0.875 and c["taus"].min() < 0.125 and c["taus"].max() > 0.875
        assert set(e["next_actions"].tolist()) == {0, 1} and k["band_flips"] >= 1
        assert (np.argmax(e["q_dash"], axis=1) != e["next_actions"]).sum() == k["band_flips"]      # the argmax over the tau_dashes band is not a* on these rows
    # nothing excluded: the expectation covers every row and is finite
    for key in ("grads", "target", "current", "q"):
        assert np.isfinite(e[key]).all(), key
    assert e["target"].shape == e["current"].shape == (mb, K.NT) and e["next_actions"].shape == (mb,) and e["grads"].shape == (K.NP,) and np.abs(e["grads"]).max() > 0
    assert e["loss"] > 0 and k["zero_gap"] > K.NEAR_ZERO and k["placed_zero"]
    gap = np.abs(e["q"][:, 0] - e["q"][:, 1])
    if fam == "target_tie":
        assert (gap == 0).all() and (e["next_actions"] == 0).all()
        t = c["target"]
        assert np.array_equal(t[K.QW2:K.QW2 + K.HID], t[K.QW2 + K.HID:K.QB2]) and t[K.QB2] == t[K.QB2 + 1]
    else:
        assert gap.min() >= K.CLOSE_Q[fam] == 2 * K.BOUND[fam]["q"] > 0                              # every successor, the terminated ones included
    assert not np.array_equal(c["params"][:K.QW2], c["target"][:K.QW2])                              # an independent draw
    # ---- what the family is named for, in float64
    d = K.pairs(e)
    ad = np.abs(d)
    r_next = rew[nx].astype(np.float64)
    zero = e["grads"] == 0
    zt = lambda name: zero[K.tensor_slice(name)]   # noqa: E731
    if fam != "huber_placed":
        assert np.abs(ad - 1).min() > R.NEAR_KAPPA_REL * K.scale_of(e)                              # no td error where value and slope jump
    if fam == "plain":
        ax = (1, 2)
        assert ((ad <= 1).any(axis=ax) & (ad > 1).any(axis=ax) & (d < 0).any(axis=ax) & (d >= 0).any(axis=ax)).sum() >= 1   # _iqn_ref's mixed_rows condition
        assert c["p_term"] == 1 / 3 and set(rew[nx].tolist()) <= set(K.REWARDS.tolist())
    if fam == "tails":
        assert np.abs(ad - 1).min() >= K.TAIL_KAPPA_GAP == 0.05
        inside = (ad < 1).all(axis=(1, 2))
        assert (inside | (ad > 1).all(axis=(1, 2))).all() and inside.any() and (~inside).any()       # a row lies all inside kappa or all beyond it; the batch holds both
        assert (d < 0).any() and (d > 0).any() and set(rew[nx].tolist()) <= set(K.TAIL_REWARDS.tolist())
        assert np.array_equal(np.ldexp(c["params"][K.QW2:].astype(np.float64), 6).astype(f32).astype(np.float64), np.ldexp(c["params"][K.QW2:].astype(np.float64), 6))
    if fam == "terminal":
        assert (~live).sum() == (mb if c["p_term"] == 1.0 else 0)
    if c["name"] in ("terminal_all_9", "gamma_0_17", "huber_placed_13"):
        assert np.array_equal(e["target"], np.repeat(r_next[:, None], K.NT, axis=1))                # the reward in all 64 places
    if c["name"] == "gamma_0_17":
        assert live.any()                                                                           # on live rows too
    if fam == "huber_placed":
        assert not live.any() and not c["params"][K.QW2:K.QB2].any() and c["params"][K.QB2:].tolist() == [0.0, 0.5]
        b2 = c["params"][K.QB2:].astype(np.float64)
        assert np.array_equal(e["current"], np.repeat(b2[act[idx]][:, None], K.NT, axis=1))         # current is Q.b2 of the stored action
        assert np.array_equal(np.ldexp(r_next, 20), np.round(np.ldexp(r_next, 20)))                 # dyadic
        for v in K.HUBER_U:
            assert (d == v).any(), v                                                                # each edge of the loss is reached, exactly
        assert (d.astype(f32) == d).all()                                                           # and f32 forms the same d: target - current is exact
        assert zero[:K.QW2].all() and zero[:K.QW2].sum() == 43_872 and not zt("QB2").any() and not zt("QW2").all()
        rowloss = (np.abs(c["taus"].astype(np.float64)[:, :, None] - (d < 0)) * np.where(ad <= 1, d * d, ad - 0.5)).sum(axis=(1, 2))
        wsum = np.abs(c["taus"].astype(np.float64)[:, :, None] - (d < 0)).sum(axis=(1, 2))
        at_kappa = np.flatnonzero((ad == 1).all(axis=(1, 2)))
        assert len(at_kappa) >= 2 and np.allclose(rowloss[at_kappa], wsum[at_kappa], rtol=1e-15)     # the loss at d = +-1 has value 1 (times the weights)
    if fam == "kink_placed":
        assert all(np.array_equal(c["units"][s], K.KINK_UNITS[s]) for s in K.SITES) and k["kink_live"]
        for s in K.SITES:
            wk, bk = K.SITE_WB[s]
            u = c["units"][s]
            assert zt(wk).reshape(K.SHAPES[wk])[u].all() and zt(bk)[u].all() and not e["sides"][s][..., u].any()
            assert not c["params"][K.tensor_slice(wk)].reshape(K.SHAPES[wk])[u].any() and not c["params"][K.tensor_slice(bk)][u].any()
        # a unit that is 0 in every row also leaves the next layer's column exactly 0
        assert zt("FW2").reshape(64, 32)[:, [0, 31]].all() and zt("FW3").reshape(64, 64)[:, [0, 63]].all() and zt("QW2").reshape(2, 512)[:, [0, 39, 480, 511]].all()
        assert zt("QW1").reshape(512, 64)[:, [0, 63]].all()                                         # prod_e = emb_e te_e with either factor 0
        assert zero.sum() >= K.KINK_ZEROS
    if fam in K.DEAD_ZERO:
        k_dead = K.DEAD_BIAS[fam]
        assert (c["params"][K.tensor_slice(k_dead)] == -1e3).all() and not e["sides"][dict(FB3="emb", CB="te", QB1="head")[k_dead]].any()
        assert [name for name in K.ORDER if zt(name).all()] == list(K.DEAD_ZERO[fam])                # worked out from the float64 gradient: exactly these tensors
        assert all(zt(name).mean() < 0.9 for name in K.ORDER if name not in K.DEAD_ZERO[fam])
    if fam == "dead_head":
        assert zero.sum() == K.NP - 2 and np.array_equal(e["current"], np.repeat(c["params"][K.QB2:].astype(np.float64)[act[idx]][:, None], K.NT, axis=1))
    if fam == "single_action":
        a = int(c["place"][-1])
        g2, gb2 = zt("QW2").reshape(2, K.HID), zt("QB2")
        assert (act[idx] == a).all() and g2[1 - a].all() and gb2[1 - a] and not g2[a].all() and not gb2[a]
        assert zero.sum() >= K.HID + 1
    elif mb >= 5:
        assert set(act[idx].tolist()) == {0, 1}


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_autograd_agrees_with_the_hand_written_backward(i):
    """float64 against float64: _iqn_ref.update derives forward, targets and backward by hand in numpy, this file's reference by torch autograd"""
    c = K.make_case(i)
    e = c["exp"]
    r = R.update(c["params"], c["target"], K.ringv(c), c["eidx"], c["taus"], c["next_taus"], c["tau_dashes"], gamma=c["gamma"], dtype=np.float64)
    sc = K.scale_of(e)
    assert np.abs(r["q_next"] - e["q"]).max() <= 1e-12 * sc
    if c["family"] != "target_tie":                                                                 # (one 2-column product need not tie bit for bit)
        assert np.array_equal(r["next_actions"], e["next_actions"])
        assert np.abs(r["target"] - e["target"]).max() <= 1e-12 * sc
    else:
        assert np.abs(r["q_next"][:, 0] - r["q_next"][:, 1]).max() <= 1e-12 * sc
    loss, g, cur, fw = R.loss_grad(c["params"], K.batch_of(c)[0], K.batch_of(c)[1], e["target"], c["taus"], dtype=np.float64)
    assert abs(loss - e["loss"]) <= 1e-12 * abs(e["loss"]) and np.abs(cur - e["current"]).max() <= 1e-12 * sc
    assert np.abs(g - e["grads"]).max() <= 1e-11 * np.abs(e["grads"]).max()
    assert max(K.tensor_errors(g, e["grads"]).values()) <= 1e-10                                    # tensor by tensor; all-zero tensors exactly zero
    assert np.array_equal(g == 0, e["grads"] == 0)                                                  # the exact zeros are the same elements
    assert all(np.array_equal(K.sides(fw)[s], e["sides"][s]) for s in K.SITES)


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_f32_picks_the_same_action_and_relu_side_on_every_row(i, f32_eval):
    c, g = K.make_case(i), f32_eval[i]
    e = c["exp"]
    assert np.array_equal(g["next_actions"], e["next_actions"])                                     # no row excluded
    assert all(np.array_equal(g["sides"][s], e["sides"][s]) for s in K.SITES)                       # (a placed unit is exactly 0 in every precision: not > 0)
    e32 = K.evaluate(c, dtype=torch.float32)                                                        # the reference itself in float32: the same a*, the same sides
    s32 = K.sides(e32["pre"])
    assert np.array_equal(e32["next_actions"], e["next_actions"]) and all(np.array_equal(s32[s], e["sides"][s]) for s in K.SITES)
    assert not K.within(K.figures(e, e32), c["family"])                                              # and inside the device bound
    if c["family"] == "kink_placed":
        assert all(not e32["pre"][K.SITE_Z[s]][..., c["units"][s]].any() for s in K.SITES)
    if c["family"] == "target_tie":
        q = g["q"].astype(f32)
        assert np.array_equal(q[:, 0].view(np.uint32), q[:, 1].view(np.uint32)) and not g["next_actions"].any()
        assert np.array_equal(e32["q"][:, 0], e32["q"][:, 1])
    if c["name"] in ("terminal_all_9", "gamma_0_17", "huber_placed_13"):                            # r + 0 * quantile is r, bit for bit
        Rw = K.batch_of(c)[3]
        assert np.array_equal(g["target"].astype(f32).view(np.uint32), np.repeat(Rw[:, None], K.NT, axis=1).view(np.uint32))
    if c["family"] in ("huber_placed", "dead_head"):
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
    assert K.SHIPPED == dict(target=R.BOUND_QUANT_REL, current=R.BOUND_QUANT_REL, q=R.BOUND_Q_ABS, loss=R.BOUND_LOSS_REL, grad=R.BOUND_GRAD_REL, tensor=R.BOUND_GRAD_TENSOR_REL)
    assert K.NO_FLOOR == (("tails", "q"),)
    for fam, w in worst.items():
        print("%-14s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
        for k, v in w.items():
            assert v <= K.MEASURED[fam][k], (fam, k, v)                          # the stored values cover the measurement
            assert K.MEASURED[fam][k] <= 1.25 * v, (fam, k, v)                   # and the table cannot drift loose
            if (fam, k) in K.NO_FLOOR:                                           # narrower than the rule: 8 x MEASURED alone, below the shipped bound
                assert K.BOUND[fam][k] == 8 * K.MEASURED[fam][k] < K.SHIPPED[k]
            else:
                assert K.BOUND[fam][k] == max(8 * K.MEASURED[fam][k], K.SHIPPED[k])  # never below what tests/test_gpu_iqn_cases.py holds the kernel to
        assert K.CLOSE_Q[fam] == 2 * K.BOUND[fam]["q"]
    # tails: under the shipped q bound some successor's action values lie closer than CLOSE_Q would be (the reason for NO_FLOOR)
    gaps = [np.abs(np.diff(_case(n)["exp"]["q"], axis=1)).min() for n in TAILS]
    assert min(gaps) < 2 * R.BOUND_Q_ABS and min(gaps) >= K.CLOSE_Q["tails"]


def test_the_f32_loss_stage_reaches_the_placed_edges(f32_eval):
    """huber_placed in f32: the restatement's d are the placed values exactly, so the device's loss stage runs on both sides of every edge"""
    c = _case("huber_placed_13")
    g = f32_eval[K.NAMES.index("huber_placed_13")]
    d = (g["target"].astype(f32)[:, None, :] - g["current"].astype(f32)[:, :, None]).astype(f32)
    for v in K.HUBER_U:
        assert (d == f32(v)).any(), v
    assert np.array_equal(d.astype(np.float64), K.pairs(c["exp"]))


# variant -> the named cases that catch it; "all": the wrong reading must show on every one of them, "any": on at least one
TEETH = {
    "reward_at_row": (PLAIN + TAILS, "all"),
    "terminated_at_row": (PLAIN + TAILS, "any"),
    "no_wrap": (PLAIN + TAILS, "all"),
    "tie_takes_last": (("target_tie_9",), "all"),
    "stray_action_as_1": (PLAIN + TAILS, "any"),
    "slab_left_out": (("plain_17", "tails_16", "tails_33", "tails_49", "tails_65", "tails_129"), "all"),
    "mean_over_max_slabs": (tuple(n for n in PLAIN + TAILS if n != "tails_64"), "all"),
    "pairs_transposed": (("plain_5", "plain_17") + TAILS, "all"),
    "kappa_strict": (("huber_placed_13",), "all"),
    "huber_halved": (("huber_placed_13", "plain_17") + TAILS, "all"),
    "greedy_by_online_net": (("plain_17",) + TAILS, "all"),
    "greedy_by_tau_dashes": (("tau_bands_17",), "all"),
    "taus_swapped": (("plain_5", "plain_17", "tau_bands_17") + TAILS, "all"),
    "cos_from_k0": (PLAIN + TAILS, "all"),
    "other_action_rows_touched": (("single_action0_9", "single_action1_9"), "all"),
    "relu_one_at_zero_h1": (("kink_placed_8",), "all"),
    "relu_one_at_zero_h2": (("kink_placed_8",), "all"),
    "relu_one_at_zero_emb": (("kink_placed_8",), "all"),
    "relu_one_at_zero_te": (("kink_placed_8",), "all"),
    "relu_one_at_zero_head": (("kink_placed_8",), "all"),
    "last_head_block_left_out": (("plain_5", "plain_17") + TAILS, "all"),
    "tau_row_63_left_out": (("plain_5", "plain_17") + TAILS, "all"),
}
ACTION_VARIANTS = ("tie_takes_last", "greedy_by_online_net", "greedy_by_tau_dashes")


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
    if variant in ACTION_VARIANTS:
        assert kinds == {"actions"}                                              # the a* variants change next_actions
    if variant == "tie_takes_last":
        assert out["target_tie_9"] == ("actions", 9)
    if variant in ("kappa_strict", "huber_halved"):                              # both move the loss of the rows at d == +-1, whose float64 value is 1 per unit weight
        c = _case("huber_placed_13")
        w = K.evaluate(c, variant=variant)
        assert abs(w["loss"] - c["exp"]["loss"]) > K.BOUND["huber_placed"]["loss"] * c["exp"]["loss"]
        assert np.array_equal(w["target"], c["exp"]["target"]) and np.array_equal(w["current"], c["exp"]["current"])
    if variant == "other_action_rows_touched":                                   # non-zero exactly where float64 has the other action's exact zeros
        for name in names:
            c = _case(name)
            a = int(c["place"][-1])
            w = K.evaluate(c, variant=variant)
            assert w["grads"][K.QW2:K.QB2].reshape(2, K.HID)[1 - a].any() and w["grads"][K.QB2 + 1 - a] != 0
            assert w["loss"] == c["exp"]["loss"] and np.array_equal(w["grads"][:K.QW2], c["exp"]["grads"][:K.QW2])   # and nowhere else


@pytest.mark.parametrize("variant", RELU)
def test_a_wrong_sub_gradient_is_caught_by_kink_placed_alone(variant):
    """sub-gradient 1 at exactly 0 shows where float64 holds exact zeros on kink_placed_8 and is bit for bit the right reading on every other case: no other case has a
    pre-activation of exactly 0 at that site (the tails family is represented by its smallest and largest batch)"""
    c = _case("kink_placed_8")
    w = K.evaluate(c, variant=variant)
    assert w["grads"][c["exp"]["grads"] == 0].any() and w["loss"] == c["exp"]["loss"]
    assert K.figures(c["exp"], w)["tensor"] == np.inf or max(K.figures(c["exp"], w)[k] / K.BOUND["kink_placed"][k] for k in K.FIGURES) > 1
    for name in K.NAMES:
        if name == "kink_placed_8" or (name in TAILS and name not in ("tails_16", "tails_129")):
            continue
        c = _case(name)
        w = K.evaluate(c, variant=variant)
        assert np.array_equal(w["grads"], c["exp"]["grads"]) and w["loss"] == c["exp"]["loss"], name


@pytest.mark.parametrize("name", ("plain_5", "bad_index_5", "target_tie_9"))
def test_the_poison_is_never_read(name):
    """replacing any single unreferenced observation or reward by a finite value leaves the expectation bit for bit; a read at the row instead of the successor gives NaN"""
    c = _case(name)
    (N, S), idx, e = c["ring"], c["eidx"], c["exp"]
    cap = N * S
    nx = D.successor(idx, N, S)
    used_obs, used_rew = np.zeros(cap, bool), np.zeros(cap, bool)
    used_obs[idx] = True; used_obs[nx] = True; used_rew[nx] = True
    assert (~used_obs).sum() >= 5 and (~used_rew).sum() >= 10

    def same(w):
        return np.array_equal(w["grads"], e["grads"]) and w["loss"] == e["loss"] and np.array_equal(w["target"], e["target"]) and np.array_equal(w["q"], e["q"])

    for slot in np.flatnonzero(~used_obs):
        obs = c["observations"].copy()
        assert np.isnan(obs.reshape(cap, 4)[slot]).all()
        obs.reshape(cap, 4)[slot] = (0.5, -0.25, 0.1, 1.0)
        assert same(K.evaluate(dict(c, observations=obs))), slot
    for slot in np.flatnonzero(~used_rew):
        rew = c["rewards"].copy()
        assert np.isnan(rew.reshape(cap)[slot])
        rew.reshape(cap)[slot] = 7.0
        assert same(K.evaluate(dict(c, rewards=rew))), slot
    for variant in ("reward_at_row", "no_wrap"):
        assert _wrong(c, variant)[0] == "nan"
    bad = c["observations"].copy()                                               # and a referenced observation IS read
    bad.reshape(cap, 4)[nx[0]] += 0.5
    assert not same(K.evaluate(dict(c, observations=bad)))


def test_the_right_reading_has_no_teeth_marks():
    """the helper itself: the right reading, evaluated again, is bit for bit the expectation"""
    for name in ("plain_5", "kink_placed_8", "huber_placed_13", "tails_33"):
        c = _case(name)
        again = K.evaluate(c)
        assert np.array_equal(again["grads"], c["exp"]["grads"]) and again["loss"] == c["exp"]["loss"] and np.array_equal(again["target"], c["exp"]["target"])
        assert _wrong(c, None)[0] == "figures" and _wrong(c, None)[1] == 0.0
    assert torch.get_default_dtype() == torch.float32
