"""tests/_sac_cases.py validated on the CPU: the cases meet their conditions with no row left out and reach what they claim; the f32 oracle (oracle/cpu_ref.c) is
measured against the float64 autograd reference per family and figure and the constants of _sac_cases.MEASURED are tied to that measurement (device bound = 8 x);
six known-wrong variants of the reference are each separated from the right one by more than 10 x the bound of their case; and the oracle agrees with a torch
FLOAT32 evaluation of the same formulas within the device bounds — so when tests/test_gpu_sac_cases.py fails, a reader knows whether oracle or device is the outlier."""
import numpy as np
import pytest
import torch

import _sac_cases as K

f32 = np.float32
CASES = range(len(K.SPECS))


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    cpu_ref.lib().ref_set_num_threads(8)
    return cpu_ref


def _oracle_tie_action(R):
    a, _ = R.sac_actor_sample(K.tie_actor(), np.array([[1, 0, 0]], f32), np.array([K.TIE_EPS], f32))
    return a[0]


@pytest.fixture(scope="module")
def ties(R):
    return {b: K.finish_tie(K.make_tie_case(b, _oracle_tie_action(R))) for b in K.TIE_BATCHES}


@pytest.fixture(scope="module")
def oracle(R, ties):
    """the oracle's results on every case, computed once: {name: got}"""
    out = {K.make_case(i)["name"]: K.oracle_eval(R, K.make_case(i)) for i in CASES}
    out.update({c["name"]: K.oracle_eval(R, c) for c in ties.values()})
    return out


def _all_cases(ties):
    return [K.make_case(i) for i in CASES] + list(ties.values())


# ---- conditions and reach -----------------------------------------------------------------------------------------------------------
def test_shapes_rings_and_alphas_are_all_present():
    assert {s[2] for s in K.SPECS} == {1, 5, 16, 17, 40}
    assert {s[3] for s in K.SPECS} == {(1, 2), (3, 7), (2, 30)}
    assert {s[4] for s in K.SPECS} == {0.37, 1e-3, 5.0}
    assert {s[1] for s in K.SPECS} == {"A", "B", "C", "AC", "clamp6", "clamp20"}
    for i in CASES:
        assert K.find_seed(i, tries=K.SEEDS[i] + 1) == K.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


@pytest.mark.parametrize("i", CASES)
def test_case_meets_its_conditions_with_no_row_left_out(i):
    c = K.make_case(i)
    k = c["cond"]
    print(c["name"], {a: b for a, b in k.items() if a != "z"})
    assert K.conditions_met(c)
    assert k["max_eps"] <= K.MAX_EPS and k["min_qgap"] > K.Q_MARGIN and k["min_loss"] >= 0.1
    if c["family"] in K.TIGHT:
        assert k["min_preact"] > K.NEAR_ZERO and k["n_preact"] == c["batch"] * 8 * 512       # every unit of every forward pass of every row was looked at
    if c["batch"] >= 5:
        assert k["terminated"] >= 1 and k["wraps"] >= 2
    if (c["n_envs"], c["slots"]) == (1, 2):
        assert k["wraps"] == c["batch"]
    for key in ("eps_critic", "eps_actor", "eps_alpha"):
        assert c[key].shape == (c["batch"],) and c[key].dtype == f32
    e = c["exp"]
    assert all(np.isfinite(e[p][f]).all() for p in ("critic", "actor") for f in ("grads", "logp", "action"))


@pytest.mark.parametrize("i", CASES)
def test_case_reaches_what_it_claims(i, R, oracle):
    c = K.make_case(i)
    z = np.abs(c["cond"]["z"])
    fam, got = c["family"], oracle[c["name"]]
    if fam == "A":
        assert z.max() <= 5 + 1e-6 and (c["batch"] < 5 or (z.max() > 5 - 1e-6 and z.min() < 1e-6))
    if fam == "B":
        assert 6 - 1e-6 <= z.min() and z.max() <= 12 + 1e-6
    if fam == "C":
        assert z.min() >= 16 - 1e-6
        for p in ("critic", "actor", "alpha"):
            assert (np.abs(got[p]["action"]) == 2.0).all()                  # u == +-1 in the f32 oracle, every row
    if fam == "AC":
        for p in ("critic", "actor", "alpha"):
            zz = np.abs(c["exp"][p]["z"])
            assert (zz <= 5 + 1e-6).any() and (zz >= 16 - 1e-6).any() and not ((zz > 5 + 1e-6) & (zz < 16 - 1e-6)).any()
            assert (np.abs(got[p]["action"][zz >= 16 - 1e-6]) == 2.0).all()
    if fam in ("A", "B", "C", "AC"):
        sd, ls = c["exp"]["actor"]["sd"], c["exp"]["actor"]["ls"]
        assert 3.0 < sd.min() and sd.max() < 5.5 and (np.abs(1 - ls * ls - 0.3) < 0.1).all()
        assert (c["cond"]["z"] > 0).any() and (c["batch"] == 1 or (c["cond"]["z"] < 0).any())      # both signs
    if fam in ("clamp6", "clamp20"):
        assert not ((z > K.ILL[0]) & (z < K.ILL[1])).any()
        ls, sd, s = c["exp"]["actor"]["ls"], c["exp"]["actor"]["sd"], np.sign(K.SRAW[c["name"]])
        if fam == "clamp20":      # the clamp's end values, exactly, in float64 and (through the oracle's log-prob) in f32
            assert (ls == s).all() and np.allclose(sd, np.exp(2.0 if s > 0 else -5.0), rtol=1e-15)
            assert (np.tanh(c["exp"]["actor"]["sraw"].astype(f32)) == f32(s)).all()
        else:
            assert (np.abs(ls) < 1).all() and (1 - np.abs(ls) < 2e-5).all() and (np.sign(ls) == s).all()


def test_both_clamp_ends_are_present():
    assert {np.sign(v) * abs(v) for v in K.SRAW.values()} == {6.0, -6.0, 20.0, -20.0}


@pytest.mark.parametrize("batch", K.TIE_BATCHES)
def test_tie_case(batch, R, ties, oracle):
    c = ties[batch]
    t = c["tie_rows"]
    assert K.conditions_met(c) and t.sum() >= 2 and (~t).sum() >= 2 and c["cond"]["terminated"] >= 1 and c["cond"]["wraps"] >= 2
    obs = c["obs"].reshape(-1, 3)[c["idx"]]
    a, _ = R.sac_actor_sample(c["actor"], obs, c["eps_actor"])
    assert (a == c["a"]).all() and c["a"] > 0                                   # zero weights: every row takes the same action
    q1 = R.sac_q_forward(c["q"][:K.SQ_NP], obs, a); q2 = R.sac_q_forward(c["q"][K.SQ_NP:], obs, a)
    assert np.array_equal(q1[t], q2[t]) and (q1[t] == c["a"]).all() and (q2[~t] > q1[~t] + K.Q_MARGIN).all()     # bit-for-bit ties, and clear non-ties
    # the expected routing, stated directly: d(-min Q)/da = -1.5 on the tie rows, -1 on the others
    at = torch.tensor(a.astype(np.float64), requires_grad=True)
    o64 = torch.tensor(obs.astype(np.float64))
    qq1, _ = K.q_forward(torch.tensor(c["q"][:K.SQ_NP].astype(np.float64)), o64, at)
    qq2, _ = K.q_forward(torch.tensor(c["q"][K.SQ_NP:].astype(np.float64)), o64, at)
    tt = torch.tensor(t)
    (-torch.where(tt, 0.5 * qq1 + 0.5 * qq2, torch.minimum(qq1, qq2))).sum().backward()
    assert np.array_equal(at.grad.numpy(), np.where(t, -1.5, -1.0))
    fig = K.figures(c["exp"], oracle[c["name"]])
    assert not K.within(fig, "tie", 1.5 / 8), fig


# ---- the bounds are tied to the measurement -----------------------------------------------------------------------------------------
def test_oracle_against_float64_pins_the_bounds(R, ties, oracle):
    worst = {}
    qerr = 0.0
    for c in _all_cases(ties):
        fig = K.figures(c["exp"], oracle[c["name"]])
        print("%-14s" % c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
        w = worst.setdefault(c["family"], dict.fromkeys(K.FIGURES, 0.0))
        for k, v in fig.items():
            w[k] = max(w[k], v)
        # a critic's value: the online critics at the stored pairs, float64 against the oracle
        obs = c["obs"].reshape(-1, 3)[c["idx"]]; act = c["actions"].reshape(-1)[c["idx"]]
        for k in range(2):
            got = R.sac_q_forward(c["q"][k * K.SQ_NP:(k + 1) * K.SQ_NP], obs, act)
            qerr = max(qerr, float(np.abs(got - c["exp"]["critic"]["q"][k]).max()))
    print("q abs", qerr)
    for fam, w in worst.items():
        print("%-8s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
    assert qerr <= 1.5 * K.MEASURED_Q_ABS and K.Q_MARGIN == 8 * K.MEASURED_Q_ABS
    for fam, w in worst.items():
        for k, v in w.items():
            assert v <= 1.5 * K.MEASURED[fam][k], (fam, k, v)                     # bound / 8 x 1.5
            if fam != "AC":                                                       # (AC borrows the larger of A's and C's)
                assert v >= K.MEASURED[fam][k] / 1.5, (fam, k, v)                 # and no constant sits far above what was measured
            assert K.BOUND[fam][k] == 8 * K.MEASURED[fam][k]
        if fam in K.TIGHT:
            assert w["grad"] <= 1e-5, fam                                         # above that a tight case would be ill conditioned: redesign it, do not widen
    assert set(worst) == set(K.MEASURED)


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
def _departs(c, part, wrong, factor=10.0):
    """the figures of a wrong variant's results, taken as `got` against the right ones -> True when the gradient figure (or, non-finite, any) exceeds factor x bound"""
    fig = K.figures(c["exp"], {part: wrong})
    print(c["name"], part, {k: float("%.3g" % v) for k, v in fig.items()}, "bound", K.BOUND[c["family"]]["grad"])
    return fig["grad"] > factor * K.BOUND[c["family"]]["grad"]


@pytest.mark.parametrize("batch", K.TIE_BATCHES)
@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0)], ids=["1/0", "0/1", "1/1"])
def test_teeth_tie_routing(batch, weights, ties):
    c = ties[batch]
    assert _departs(c, "actor", K.actor_eval(c, tie_weights=weights))


@pytest.mark.parametrize("name", ["A_40", "AC_17", "clamp_p6_17"])
def test_teeth_missing_1e_6(name):
    c = K.make_case([s[0] for s in K.SPECS].index(name))
    assert _departs(c, "actor", K.actor_eval(c, variant="no_1e-6"))


@pytest.mark.parametrize("name", ["A_40", "clamp_p6_17", "clamp_m6_16", "clamp_p20_5", "clamp_m20_40"])
def test_teeth_clamp_derivative_dropped(name):
    c = K.make_case([s[0] for s in K.SPECS].index(name))
    assert _departs(c, "actor", K.actor_eval(c, variant="clamp_derivative_dropped"))


@pytest.mark.parametrize("i", [i for i in CASES if K.SPECS[i][2] >= 5 and K.SPECS[i][1] != "B"])
def test_teeth_terminated_ignored(i):
    c = K.make_case(i)
    assert _departs(c, "critic", K.critic_eval(c, variant="term_ignored"))


@pytest.mark.parametrize("i", [i for i in CASES if K.SPECS[i][1] not in ("B", "clamp20")])
def test_teeth_alpha_c_term_dropped(i):
    """(not on clamp20: there the term passes through d ls / d sraw == 0 and drops out of every gradient, rightly)"""
    c = K.make_case(i)
    assert _departs(c, "actor", K.actor_eval(c, variant="alpha_c_dropped"))


# ---- oracle against torch float32 ---------------------------------------------------------------------------------------------------
# (case, figure) at which torch's plain f32 autograd misses the device bound AGAINST FLOAT64 by itself: {case: {figure: torch f32 against float64}}, measured.
# Cause: torch's f32 tanh backward forms 1 - u^2 with one rounding, the forward's log term holds the twice-rounded 1 - u u; the two appear as a ratio
# (1 - u^2) / (2 (1 - u u) + 1e-6) in d logp / dz, and where 1 - u^2 ~ 1e-4 (|z| ~ 5) their 3e-8 difference is 1e-4 of that row's gradient.  The oracle and the
# kernels use ONE product in both places; the oracle is 2.8e-7 (A_40) and 9.1e-7 (clamp_p6_17) from float64 on the same figure.
TORCH_F32_IS_THE_OUTLIER = {"A_40": {"grad": 1.91e-5}, "clamp_p6_17": {"grad": 9.78e-5, "tensor": 2.61e-2}}


def _eval32(c, variant=None):
    tw = (0.5, 0.5) if c["family"] == "tie" else None
    return dict(critic=K.critic_eval(c, torch.float32), actor=K.actor_eval(c, torch.float32, variant=variant, tie_weights=tw), alpha=K.alpha_eval(c, c["log_alpha"], torch.float32))


def test_oracle_agrees_with_torch_float32(ties, oracle):
    """The same formulas evaluated by torch in float32 (its own summation orders, its own tanh / exp / log) against the oracle, under the DEVICE bounds, every case
    and figure: so a device that misses a bound against float64 — and against this — is the outlier, not the oracle.
    Plain f32 autograd: within the bounds everywhere except the three (case, figure) pairs of TORCH_F32_IS_THE_OUTLIER, where torch's f32 is itself outside the
    bound against float64 (asserted, with the oracle inside 1.5 / 8 of it there): not a disagreement the oracle is part of.
    With tanh's slope taken from the forward's own product (the one difference, see _sac_cases.actor_forward): within the bounds on EVERY case and figure."""
    seen = {}
    for c in _all_cases(ties):
        fam = c["family"]
        e32 = _eval32(c)
        over = K.within(K.figures(e32, oracle[c["name"]]), fam)
        if over:
            t64, o64 = K.figures(c["exp"], e32), K.figures(c["exp"], oracle[c["name"]])
            for k in over:
                assert t64[k] > K.BOUND[fam][k] and o64[k] <= 1.5 * K.MEASURED[fam][k], (c["name"], k, over[k], t64[k], o64[k])
                seen.setdefault(c["name"], {})[k] = t64[k]
        fig = K.figures(_eval32(c, "slope_from_forward_product"), oracle[c["name"]])
        print("%-14s" % c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
        assert not K.within(fig, fam), (c["name"], K.within(fig, fam))
    print(seen)
    assert {n: set(v) for n, v in seen.items()} == {n: set(v) for n, v in TORCH_F32_IS_THE_OUTLIER.items()}
    for n, v in TORCH_F32_IS_THE_OUTLIER.items():
        for k, x in v.items():
            assert x / 1.5 <= seen[n][k] <= 1.5 * x
