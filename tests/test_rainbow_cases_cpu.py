"""tests/_rainbow_cases.py and tests/_rainbow_ref.py validated on the CPU, before tests/test_gpu_rainbow_cases.py leans on them: the restatement of the draw is the
header's (counter layout, factor meanings, the element products) and is MEASURED against its float64 form; every case meets its conditions with no row left out,
rides on its tests/_nstep_cases.py ring untouched and carries the distributional edges its ring is named for; the float32 evaluation picks the same a* on every
row and is MEASURED against float64 per family and figure, with _rainbow_ref.MEASURED tied to that measurement; each deliberately wrong reading leaves a bound (or
an exact a*) on EVERY case it applies to; and the 51-update chain is measured the same way."""
import numpy as np
import pytest
import torch

import _nstep_cases as K
import _rainbow_cases as C
import _rainbow_ref as Z
from _reinforce_ref import philox

f32 = np.float32
CASES = range(len(C.SPECS))


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
    """the float32 evaluation of every case, computed once (on one thread, see one_thread)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return [Z.evaluate(C.make_case(i), torch.float32) for i in CASES]
    finally:
        torch.set_num_threads(n)


def test_layout_families_and_seeds():
    from deep_rl_amd import _native_rb as N

    assert (Z.NP, Z.HEAD, Z.BV, Z.WA, Z.BA, Z.SIGMA, Z.NHEAD, Z.NXI, Z.NROWS, Z.NA) == (N.NPARAMS, N.OFF_WV, N.OFF_BV, N.OFF_WA, N.OFF_BA, N.OFF_SIGMA, N.NHEAD, N.NXI,
                                                                                         N.NROWS, N.N_ATOMS)
    assert (Z.STREAM_ACT, Z.STREAM_LEARN) == (N.STREAM_ACT, N.STREAM_LEARN) == (13, 14)
    assert C.NAMES is K.NAMES and C.SPECS is K.SPECS and len(C.NAMES) == 14 == len(C.SEEDS) and set(C.FAMILY_OF) == set(K.NAMES) == set(C.SUPPORT)
    assert set(C.FAMILY_OF.values()) == set(Z.FAMILIES) == set(Z.MEASURED) == set(C.SCALE) and len(Z.FAMILIES) == 6
    shapes = {(s["mb"], s["n_step"], s["ring"]) for s in K.SPECS if C.FAMILY_OF[s["name"]] in C.NOISY_FAMILIES}
    assert {(1, 1, (1, 2)), (12, 2, (5, 7)), (13, 3, (5, 7)), (17, 5, (4, 12)), (129, 3, (4, 30)), (300, 16, (129, 40))} <= shapes     # every shape carries live noise
    assert len(C.noisy_cases()) == 10 and len(Z.VARIANTS) == 11
    for edge in ("clamp_lo", "clamp_hi", "on_atom", "one_atom"):
        assert sum(edge in v for v in C.EDGES.values()) >= 2                                             # every edge is placed on more than one ring
    for i in CASES:
        assert C.find_seed(i, tries=C.SEEDS[i] + 1) == C.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------------
def test_draw_restates_the_header():
    seed, a, b = 0x1234_5678_9ABC, 7, (1 << 40) + 5
    z = Z.normal(seed, a, b, 14)
    assert z.shape == (321,) and z.dtype == f32
    for c in (0, 83, 84, 134, 135, 218, 219, 320):                      # one Philox call per number, keyed b * 512 + c, words 0 and 1
        r = philox(seed, np.uint64(a), np.uint64(b * 512 + c), 14)
        u1 = (f32(r[0] >> 8) + f32(0.5)) * f32(2.0 ** -24)
        u2 = f32(r[1] >> 8) * f32(2.0 ** -24)
        assert z[c] == np.sqrt(f32(-2) * np.log(u1)) * np.cos(f32(6.28318530717958647692) * u2)
    x = Z.xi_of(z)
    assert np.array_equal(x, np.sign(z) * np.sqrt(np.abs(z)))
    fin, fout = Z.factors(x)
    assert fin.shape == (153, 84) and fout.shape == (153,) and fin.dtype == fout.dtype == f32
    assert all(np.array_equal(fin[r], x[:84]) for r in (0, 50)) and all(np.array_equal(fin[r], x[135:219]) for r in (51, 101, 102, 152))
    assert np.array_equal(fout[:51], x[84:135]) and np.array_equal(fout[51:], x[219:321])               # advantage outputs indexed a * 51 + j
    e = Z.eps_of(fin, fout)
    assert e.shape == (13005,) and e.dtype == f32
    assert np.array_equal(e[:4284].reshape(51, 84), x[84:135, None] * x[None, :84]) and np.array_equal(e[4284:4335], x[84:135])                  # Wv, bv
    assert np.array_equal(e[4335:12903].reshape(102, 84), x[219:321, None] * x[None, 135:219]) and np.array_equal(e[12903:], x[219:321])         # Wa, ba
    for other in (Z.normal(seed, a, b, 13), Z.normal(seed, a + 1, b, 14), Z.normal(seed, a, b + 1, 14), Z.normal(seed + 1, a, b, 14)):
        assert not np.array_equal(other, z) and np.abs(np.corrcoef(other, z)[0, 1]) < 0.3
    many = Z.normal(seed, np.arange(4)[:, None], np.arange(3)[None, :], 14)
    assert many.shape == (4, 3, 321) and np.array_equal(many[2, 1], Z.normal(seed, 2, 1, 14))


def test_draw_is_measured_against_float64_and_is_standard_normal():
    u = np.arange(Z.DRAW_SAMPLES, dtype=np.uint64)
    z32, z64 = Z.normal(99, u, 0, 14), Z.normal(99, u, 0, 14, np.float64)
    x = Z.xi_of(z32)
    back = (x * np.abs(x)).astype(np.float64)
    d = float(np.abs(back - z64).max())
    print("draw: xi |xi| against float64 z over %d samples: %.3g; max |z| %.3g" % (Z.DRAW_SAMPLES, d, np.abs(z64).max()))
    assert d <= Z.MEASURED_DRAW["z"] <= 1.25 * d and Z.BOUND_DRAW["z"] == 8 * Z.MEASURED_DRAW["z"]
    n = z64.size
    assert abs(z64.mean()) <= 5 / np.sqrt(n) and abs(z64.var() - 1) <= 5 * np.sqrt(2.0 / n)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=C.NAMES)
def test_case_meets_its_conditions_with_no_row_left_out(i):
    c, base = C.make_case(i), K.make_case(i)
    k, e, fam = c["cond"], c["exp"], c["family"]
    print(c["name"], fam, c["support"], k)
    assert C.conditions_met(c)
    for key in ("observations", "actions", "rewards", "terminated", "idx", "weights"):
        assert c[key] is base[key]                                                                       # the ring is the n-step case's own
    assert (c["n_step"], c["head"], c["gamma"], c["mb"]) == (base["n_step"], base["head"], base["gamma"], base["mb"])
    assert c["params"].dtype == f32 and c["params"].shape == c["target"].shape == (Z.NP,)
    assert np.array_equal(c["params"][:Z.TORSO], base["params"][:Z.TORSO]) and np.array_equal(c["target"][:Z.TORSO], base["target"][:Z.TORSO]) or fam == "synced"
    lo, hi = c["support"]
    assert np.isfinite([lo, hi]).all() and lo < hi
    sg, st = c["params"][Z.SIGMA:], c["target"][Z.SIGMA:]
    d = f32(0.5 / np.sqrt(84)) * f32(C.SCALE[fam])
    if fam == "sigma_0":
        assert not sg.any() and not st.any() and c["noisy"] == 1
    else:
        assert sg.min() >= 0.5 * d * 0.999 and sg.max() <= 1.5 * d * 1.001 and len(np.unique(sg)) > 10000
    assert c["noisy"] == (0 if fam == "off" else 1)
    if fam == "synced":
        assert np.array_equal(c["params"], c["target"]) and not np.array_equal(c["e_on"], c["e_tg"])
        assert np.abs(e["q_next"] - e["q_target"]).max(axis=1).min() > Z.CLOSE_Q[fam]                    # equal parameters, two samples: the two networks differ on every row
    elif fam != "sigma_0":
        assert not np.array_equal(sg, st)
    if fam == "weights_zero":
        assert (c["weights"] == 0).sum() == 1 and c["weights"].max() == 1
    if c["name"] in C.HEAD_SCALE:                                                                        # saturated: the 1e-8 decides logf on some atom of some row
        assert e["probs"].min() < 1e-8 and np.abs(c["params"][Z.HEAD:Z.SIGMA]).max() > 20 / np.sqrt(84)
    for key in ("e_on", "e_tg", "e_alt"):
        assert c[key].shape == (Z.NHEAD,) and c[key].dtype == f32 and np.isfinite(c[key]).all()
    assert np.array_equal(c["e_on"], Z.eps(c["noise_seed"], c["u"], 0, 14)) and np.array_equal(c["e_tg"], Z.eps(c["noise_seed"], c["u"], 1, 14))
    # nothing excluded: the expectation covers every row and is finite although the ring is NaN-poisoned beyond every walk's stop; the walk is the n-step case's
    assert np.isnan(c["rewards"]).any()
    for key in ("grads", "target_probs", "probs", "prio", "q_next", "q_target", "q_row"):
        assert np.isfinite(e[key]).all(), key
    assert np.array_equal(e["horizon"], base["exp"]["horizon"]) and np.array_equal(e["at"], base["exp"]["at"]) and e["grads"].shape == (Z.NP,)
    assert np.abs(e["target_probs"].sum(axis=1) - 1).max() < 1e-12 and e["target_probs"].min() >= 0 and e["target_probs"].shape == (c["mb"], 51)
    gap = np.abs(e["q_next"][:, 0] - e["q_next"][:, 1])
    assert gap.min() >= Z.CLOSE_Q[fam] == 2 * Z.BOUND[fam]["q"] and abs(e["loss"]) >= C.LOSS_FLOOR       # every bootstrap observation: the share left out is 0
    if c["mb"] > 1:
        assert set(e["next_actions"][e["live"] > 0].tolist()) == {0, 1}
    if fam in C.NOISY_FAMILIES:
        assert k["alt_flips"] >= 1 and np.abs(e["grads"][Z.SIGMA:]).max() > 0
    if fam == "off":
        assert not e["grads"][Z.SIGMA:].any()                                                            # exact zeros
    if fam == "sigma_0":                                                                                 # the mean network's values, a sigma gradient of g * eps
        assert np.abs(e["grads"][Z.SIGMA:] - e["grads"][Z.HEAD:Z.SIGMA] * c["e_on"].astype(np.float64)).max() <= 1e-12 * np.abs(e["grads"]).max() and e["grads"][Z.SIGMA:].any()
    for edge in C.EDGES.get(c["name"], ()):
        assert k[edge] >= 1, edge
    assert (e["prio"] >= 0).all() and np.abs(e["prio"].max() - max(0.0, e["prio"].max())) == 0


def test_the_placed_edges_are_what_their_names_say():
    c = C.make_case(C.NAMES.index("weights_span_17"))
    e = c["exp"]
    lo, hi = c["support"]
    z = lo + (hi - lo) / 50 * np.arange(51)
    tz = e["R"][:, None] + e["lg"][:, None] * z[None, :]
    assert np.array_equal(e["at_lo"] > 0, np.clip(tz, lo, hi) == lo) and (tz < lo).any() and (tz > hi).any()
    term = e["lg"] == 0
    rows = np.where(term & (e["same"].all(axis=1)))[0]
    assert len(rows) >= 1
    for r in rows:                                                                                       # a terminal row beyond the support: one atom takes everything
        k = 0 if e["R"][r] <= lo else 50
        assert e["R"][r] <= lo or e["R"][r] >= hi
        assert abs(e["target_probs"][r, k] - 1) < 1e-12 and (np.delete(e["target_probs"][r], k) == 0).all()


@pytest.mark.parametrize("i", CASES, ids=C.NAMES)
def test_f32_takes_the_same_walk_and_action_on_every_row(i, f32_eval):
    e, g = C.make_case(i)["exp"], f32_eval[i]
    assert np.array_equal(g["next_actions"], e["next_actions"]) and np.array_equal(g["horizon"], e["horizon"]) and np.array_equal(g["at"], e["at"])


def test_measured_is_what_float32_gives_against_float64(f32_eval):
    worst = {}
    for i in CASES:
        c = C.make_case(i)
        fig = Z.figures(c["exp"], f32_eval[i])
        print("%-18s %-12s" % (c["name"], c["family"]), {k: float("%.3g" % v) for k, v in fig.items()})
        assert set(fig) == set(Z.FIGURES)
        w = worst.setdefault(c["family"], {})
        for k, v in fig.items():
            w[k] = max(w.get(k, 0.0), v)
    assert Z.BAR == dict(loss=2e-5, grad=1e-5, grad_sigma=1e-5)
    for fam, w in worst.items():
        print("%-12s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
        for k, v in w.items():
            assert v <= Z.MEASURED[fam][k], (fam, k, v)                          # the stored values cover the measurement
            assert Z.MEASURED[fam][k] <= 1.25 * v, (fam, k, v)                   # and the table cannot drift loose
            assert Z.BOUND[fam][k] == max(8 * Z.MEASURED[fam][k], Z.BAR.get(k, 0.0))
        assert set(Z.BOUND[fam]) == set(Z.FIGURES) and all(Z.BOUND[fam][k] == 8 * Z.MEASURED[fam][k] for k in ("probs", "q", "target_probs", "prio"))   # no bar on these
    assert worst["off"]["grad_sigma"] == 0.0 == Z.MEASURED["off"]["grad_sigma"]


MIN_APPLIES = dict(no_noise=10, target_shares_online_sample=10, argmax_by_target_net=8, one_step_projection=8, projection_unclamped=8, l_equals_u_mass_dropped=8,
                   dueling_mean_missing=14, weights_ignored=1, priority_weighted=1, sigma_grad_unscaled=10, eps_inside_softmax_not_log=1)


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_a_wrong_reading_leaves_a_bound_on_every_case_it_applies_to(variant):
    """a figure beyond its bound, or an a* that differs: the device test compares next_actions exactly"""
    out = {}
    for i in CASES:
        c = C.make_case(i)
        if not C.applies(variant, c):
            continue
        wrong = Z.evaluate(c, variant=variant)
        fig = Z.figures(c["exp"], wrong)
        b = Z.BOUND[c["family"]]
        worst = max((fig[k] / b[k]) if b[k] > 0 else (np.inf if fig[k] > 0 else 0.0) for k in Z.FIGURES)
        out[c["name"]] = np.inf if not np.array_equal(wrong["next_actions"], c["exp"]["next_actions"]) else worst
    print(variant, {k: float("%.3g" % v) for k, v in out.items()})
    assert len(out) >= MIN_APPLIES[variant] and min(out.values()) > 1


def test_what_only_one_figure_tells():
    c = C.make_case(C.NAMES.index("weights_span_17"))
    w = Z.evaluate(c, variant="sigma_grad_unscaled")
    fig = Z.figures(c["exp"], w)
    assert all(fig[k] == 0 for k in Z.FIGURES if k != "grad_sigma") and fig["grad_sigma"] > Z.BOUND[c["family"]]["grad_sigma"]
    w = Z.evaluate(c, variant="priority_weighted")
    fig = Z.figures(c["exp"], w)
    assert all(fig[k] == 0 for k in Z.FIGURES if k != "prio") and fig["prio"] > Z.BOUND[c["family"]]["prio"]
    assert np.array_equal(w["prio"], c["exp"]["prio"] * c["weights"].astype(np.float64))                 # the right priority is the UNWEIGHTED row loss


def test_chain_of_51_noisy_weighted_updates_is_measured(R, one_thread):
    ring, indices, weights, params, target, pairs = Z.chain_data(R)
    assert indices.shape == weights.shape == (Z.CHAIN_UPDATES, Z.CHAIN_BATCH) and params.shape == target.shape == (Z.NP,) and len(pairs) == 51
    assert not np.array_equal(pairs[0][0], pairs[0][1]) and not np.array_equal(pairs[0][0], pairs[1][0])
    head = Z.CHAIN_STEPS
    l64, p64 = Z.chain(ring, indices, weights, params, target, Z.CHAIN_N, head, Z.CHAIN_SUPPORT, pairs)
    l32, p32 = Z.chain(ring, indices, weights, params, target, Z.CHAIN_N, head, Z.CHAIN_SUPPORT, pairs, torch.float32)
    fl, fp = float((np.abs(l32 - l64) / np.abs(l64)).max()), float(np.abs(p32 - p64).max())
    print("chain: loss rel %.3g, params abs %.3g; losses %.4f .. %.4f" % (fl, fp, l64[0], l64[-1]))
    assert np.abs(p64 - params)[:Z.SIGMA].max() > 20 * Z.LR and np.abs(p64 - params)[Z.SIGMA:].max() > 20 * Z.LR      # the means moved, and the sigmas
    for v, key in ((fl, "loss"), (fp, "params")):
        assert v <= Z.MEASURED_CHAIN[key] <= 1.25 * v, (key, v)
    assert Z.BOUND_CHAIN == dict(loss=max(8 * Z.MEASURED_CHAIN["loss"], Z.BAR["loss"]), params=8 * Z.MEASURED_CHAIN["params"])
    assert Z.CHAIN_UPDATES == 51 and Z.CHAIN_N == 3 and Z.CHAIN_SUPPORT == (0.0, 100.0)
