"""tests/_noisy_cases.py and tests/_noisy_ref.py validated on the CPU, before tests/test_gpu_noisy_cases.py leans on them: the restatement of the draw is the
header's (counter layout, factor meanings, f, the element products) and is MEASURED against its float64 form; every case meets its conditions with no row left
out and rides on its tests/_nstep_cases.py ring untouched; the float32 evaluation picks the same a* on every row and is MEASURED against float64 per family and
figure, with _noisy_ref.MEASURED tied to that measurement; each deliberately wrong reading leaves a bound on EVERY noisy case; with noisy = 0, and with sigma == 0 in
everything but the sigma gradient, the restatement IS tests/_nstep_ref.py's; and the 51-update chain is measured the same way."""
import numpy as np
import pytest
import torch

import _noisy_cases as C
import _noisy_ref as Z
import _nstep_cases as K
import _nstep_ref as X
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
    from deep_rl_amd import _native_nz as N

    assert (Z.NP, Z.NP_MEAN, Z.HEAD, Z.SIGMA, Z.NHEAD, Z.NXI) == (N.NPARAMS, 11019, N.OFF_WV, N.OFF_SIGMA, N.NHEAD, N.NXI) == (11274, 11019, 10764, 11019, 255, 171)
    assert (Z.STREAM_ACT, Z.STREAM_LEARN) == (N.STREAM_ACT, N.STREAM_LEARN) == (13, 14)
    assert C.NAMES is K.NAMES and C.SPECS is K.SPECS and len(C.NAMES) == 14 == len(C.SEEDS) and set(C.FAMILY_OF) == set(K.NAMES)
    assert set(C.FAMILY_OF.values()) == set(Z.FAMILIES) == set(Z.MEASURED) == set(C.SCALE) and len(Z.FAMILIES) == 6
    shapes = {(s["mb"], s["n_step"], s["ring"]) for s in K.SPECS if C.FAMILY_OF[s["name"]] in C.NOISY_FAMILIES}
    assert {(1, 1, (1, 2)), (12, 2, (5, 7)), (13, 3, (5, 7)), (17, 5, (4, 12)), (129, 3, (4, 30)), (300, 16, (129, 40))} <= shapes     # every shape carries live noise
    assert C.FAMILY_OF["synced_17"] == "synced" and C.FAMILY_OF["weights_span_17"] == "weights_zero" and len(C.noisy_cases()) == 10
    for i in CASES:
        assert C.find_seed(i, tries=C.SEEDS[i] + 1) == C.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------------
def test_draw_restates_the_header():
    seed, a, b = 0x1234_5678_9ABC, 7, (1 << 40) + 5
    z = Z.normal(seed, a, b, 14)
    assert z.shape == (171,) and z.dtype == f32
    for c in (0, 84, 85, 170):                                          # one Philox call per number, keyed b * 256 + c, words 0 and 1
        r = philox(seed, np.uint64(a), np.uint64(b * 256 + c), 14)
        u1 = (f32(r[0] >> 8) + f32(0.5)) * f32(2.0 ** -24)
        u2 = f32(r[1] >> 8) * f32(2.0 ** -24)
        assert z[c] == np.sqrt(f32(-2) * np.log(u1)) * np.cos(f32(6.28318530717958647692) * u2)
    x = Z.xi_of(z)
    assert np.array_equal(x, np.sign(z) * np.sqrt(np.abs(z))) and np.array_equal(np.sign(x), np.sign(z))
    e = Z.eps_of(x)
    assert e.shape == (255,) and e.dtype == f32
    assert np.array_equal(e[:84], x[84] * x[:84]) and e[84] == x[84]                                   # Wv[k], bv
    for j in range(2):
        assert np.array_equal(e[85 + 84 * j:85 + 84 * (j + 1)], x[169 + j] * x[85:169]) and e[253 + j] == x[169 + j]   # Wa[j][k], ba[j]
    te = Z.eps_of(torch.from_numpy(x.astype(np.float64))).numpy()
    assert np.abs(te - e).max() <= 4e-7 * np.abs(e).max()                                              # the torch path lays the same factors
    # other keys, other samples: the stream, a, b and the seed all enter
    for other in (Z.normal(seed, a, b, 13), Z.normal(seed, a + 1, b, 14), Z.normal(seed, a, b + 1, 14), Z.normal(seed + 1, a, b, 14)):
        assert not np.array_equal(other, z) and np.abs(np.corrcoef(other, z)[0, 1]) < 0.3
    many = Z.normal(seed, np.arange(4)[:, None], np.arange(3)[None, :], 14)
    assert many.shape == (4, 3, 171) and np.array_equal(many[2, 1], Z.normal(seed, 2, 1, 14))


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
    print(c["name"], fam, k)
    assert C.conditions_met(c)
    for key in ("observations", "actions", "rewards", "terminated", "idx", "weights"):
        assert c[key] is base[key]                                                                       # the ring is the n-step case's own
    assert (c["n_step"], c["head"], c["gamma"], c["mb"]) == (base["n_step"], base["head"], base["gamma"], base["mb"])
    assert c["params"].dtype == f32 and c["params"].shape == c["target"].shape == (Z.NP,)
    assert np.array_equal(c["params"][:Z.NP_MEAN], base["params"]) and np.array_equal(c["target"][:Z.NP_MEAN], base["target"])
    sg, st = c["params"][Z.SIGMA:], c["target"][Z.SIGMA:]
    d = f32(0.5 / np.sqrt(84)) * f32(C.SCALE[fam])
    if fam == "sigma_0":
        assert not sg.any() and not st.any() and c["noisy"] == 1
    else:
        assert sg.min() >= 0.5 * d * 0.999 and sg.max() <= 1.5 * d * 1.001 and len(np.unique(sg)) > 200
    assert c["noisy"] == (0 if fam == "off" else 1)
    if fam == "synced":
        assert np.array_equal(c["params"], c["target"]) and not np.array_equal(c["xi_on"], c["xi_tg"])
        assert np.abs(e["q_next"] - e["q_target"]).max(axis=1).min() > Z.CLOSE_Q[fam]                                # equal parameters, two samples: the two networks differ on every row
    elif fam != "sigma_0":
        assert not np.array_equal(sg, st)
    if fam == "weights_zero":
        assert (c["weights"] == 0).sum() == 1 and c["weights"].max() == 1
    for key in ("xi_on", "xi_tg", "xi_alt"):
        assert c[key].shape == (171,) and c[key].dtype == f32 and np.isfinite(c[key]).all()
    assert np.array_equal(c["xi_on"], Z.xi(c["noise_seed"], c["u"], 0, 14)) and np.array_equal(c["xi_tg"], Z.xi(c["noise_seed"], c["u"], 1, 14))
    # nothing excluded: the expectation covers every row and is finite; the walk is the n-step case's
    for key in ("grads", "target", "current", "td_abs", "q_next", "q_target", "q_row"):
        assert np.isfinite(e[key]).all(), key
    assert np.array_equal(e["horizon"], base["exp"]["horizon"]) and np.array_equal(e["at"], base["exp"]["at"]) and e["grads"].shape == (Z.NP,)
    gap = np.abs(e["q_next"][:, 0] - e["q_next"][:, 1])
    assert gap.min() >= Z.CLOSE_Q[fam] == 2 * Z.BOUND[fam]["q"] and abs(e["loss"]) >= C.LOSS_FLOOR       # every bootstrap observation: the share left out is 0
    if c["mb"] > 1:
        assert set(e["next_actions"][e["live"] > 0].tolist()) == {0, 1}
    if fam in C.NOISY_FAMILIES:
        assert k["alt_flips"] >= 1 and np.abs(e["grads"][Z.SIGMA:]).max() > 0
    if fam == "off":
        assert not e["grads"][Z.SIGMA:].any()                                                            # exact zeros
        n = X.evaluate(base)
        for key in ("target", "current", "td_abs", "next_actions", "q_next", "q_target", "q_row"):
            assert np.array_equal(e[key], n[key]), key
        assert e["loss"] == n["loss"] and np.array_equal(e["grads"][:Z.NP_MEAN], n["grads"])             # noisy = 0 IS the n-step restatement
    if fam == "sigma_0":                                                                                 # the mean network's values, a sigma gradient of g * eps
        n = X.evaluate(base)
        assert np.array_equal(e["target"], n["target"]) and np.array_equal(e["grads"][:Z.NP_MEAN], n["grads"])
        eps = Z.eps_of(c["xi_on"].astype(np.float64))
        assert np.abs(e["grads"][Z.SIGMA:] - e["grads"][Z.HEAD:Z.SIGMA] * eps).max() <= 1e-12 * np.abs(e["grads"]).max() and e["grads"][Z.SIGMA:].any()


@pytest.mark.parametrize("i", CASES, ids=C.NAMES)
def test_f32_takes_the_same_walk_and_action_on_every_row(i, f32_eval):
    e, g = C.make_case(i)["exp"], f32_eval[i]
    assert np.array_equal(g["next_actions"], e["next_actions"]) and np.array_equal(g["horizon"], e["horizon"]) and np.array_equal(g["at"], e["at"])


def test_measured_is_what_float32_gives_against_float64(f32_eval):
    worst = {}
    for i in CASES:
        c = C.make_case(i)
        fig = Z.figures(c["exp"], f32_eval[i], c["ring_family"])
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
        assert set(Z.BOUND[fam]) == set(Z.FIGURES) and all(Z.BOUND[fam][k] == 8 * Z.MEASURED[fam][k] for k in ("q", "target", "current", "td_abs"))   # no bar on these
    assert worst["off"]["grad_sigma"] == 0.0 == Z.MEASURED["off"]["grad_sigma"]


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_a_wrong_reading_leaves_a_bound_on_every_noisy_case(variant):
    """a figure beyond its bound, or an a* that differs: the device test compares next_actions exactly"""
    out = {}
    for i in C.noisy_cases():
        c = C.make_case(i)
        wrong = Z.evaluate(c, variant=variant)
        fig = Z.figures(c["exp"], wrong, c["ring_family"])
        worst = max(fig[k] / Z.BOUND[c["family"]][k] for k in Z.FIGURES)
        out[c["name"]] = np.inf if not np.array_equal(wrong["next_actions"], c["exp"]["next_actions"]) else worst
    print(variant, {k: float("%.3g" % v) for k, v in out.items()})
    assert len(out) == 10 and min(out.values()) > 1


def test_only_the_sigma_gradient_tells_the_two_scalings():
    """sigma_grad_unscaled and sigma_grad_by_xi_not_eps leave every other figure untouched"""
    c = C.make_case(C.NAMES.index("plain_13_n3"))
    for variant in ("sigma_grad_unscaled", "sigma_grad_by_xi_not_eps"):
        w = Z.evaluate(c, variant=variant)
        fig = Z.figures(c["exp"], w, c["ring_family"])
        assert all(fig[k] == 0 for k in Z.FIGURES if k != "grad_sigma") and fig["grad_sigma"] > Z.BOUND[c["family"]]["grad_sigma"]
    w = Z.evaluate(c, variant="sigma_grad_by_xi_not_eps")
    bias = np.array([84, 253, 254])
    assert np.array_equal(w["grads"][Z.SIGMA + bias], c["exp"]["grads"][Z.SIGMA + bias])                 # a bias's eps IS its output factor


def test_chain_of_51_noisy_weighted_updates_is_measured(R, one_thread):
    ring, indices, weights, params, target, pairs = Z.chain_data(R)
    assert indices.shape == weights.shape == (Z.CHAIN_UPDATES, Z.CHAIN_BATCH) and params.shape == target.shape == (Z.NP,) and len(pairs) == 51
    assert not np.array_equal(pairs[0][0], pairs[0][1]) and not np.array_equal(pairs[0][0], pairs[1][0])
    head = Z.CHAIN_STEPS
    l64, p64 = Z.chain(ring, indices, weights, params, target, Z.CHAIN_N, head, pairs)
    l32, p32 = Z.chain(ring, indices, weights, params, target, Z.CHAIN_N, head, pairs, torch.float32)
    fl, fp = float((np.abs(l32 - l64) / np.abs(l64)).max()), float(np.abs(p32 - p64).max())
    print("chain: loss rel %.3g, params abs %.3g; losses %.4f .. %.4f" % (fl, fp, l64[0], l64[-1]))
    assert np.abs(p64 - params)[:Z.NP_MEAN].max() > 20 * Z.LR and np.abs(p64 - params)[Z.SIGMA:].max() > 20 * Z.LR      # the means moved, and the sigmas
    for v, key in ((fl, "loss"), (fp, "params")):
        assert v <= Z.MEASURED_CHAIN[key] <= 1.25 * v, (key, v)
    assert Z.BOUND_CHAIN == dict(loss=max(8 * Z.MEASURED_CHAIN["loss"], Z.BAR["loss"]), params=8 * Z.MEASURED_CHAIN["params"])
    assert Z.CHAIN_UPDATES == 51 and Z.CHAIN_N == 3
