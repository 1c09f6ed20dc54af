"""tests/_optim_cases.py on the CPU: every family has the property it is named for; an f32 emulation of mi_adam_elem with the square root and the reciprocal pushed
by -1, 0, +1 ulp stays inside `bound` on every non-special case; the C oracle's adam_step and clip_grad_norm agree with update64 and norm64; every wrong reading in
VARIANTS breaks the bound or bit-exactness on its named case (so the GPU assertions would fail on a kernel that computed it); and the GPU test's lists of case names
are the module's."""
import itertools
import math

import numpy as np
import pytest

import _optim_cases as C

f32, f64 = np.float32, np.float64
MIN_NORMAL = 2.0 ** -126

# The oracle (oracle/cpu_ref.c: ref_adam_step) evaluates p + (-step_size) * (m' / (sqrtf(v') / f32(sqrt(bc2)) + eps)) in f32 with true divisions; update64 uses
# rbc2 = f32(1 / sqrt(bc2)).  Derived the way FACTOR is, in ulp (2^-23 relative at the widest) of the update term: sqrtf 1/2, the division by bc2_sqrt 1/2, the
# rounding of f32(sqrt(bc2)) 1/2 and that of update64's own rbc2 1/2 (the two constants stand for the same real number), the sum with eps 1/2, m' / denom 1/2, the
# product by step_size 1/2: 3.5 ulp.  The last addition's rounding is `bound`'s own second term.
ORACLE_FACTOR = 3.5


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    return cpu_ref


def _normal_or_zero(a):
    a = np.abs(np.asarray(a, f64))
    return bool(np.all((a == 0) | ((a >= MIN_NORMAL) & np.isfinite(a))))


def _runs(names, case):
    for name in names:
        for run in case(name):
            yield name, run


def test_hyperparameters_steps_and_lengths_are_the_issues():
    assert C.PAD == 67 and C.FACTOR == 4.0
    assert C.HPS == [(2.5e-4, .9, .999, 1e-5), (2.5e-4, .9, .999, 1e-8), (2.5e-4, .9, .999, 0.01 / 128), (5e-5, .9, .999, 1e-2 / 32), (1e-2, .9, .999, 1e-8), (1e-3, .5, .9, 1e-3)]
    assert C.STEPS == [1, 2, 10, 1000, 10 ** 6, 2 ** 31 + 5] and C.ADAM_NS == [1, 255, 256, 257, 9155]
    assert C.CLIP_NS == [1, 63, 64, 65, 255, 256, 257, 9154, 9155, 9156, 16384, 16385, 32769]
    for step in (10 ** 6, 2 ** 31 + 5):                                  # both corrections exactly 1
        for hp in C.HPS:
            k = C.adam_consts(step, *hp)
            assert k.rbc2 == 1.0 and k.step_size == f32(hp[0])
    k = C.adam_consts(1, *C.HP_ODD)
    assert k.w1 == f32(0.5) and k.b2 == f32(0.9) and k.w2 == f32(1.0 - 0.9) and k.step_size == f32(1e-3 / 0.5) and k.rbc2 == f32(1.0 / math.sqrt(1.0 - 0.9)) and k.eps == f32(1e-3)
    seen = set()
    for name in C.adam_case_names():                                     # the full product, nothing left out
        if name.startswith("drawn_"):
            for run in C.adam_case(name):
                (step, hp, _), = run["seq"]
                seen.add((run["n"], step, hp, run["warm"]))
                assert run["warm"] or not (run["m"][:run["n"]].any() or run["v"][:run["n"]].any())
    assert seen == set(itertools.product(C.ADAM_NS, C.STEPS, C.HPS, (False, True)))
    seen = set()
    for n in C.CLIP_NS:
        for run in C.clip_case("drawn_n%d" % n):
            (step, hp, _), = run["seq"]
            seen.add((n, step, hp, run["max_norm"]))
    assert seen == set(itertools.product(C.CLIP_NS, (1, 1000), (C.HP_PPO, C.HP_ODD), (0.5, float("inf"))))


def test_pads_and_determinism():
    for names, case in ((C.adam_case_names(), C.adam_case), (C.clip_case_names(), C.clip_case)):
        for name, run in _runs(names[::7], case):
            n = run["n"]
            for salt, key in enumerate(("p", "m", "v")):
                assert run[key].size == n + C.PAD and run[key].dtype == f32
                assert np.array_equal(run[key][n:], C._pad_pattern(n + C.PAD, n, salt)) and np.all(np.isfinite(run[key]))
            for _, _, g in run["seq"]:
                assert g.size == n + C.PAD and np.all(np.isnan(g[n:]))
    a, b = C.adam_case("drawn_n257_step2"), C.adam_case("drawn_n257_step2")
    assert all(np.array_equal(C.bits(x[key]), C.bits(y[key])) for x, y in zip(a, b) for key in ("p", "m", "v"))
    assert all(np.array_equal(C.bits(x["seq"][0][2]), C.bits(y["seq"][0][2])) for x, y in zip(a, b))
    assert not np.array_equal(a[0]["seq"][0][2], a[2]["seq"][0][2])


def test_drawn_intermediates_are_normal_or_zero():
    zeros = 0
    for name, run in _runs([n for n in C.adam_case_names() if n.startswith("drawn_")], C.adam_case):
        n = run["n"]
        (step, hp, g), = run["seq"]
        k = C.adam_consts(step, *hp)
        g, m, v = g[:n], run["m"][:n], run["v"][:n]
        m1, v1 = C.moments32(g, m, v, k)
        a = np.abs(g[g != 0])
        assert a.size == 0 or (a.min() >= f32(1e-12) and a.max() <= f32(1e3))
        zeros += int((g == 0).sum())
        for x in (g * g, k.w2 * (g * g), v * k.b2, v1, g - m, k.w1 * (g - m), m1):
            assert _normal_or_zero(x), run["label"]
        u, want = C.update64(run["p"][:n], m1, v1, k)
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(want))
    assert zeros > 1000                                                  # the exact zeros are there


def test_first_step_moves_by_lr_against_the_sign():
    for run in C.adam_case("first_step"):
        n = run["n"]
        (step, hp, g), = run["seq"]
        assert step == 1 and not run["m"][:n].any() and not run["v"][:n].any() and np.abs(g[:n]).min() >= 1000 * hp[3]
        k = C.adam_consts(1, *hp)
        m1, v1 = C.moments32(g[:n], run["m"][:n], run["v"][:n], k)
        u, want = C.update64(run["p"][:n], m1, v1, k)
        assert np.array_equal(np.sign(u), np.sign(g[:n]))
        assert np.all(np.abs(np.abs(u) / hp[0] - 1.0) <= hp[3] / np.abs(g[:n]) + 1e-6)
        got, _, _ = C.emulate32(run["p"][:n], g[:n], run["m"][:n], run["v"][:n], k)
        want_lr = run["p"][:n].astype(f64) - hp[0] * np.sign(g[:n])       # the sign property itself, to within the bound and the eps / |g| the denominator keeps
        assert np.all(np.abs(got - want_lr) <= C.bound(None, u, want) + hp[0] * (hp[3] / np.abs(g[:n]) + 1e-6))


def test_zero_grad_only_decays_and_still_moves():
    for run in C.adam_case("zero_grad"):
        n = run["n"]
        (step, hp, g), = run["seq"]
        assert not g[:n].any() and run["m"][:n].any() and run["v"][:n].any()
        k = C.adam_consts(step, *hp)
        m1, v1 = C.moments32(g[:n], run["m"][:n], run["v"][:n], k)
        assert np.all(np.abs(m1) <= np.abs(run["m"][:n])) and np.all(v1 <= run["v"][:n])
        nz = run["m"][:n] != 0
        assert np.all(np.abs(m1[nz]) < np.abs(run["m"][:n][nz])) and np.all(np.sign(m1) == np.sign(run["m"][:n]))
        got, _, _ = C.emulate32(run["p"][:n], g[:n], run["m"][:n], run["v"][:n], k)
        assert (got != run["p"][:n]).sum() > n // 2


def test_tiny_has_subnormal_second_moments_and_eps_dominates():
    sub = 0
    for run in C.adam_case("tiny"):
        n = run["n"]
        (step, hp, g), = run["seq"]
        a = np.abs(g[:n])
        assert a.min() >= f32(1e-22) and a.max() <= f32(1e-19)
        k = C.adam_consts(step, *hp)
        m1, v1 = C.moments32(g[:n], run["m"][:n], run["v"][:n], k)
        assert np.all(v1 < MIN_NORMAL) and np.all(g[:n] * g[:n] < MIN_NORMAL)
        sub += int(((v1 > 0) & (v1 < MIN_NORMAL)).sum())
        assert np.all(np.sqrt(v1.astype(f64)) * f64(k.rbc2) * 2.0 ** 9 < f64(k.eps))
        assert _normal_or_zero(m1) and np.all(m1 != 0)
    assert sub > 100


def test_overflow_and_nan_elem_have_what_they_are_named_for():
    for run in C.adam_case("overflow"):
        n, at = run["n"], run["at"]
        assert len(run["seq"]) == 2 and {0, n - 1} <= set(at.tolist())
        p, m, v = run["p"][:n], run["m"][:n], run["v"][:n]
        for step, hp, g in run["seq"]:
            k = C.adam_consts(step, *hp)
            with np.errstate(over="ignore"):
                assert np.all(np.abs(g[at]) == f32(3e19)) and np.all(np.isinf(g[at] * g[at]))
            p1, m1, v1 = C.emulate32(p, g[:n], m, v, k)
            assert np.all(np.isinf(v1[at])) and np.all(np.isfinite(m1)) and np.isinf(v1).sum() == at.size
            assert np.array_equal(C.bits(p1[at]), C.bits(p[at]))         # bit for bit unchanged, both steps
            others = np.setdiff1d(np.arange(n), at)
            assert (p1[others] != p[others]).sum() > others.size // 2
            p, m, v = p1, m1, v1
    run, = C.adam_case("nan_elem")
    (step, hp, g), = run["seq"]
    assert np.isnan(g[:run["n"]]).sum() == 1 and np.isnan(g[run["at"]])
    p1, m1, v1 = C.emulate32(run["p"][:run["n"]], g[:run["n"]], run["m"][:run["n"]], run["v"][:run["n"]], C.adam_consts(step, *hp))
    for a in (p1, m1, v1):
        assert np.flatnonzero(np.isnan(a)).tolist() == [run["at"]]


def test_norm_families_have_what_they_are_named_for():
    for n in C.CLIP_NS:
        run, = C.clip_case("ones_n%d" % n)
        g = run["seq"][0][2]
        assert np.all(g[:n] == 1) and C.norm64(g, n) == f32(math.sqrt(n))
        places = set()
        for run in C.clip_case("one_hot_n%d" % n):
            g = run["seq"][0][2]
            at, = np.flatnonzero(g[:n])
            assert g[at] == 3 and C.norm64(g, n) == f32(3.0)
            places.add(int(at))
        nb = (n + 63) // 64
        assert {0, n - 1, min(63, n - 1), 64 * (nb - 1)} <= places and len(places) >= min(n, 5)
        run, = C.clip_case("dyadic_n%d" % n)
        g = run["seq"][0][2][:n].astype(f64)
        assert set(np.unique(np.abs(g) * 16).tolist()) <= {1.0, 2.0, 3.0}
        sq = g * g
        rng = np.random.default_rng(n)
        sums = {math.fsum(sq.tolist()), float(np.sum(sq)), float(np.sum(sq[rng.permutation(n)])), float(np.cumsum(sq[::-1])[-1]), float(np.cumsum(sq.astype(f32)[rng.permutation(n)])[-1])}
        assert len(sums) == 1                                            # order-independent, even accumulated in f32: n * 9 / 256 < 2^24 / 256
        run, = C.clip_case("small_n%d" % n)
        g = run["seq"][0][2]
        assert np.all(np.abs(g[:n]) == f32(1e-30)) and C.norm64(g, n, "norm_in_f32") == 0 and C.norm64(g, n) > 0
        assert C.coef32(C.norm64(g, n), 0.5) == 1
        run, = C.clip_case("at_max_norm_n%d" % n)
        g = run["seq"][0][2]
        assert np.count_nonzero(g[:n]) == 1 and C.norm64(g, n) == f32(0.5) == f32(run["max_norm"])
        c = C.coef32(C.norm64(g, n), 0.5)
        assert c < 1 and abs(1.0 - float(c) - 2e-6) < 2e-7             # bites by one part in 5e5
        run, = C.clip_case("just_below_n%d" % n)
        g = run["seq"][0][2]
        assert C.norm64(g, n) == f32(0.499999) < f32(0.5) and C.coef32(C.norm64(g, n), 0.5) == 1
        run, = C.clip_case("zero_n%d" % n)
        g = run["seq"][0][2]
        assert not g[:n].any() and C.norm64(g, n) == 0 and C.coef32(0.0, 0.5) == 1
    for n in C.HUGE_NS:
        run, = C.clip_case("huge_n%d" % n)
        g = run["seq"][0][2]
        assert max(C.HUGE_NS) == 9156 and np.all(np.abs(g[:n]) == f32(1e30))
        assert np.isinf(C.norm64(g, n, "norm_in_f32")) and np.isfinite(C.norm64(g, n))
        c = C.coef32(C.norm64(g, n), 0.5)
        assert MIN_NORMAL <= c < 1e-30


def test_exact_families_round_the_same_whatever_the_order_of_the_sum():
    """grad_norm is pinned bit for bit on EXACT_FAMILIES.  ones, one_hot, dyadic, at_max_norm and zero have sums of squares that are exact in float64 in any order;
    huge and small sum n equal 46-bit squares, which a float64 tree may round in its last bits — so show that the f32 norm is the same for every float64 sum within
    2^-40 relative of the true one (a tree over 9,156 terms is within 9156 * 2^-53 < 2^-39.8)."""
    for fam in C.EXACT_FAMILIES:
        for n in (C.HUGE_NS if fam == "huge" else C.CLIP_NS):
            for run in C.clip_case("%s_n%d" % (fam, n)):
                assert run["exact"]
                g = run["seq"][0][2][:n].astype(f64)
                s = math.fsum((g * g).tolist())
                assert f32(math.sqrt(s * (1 - 2.0 ** -39))) == f32(math.sqrt(s)) == f32(math.sqrt(s * (1 + 2.0 ** -39))) == C.norm64(run["seq"][0][2], n), run["label"]
    assert not any(run["exact"] for n in C.CLIP_NS for run in C.clip_case("drawn_n%d" % n))


def test_nan_and_inf_norm_cases():
    run, = C.clip_case("nan_norm")
    g = run["seq"][0][2]
    assert run["n"] == 257 and np.isnan(g[:257]).sum() == 1 and np.isnan(C.norm64(g, 257)) and np.isnan(C.coef32(C.norm64(g, 257), 0.5))
    run, = C.clip_case("inf_norm")
    g = run["seq"][0][2]
    assert np.isinf(g[:257]).sum() == 1 and g[run["at"]] == np.inf and C.norm64(g, 257) == np.inf and C.coef32(np.inf, 0.5) == 0
    with np.errstate(all="ignore"):
        ge = g[:257] * C.coef32(np.inf, 0.5)
    assert np.flatnonzero(np.isnan(ge)).tolist() == [run["at"]] and not ge[~np.isnan(ge)].any()


def test_chains_change_lr_and_run_consecutive_steps():
    for names, case in ((C.adam_case_names(), C.adam_case), (C.clip_case_names(), C.clip_case)):
        chains = [n for n in names if n.startswith("chain_")]
        assert len(chains) == 4
        for name, run in _runs(chains, case):
            steps = [s for s, _, _ in run["seq"]]
            assert steps in ([1, 2, 3, 4, 5, 6], list(range(10 ** 6, 10 ** 6 + 6)))
            assert len({hp[0] for _, hp, _ in run["seq"]}) == 6 and len({hp[1:] for _, hp, _ in run["seq"]}) == 1
            assert not any(np.array_equal(a[2], b[2]) for a, b in zip(run["seq"], run["seq"][1:]))


def _emulated_chain(run, ds=0, dr=0, clip=False):
    """the runs' steps on the emulation, the state carried as the device carries it -> per step (before, g, k, got, coef)"""
    n = run["n"]
    p, m, v = run["p"].copy(), run["m"].copy(), run["v"].copy()
    for step, hp, g in run["seq"]:
        k = C.adam_consts(step, *hp)
        coef = C.coef32(C.norm64(g, n), run["max_norm"]) if clip else None
        with np.errstate(all="ignore"):
            ge = g[:n] if coef is None else g[:n] * coef
        before = (p.copy(), m.copy(), v.copy())
        p[:n], m[:n], v[:n] = C.emulate32(p[:n], ge, m[:n], v[:n], k, ds, dr)
        yield before, g, k, (p.copy(), m.copy(), v.copy()), coef, hp


def test_emulation_stays_inside_the_bound_on_every_adam_case():
    """f32 arithmetic as the kernel's, square root and reciprocal each displaced by -1, 0, +1 ulp from the correctly rounded value: inside `bound` everywhere, and close
    to it somewhere — the factor is neither loose nor fitted"""
    worst, term = 0.0, 0.0
    for name, run in _runs(C.adam_case_names(), C.adam_case):
        n = run["n"]
        for ds, dr in itertools.product((-1, 0, 1), repeat=2):
            for before, g, k, got, _, _ in _emulated_chain(run, ds, dr):
                worst = max(worst, C.check_step(run, before, g, k, got))
                if run["family"] not in ("overflow", "nan_elem"):
                    term = max(term, C.term_error_ulp(g[:n], before[1][:n], before[2][:n], k, ds, dr))
    assert 0.9999 < worst <= 1.0, worst                                  # (the last addition's half spacing alone comes this close wherever the update is far below p)
    assert 3.0 < term <= C.FACTOR, term                                  # the update term by itself: s + r + 2 ulp holds, and more than three of the four are used


def test_emulation_stays_inside_the_bound_on_every_clip_case():
    worst = 0.0
    for name, run in _runs(C.clip_case_names(), C.clip_case):
        for ds, dr in ((-1, -1), (0, 0), (1, 1), (-1, 1)):
            for before, g, k, got, coef, _ in _emulated_chain(run, ds, dr, clip=True):
                worst = max(worst, C.check_step(run, before, g, k, got, coef=coef))
    assert 0.5 < worst <= 1.0, worst


def test_oracle_adam_step_and_clip_grad_norm_agree_with_the_restatements(R):
    worst = 0.0
    for name, run in _runs([n for n in C.adam_case_names() if n.startswith("drawn_")], C.adam_case):
        n = run["n"]
        (step, hp, g), = run["seq"]
        k = C.adam_consts(step, *hp)
        p, m, v = run["p"][:n].copy(), run["m"][:n].copy(), run["v"][:n].copy()
        R.adam_step(p, g[:n].copy(), m, v, step, hp[0], hp[1], hp[2], hp[3])
        m1, v1 = C.moments32(g[:n], run["m"][:n], run["v"][:n], k)
        assert np.array_equal(C.bits(m), C.bits(m1)) and np.array_equal(C.bits(v), C.bits(v1)), run["label"]
        u, want = C.update64(run["p"][:n], m1, v1, k)
        tol = ORACLE_FACTOR * 2.0 ** -23 * np.abs(u) + 0.5 * C.spacing_f32(want) + 2.0 ** -148
        r = float((np.abs(p.astype(f64) - want) / tol).max())
        assert r <= 1.0, (run["label"], r)
        worst = max(worst, r)
    assert worst > 0.5
    for n in C.CLIP_NS:
        for run in C.clip_case("drawn_n%d" % n):
            g = run["seq"][0][2]
            mx = min(run["max_norm"], 3e38)
            gc = g[:n].copy()
            total = f32(R.clip_grad_norm(gc, mx))
            want = C.norm64(g, n)
            assert abs(float(total) - float(want)) <= float(np.spacing(want)), run["label"]     # a sequential float64 sum against fsum: the f32 rounding may fall either way
            assert np.array_equal(C.bits(gc), C.bits(g[:n] * C.coef32(total, mx)))


def test_polyak_cases():
    for name in C.polyak_case_names():
        c = C.polyak_case(name)
        n, t, p = c["n"], c["t"], c["p"]
        assert t.size == p.size == n + C.PAD and np.all(np.isnan(p[n:])) and np.all(np.isfinite(t))
        want = C.polyak32(t[:n], p[:n], c["tau"])
        if c["tau"] == 0:
            assert np.array_equal(C.bits(want), C.bits(t[:n]))
        elif c["tau"] == 1:
            assert np.array_equal(C.bits(want), C.bits(p[:n]))
        else:
            assert not np.array_equal(want, t[:n]) and not np.array_equal(want, p[:n])
            sub = (np.abs(p[:n]) > 0) & (np.abs(p[:n]) < MIN_NORMAL)
            assert sub.any()
            if n > 1:
                assert np.signbit(t[:n][t[:n] == 0]).tolist() == [False, True, True] and (p[:n] == 0).sum() == 3
                assert np.signbit(want[:3]).tolist() == [False, True, False]          # +0 + -0, -0 + -0, -0 + +0


def _expect_failure(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError("%s would not be seen" % what)


def test_every_variant_breaks_its_named_case():
    """the honest emulation stands in for the device: checked against a wrong reading's own expectation it has to fail on the case VARIANTS names"""
    assert sorted(C.VARIANTS) == sorted(["eps_inside_sqrt", "eps_scaled_by_rbc2", "no_bias_correction2", "bias_correction1_missing", "v_from_clipped_g_but_m_from_raw_g",
                                         "norm_in_f32", "norm_drops_last_block", "norm_reads_to_multiple_of_64", "coef_without_1e-6", "coef_not_capped", "polyak_tau_swapped"])
    for variant, spec in C.VARIANTS.items():
        if spec["api"] == "polyak":
            c = C.polyak_case(spec["case"])
            got = C.polyak32(c["t"][:c["n"]], c["p"][:c["n"]], c["tau"])
            assert not np.array_equal(C.bits(got), C.bits(C.polyak32(c["t"][:c["n"]], c["p"][:c["n"]], c["tau"], variant))), variant
            continue
        assert spec["case"] in (C.adam_case_names() if spec["api"] == "adam" else C.clip_case_names())
        run = (C.adam_case if spec["api"] == "adam" else C.clip_case)(spec["case"])[C.VARIANT_RUN.get(variant, 0)]
        n = run["n"]
        (before, g, k, got, coef, hp), = list(_emulated_chain(run, clip=spec["api"] == "clip"))[:1]
        C.check_step(run, before, g, k, got, coef=coef)                # the right reading passes
        if spec["kind"] == "norm":
            assert C.bits(C.norm64(g, n, variant)) != C.bits(C.norm64(g, n)), variant
        elif spec["kind"] == "coef":
            bad = C.coef32(C.norm64(g, n), run["max_norm"], variant)
            assert bad != coef
            _expect_failure(lambda: C.check_step(run, before, g, k, got, coef=bad), variant)
        else:
            if variant == "v_from_clipped_g_but_m_from_raw_g":
                assert coef < 1
            _expect_failure(lambda: C.check_step(run, before, g, k, got, coef=coef, variant=variant, lr=hp[0]), variant)


def test_gpu_test_lists_the_modules_cases():
    import test_gpu_optim_cases as T

    assert T.ADAM_NAMES == C.adam_case_names() and T.CLIP_NAMES == C.clip_case_names() and T.POLYAK_NAMES == C.polyak_case_names()
    assert T.VARIANT_NAMES == list(C.VARIANTS)
    assert len(set(T.ADAM_NAMES)) == len(T.ADAM_NAMES) and len(set(T.CLIP_NAMES)) == len(T.CLIP_NAMES)
