"""Placed inputs and numpy restatements for the optimizer step every algorithm here ends in: mi_adam (mi_adam_elem, csrc/mi_common.h), mi_clip_adam (block_grad_norm
and the clip coefficient, csrc/mi_update.hip) and mi_polyak (csrc/mi_sac.hip).  numpy only: no GPU, no torch.

What is restated, and how exactly
  adam_consts   the six f32 constants as the host forms them (bias corrections in double, one rounding to f32 each)
  moments32     m' = m + w1 (g - m), v' = v b2 + w2 (g g) in numpy float32, one rounding per operation.  The libraries are built with -ffp-contract=off, so this is
                the kernel's contract BIT FOR BIT
  update64      u = step_size m' / (sqrt(v') rbc2 + eps) in float64 from the f32 values widened; want = p - u
  bound         4 * 2^-23 |u| + 1/2 spacing_f32(|want|) + 2^-148
  norm64        sqrt(fsum(g_i^2)) in float64, rounded to f32;  coef32 = min(f32(max_norm) / (total + f32(1e-6)), 1) in f32
  polyak32      tau p + (1 - tau) t in f32, one rounding per operation

The factor 4 of `bound` is derived, not measured.  The kernel evaluates  p + (-step_size) * (m' * rcp(sqrt(v') * rbc2 + eps))  with the hardware square root and
reciprocal (v_sqrt_f32, v_rcp_f32).  With ulp = 2^-23 relative (the widest an f32 ulp gets): the square root is off by s ulp; the product by rbc2 adds 1/2; the sum
with eps adds 1/2 (and passes on at most what the first term carried, eps > 0 and sqrt >= 0 being of one sign); the reciprocal adds r; the product by m' 1/2; the
product by step_size 1/2: s + r + 2 ulp of the update term, and the last addition rounds once more, 1/2 spacing of the result.  s = r = 1 are the accuracies the
public CDNA instruction-set manuals give for the two instructions (1 ulp each), the figures mi_adam_elem's own comment quotes.  The MI355X micro-architecture guide
this project keeps to lists both instructions only by their issue cost and states no accuracy for either, so nothing there calls for another factor: 4 stands as
derived.  It is never fitted to what a device returns (tests/test_optim_cases_cpu.py: an f32 emulation with both instructions pushed by -1, 0, +1 ulp reaches 0.9999
of it and never exceeds it).

Every buffer is n + PAD long.  The pad of g holds NaN (an over-read of the norm shows as a NaN norm); the pads of p, m, v hold a recognisable finite pattern that
has to come back bit for bit.  All draws come from np.random.default_rng([SEED, ...]): no global state.

A NAMED CASE is a list of RUNS.  A run is a dict: family, n, p, m, v (n + PAD each), seq = [(step, hp, g), ...] applied in order to the carried device state, and
for mi_clip_adam max_norm and exact (the sum of squares is exact in any order: grad_norm is pinned bit for bit).  check_step is the one assertion both the CPU
emulation and the device's output go through; VARIANTS are wrong readings of the same step it can be switched to, so that a test can show it would have failed."""
import math
from collections import namedtuple

import numpy as np

f32, f64 = np.float32, np.float64
SEED = 20261
PAD = 67
FACTOR = 4.0                      # s + r + 2 with s = r = 1: see the module docstring
TINY_ABS = 2.0 ** -126            # the `tiny` family's allowance on m', v': a flushed subnormal

HPS = [(2.5e-4, 0.9, 0.999, 1e-5),           # PPO
       (2.5e-4, 0.9, 0.999, 1e-8),           # DQN
       (2.5e-4, 0.9, 0.999, 0.01 / 128),     # C51, QR-DQN
       (5e-5, 0.9, 0.999, 1e-2 / 32),        # IQN
       (1e-2, 0.9, 0.999, 1e-8),             # REINFORCE
       (1e-3, 0.5, 0.9, 1e-3)]               # nothing at its default
HP_PPO, HP_ODD = HPS[0], HPS[5]
STEPS = [1, 2, 10, 1000, 10 ** 6, 2 ** 31 + 5]
ADAM_NS = [1, 255, 256, 257, 9155]
CLIP_NS = [1, 63, 64, 65, 255, 256, 257, 9154, 9155, 9156, 16384, 16385, 32769]
CLIP_STEPS = [1, 1000]
CLIP_HPS = [HP_PPO, HP_ODD]
MAX_NORMS = [0.5, float("inf")]
HUGE_NS = [n for n in CLIP_NS if n <= 9156]
NORM_FAMILIES = ["ones", "one_hot", "dyadic", "huge", "small", "at_max_norm", "just_below", "zero"]
EXACT_FAMILIES = ["ones", "one_hot", "dyadic", "huge", "small", "zero", "at_max_norm"]     # grad_norm bit for bit
SPECIAL_N = 257
CHAIN_NS = [257, 9155]
TAUS = [0.0, 0.005, 0.5, 1.0]
POLYAK_NS = [1, 255, 257, 9155]

Consts = namedtuple("Consts", "w1 b2 w2 step_size rbc2 eps")


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def adam_consts(step, lr, b1, b2, eps):
    """the six f32 constants exactly as adam_consts (csrc/mi_update.hip) and adam_launch (csrc/mi_sac.hip) form them"""
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2 = 1.0 - math.pow(b2, float(step))
    return Consts(f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(lr / bc1), f32(1.0 / math.sqrt(bc2)), f32(eps))


def moments32(g, m, v, k):
    g, m, v = (np.asarray(a, f32) for a in (g, m, v))
    with np.errstate(all="ignore"):
        m1 = m + k.w1 * (g - m)
        v1 = v * k.b2 + k.w2 * (g * g)
    assert m1.dtype == f32 and v1.dtype == f32
    return m1, v1


def update_term64(m1, v1, k, variant=None, lr=None):
    """u of update64.  variant: a wrong reading of the denominator or of the bias corrections (VARIANTS); the two bias variants need the run's lr"""
    m1, v1 = np.asarray(m1, f32).astype(f64), np.asarray(v1, f32).astype(f64)
    step_size, rbc2, eps = f64(k.step_size), f64(k.rbc2), f64(k.eps)
    with np.errstate(all="ignore"):
        if variant == "eps_inside_sqrt":
            den = np.sqrt(v1 + eps) * rbc2
        elif variant == "eps_scaled_by_rbc2":
            den = (np.sqrt(v1) + eps) * rbc2
        elif variant == "no_bias_correction2":
            den = np.sqrt(v1) + eps
        else:
            den = np.sqrt(v1) * rbc2 + eps
        if variant == "bias_correction1_missing":
            step_size = f64(f32(lr))
        return step_size * m1 / den


def update64(p, m1, v1, k, variant=None, lr=None):
    """-> (u, want): the update term and the stepped parameter in float64"""
    u = update_term64(m1, v1, k, variant, lr)
    return u, np.asarray(p, f32).astype(f64) - u


def spacing_f32(x):
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(x, f64)).astype(f32)).astype(f64)


def bound(p, u, want):
    return FACTOR * 2.0 ** -23 * np.abs(u) + 0.5 * spacing_f32(want) + 2.0 ** -148


def norm64(g, n=None, variant=None):
    """the pre-clip total norm of g[:n] as an f32.  g may be the padded buffer; only norm_reads_to_multiple_of_64 looks past n"""
    g = np.asarray(g, f32)
    n = g.size if n is None else n
    if variant == "norm_reads_to_multiple_of_64":
        x = g[:min(g.size, (n + 63) // 64 * 64)]
    elif variant == "norm_drops_last_block":
        x = g[:(n - 1) // 64 * 64]
    else:
        x = g[:n]
    with np.errstate(all="ignore"):
        if variant == "norm_in_f32":
            s = f32(0.0)
            for q in (x * x).reshape(-1):
                s = f32(s + q)
            return f32(np.sqrt(s))
        x = x.astype(f64)
        sq = x * x                                    # exact: 24-bit significands
        if not np.all(np.isfinite(sq)):
            return f32(np.sqrt(f64(np.sum(sq))))      # nan / inf propagate as IEEE sums do
        return f32(math.sqrt(math.fsum(sq.tolist())))


def coef32(total, max_norm, variant=None):
    total = f32(total)
    with np.errstate(all="ignore"):
        c = f32(max_norm) / (total if variant == "coef_without_1e-6" else total + f32(1e-6))
    c = f32(c)
    if variant == "coef_not_capped":
        return c
    return f32(1.0) if c > f32(1.0) else c            # a NaN coefficient stays NaN, as `coef > 1 ? 1 : coef` leaves it


def polyak32(t, p, tau, variant=None):
    t, p, tau = np.asarray(t, f32), np.asarray(p, f32), f32(tau)
    if variant == "polyak_tau_swapped":
        return (f32(1.0) - tau) * p + tau * t
    out = tau * p + (f32(1.0) - tau) * t
    assert out.dtype == f32
    return out


def emulate32(p, g, m, v, k, ds=0, dr=0):
    """mi_adam_elem in numpy float32 with a correctly rounded square root and reciprocal, each then displaced by ds / dr ulp (-1, 0, +1) -> (p', m', v')"""
    m1, v1 = moments32(g, m, v, k)
    with np.errstate(all="ignore"):
        out = np.asarray(p, f32) + (-k.step_size) * _ratio32(m1, v1, k, ds, dr)
    assert out.dtype == f32
    return out, m1, v1


def _ratio32(m1, v1, k, ds, dr):
    with np.errstate(all="ignore"):
        den = _displace(np.sqrt(v1), ds) * k.rbc2 + k.eps
        return m1 * _displace(f32(1.0) / den, dr)


def term_error_ulp(g, m, v, k, ds=0, dr=0):
    """the emulated f32 update term step_size (m' rcp(..)) against update64's u, in units of 2^-23 |u|: what FACTOR bounds, without the last addition's rounding
    (elements whose term is below 2^-100 are left out: a subnormal term has no relative accuracy to speak of)"""
    m1, v1 = moments32(g, m, v, k)
    with np.errstate(all="ignore"):
        t = k.step_size * _ratio32(m1, v1, k, ds, dr)
    u = update_term64(m1, v1, k)
    ok = np.isfinite(u) & (np.abs(u) > 2.0 ** -100)
    return float((np.abs(t.astype(f64) - u)[ok] / (2.0 ** -23 * np.abs(u[ok]))).max()) if ok.any() else 0.0


def _displace(x, d):
    if d == 0:
        return x
    y = np.nextafter(x, f32(np.inf) if d > 0 else f32(-np.inf))
    return np.where(np.isfinite(x) & (x != 0), y, x).astype(f32)


# the wrong readings: what each is switched into, and the named case (and run) on which the device's output is outside the reading's own tolerance
VARIANTS = {
    "eps_inside_sqrt": dict(kind="update", api="adam", case="drawn_n257_step1"),
    "eps_scaled_by_rbc2": dict(kind="update", api="adam", case="drawn_n257_step10"),
    "no_bias_correction2": dict(kind="update", api="adam", case="drawn_n257_step1"),
    "bias_correction1_missing": dict(kind="update", api="adam", case="first_step"),
    "v_from_clipped_g_but_m_from_raw_g": dict(kind="moments", api="clip", case="drawn_n257"),
    "norm_in_f32": dict(kind="norm", api="clip", case="huge_n257"),
    "norm_drops_last_block": dict(kind="norm", api="clip", case="one_hot_n257"),       # run 1: the 3 sits at n - 1
    "norm_reads_to_multiple_of_64": dict(kind="norm", api="clip", case="ones_n65"),
    "coef_without_1e-6": dict(kind="coef", api="clip", case="at_max_norm_n257"),
    "coef_not_capped": dict(kind="coef", api="clip", case="small_n257"),
    "polyak_tau_swapped": dict(kind="polyak", api="polyak", case="tau0.005_n257"),
}
VARIANT_RUN = {"norm_drops_last_block": 1}      # which run of the named case (default 0)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the one assertion
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def check_step(run, before, g, k, got, coef=None, variant=None, lr=None, stats=None):
    """One optimizer step of `run` (family, n) from `before` = (p, m, v) with gradient g (the padded buffer) and constants k gave `got` = (p, m, v): pads bit for bit,
    m' and v' bit for bit against moments32 (tiny: within 2^-126), p within `bound` of update64 wherever that is finite, NaN exactly where the restatement has NaN,
    p bit for bit unchanged where v' overflowed.  coef: the clip coefficient applied to g first (in f32, as the kernel does).  stats: a dict that keeps the running term_ulp_seen.
    -> the largest err / bound"""
    n, fam = run["n"], run["family"]
    p0, m0, v0 = (np.asarray(a, f32) for a in before)
    pg, mg, vg = (np.asarray(a, f32) for a in got)
    for name, a, b in (("p", p0, pg), ("m", m0, mg), ("v", v0, vg)):
        assert a.size == b.size == n + PAD
        assert np.array_equal(bits(a[n:]), bits(b[n:])), "%s: the pad behind %s changed" % (run["label"], name)
    graw = np.asarray(g, f32)[:n]
    with np.errstate(all="ignore"):
        ge = graw if coef is None else graw * f32(coef)
    if variant == "v_from_clipped_g_but_m_from_raw_g":
        m1, _ = moments32(graw, m0[:n], v0[:n], k)
        _, v1 = moments32(ge, m0[:n], v0[:n], k)
    else:
        m1, v1 = moments32(ge, m0[:n], v0[:n], k)
    u, want = update64(p0[:n], m1, v1, k, variant, lr)
    nan = np.isnan(m1) | np.isnan(v1) | np.isnan(want)
    assert np.array_equal(np.isnan(mg[:n]), np.isnan(m1)) and np.array_equal(np.isnan(vg[:n]), np.isnan(v1)), "%s: NaN moments in other places" % run["label"]
    assert np.array_equal(np.isnan(pg[:n]), nan), "%s: NaN parameters in other places" % run["label"]
    ok = ~nan
    if fam == "tiny":
        assert np.all(np.abs(mg[:n].astype(f64) - m1) <= TINY_ABS) and np.all(np.abs(vg[:n].astype(f64) - v1) <= TINY_ABS), run["label"]
    else:
        okm, okv = ~np.isnan(m1), ~np.isnan(v1)
        assert np.array_equal(bits(mg[:n])[okm], bits(m1)[okm]), "%s: exp_avg differs from moments32 in %d places" % (run["label"], int((bits(mg[:n]) != bits(m1))[okm].sum()))
        assert np.array_equal(bits(vg[:n])[okv], bits(v1)[okv]), "%s: exp_avg_sq differs from moments32 in %d places" % (run["label"], int((bits(vg[:n]) != bits(v1))[okv].sum()))
    over = np.isinf(v1) & np.isfinite(m1)
    assert np.array_equal(bits(pg[:n])[over], bits(p0[:n])[over]), "%s: a parameter moved where exp_avg_sq overflowed" % run["label"]
    if not ok.any():
        return 0.0
    err = np.abs(pg[:n].astype(f64) - want)[ok]
    ratio = err / bound(p0[:n], u, want)[ok]
    worst = float(ratio.max())
    if stats is not None:                             # what of the error the last addition's half spacing cannot explain, in ulp (2^-23 |u|) of the update term
        big = np.abs(u[ok]) > 2.0 ** -100
        if big.any():
            ex = (err[big] - 0.5 * spacing_f32(want)[ok][big]) / (2.0 ** -23 * np.abs(u[ok][big]))
            stats["term_ulp_seen"] = max(stats.get("term_ulp_seen", 0.0), float(ex.max()))
    assert worst <= 1.0, "%s: parameter off by %.4f of the bound (element %d)" % (run["label"], worst, int(np.flatnonzero(ok)[ratio.argmax()]))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _pad_pattern(tot, n, salt):
    """the recognisable finite pattern behind p, m, v: -(1000 + salt) - j / 64"""
    return (-(1000.0 + salt) - np.arange(tot - n) / 64.0).astype(f32)


def _drawn_g(rng, tot):
    g = (10.0 ** rng.uniform(-12.0, 3.0, tot) * rng.choice([-1.0, 1.0], tot)).astype(f32)
    g[rng.random(tot) < 0.1] = 0.0
    return g


def _drawn_moments(rng, tot):
    """as tests/_reinforce_cases.adam_cases draws them"""
    v = (10.0 ** rng.uniform(-12.0, 3.0, tot)).astype(f32) ** 2
    v[rng.random(tot) < 0.1] = 0.0
    m = (rng.normal(0.0, 1.0, tot) * np.sqrt(v)).astype(f32)
    return m, v


def _finish(run):
    n = run["n"]
    tot = n + PAD
    for salt, key in enumerate(("p", "m", "v")):
        run[key] = np.ascontiguousarray(run[key], f32)
        run[key][n:] = _pad_pattern(tot, n, salt)
    seq = []
    for step, hp, g in run["seq"]:
        g = np.ascontiguousarray(g, f32).copy()
        g[n:] = np.nan
        seq.append((step, hp, g))
    run["seq"] = seq
    return run


def _base(rng, n, warm):
    tot = n + PAD
    p = rng.normal(0.0, 0.5, tot).astype(f32)
    m, v = _drawn_moments(rng, tot) if warm else (np.zeros(tot, f32), np.zeros(tot, f32))
    return p, m, v


def _drawn_run(key, n, step, hp, warm, label, family="drawn", **extra):
    rng = _rng(*key)
    g = _drawn_g(rng, n + PAD)
    p, m, v = _base(rng, n, warm)
    return _finish(dict(family=family, n=n, p=p, m=m, v=v, seq=[(step, hp, g)], label=label, warm=bool(warm), **extra))


def _chain_run(key, n, first, hps, label, **extra):
    """six consecutive steps first .. first + 5 with their own gradients; lr changes from step to step (annealing, ppo.py:107-108)"""
    rng = _rng(*key)
    p, m, v = _base(rng, n, False)
    seq = []
    for j in range(6):
        lr, b1, b2, eps = hps
        seq.append((first + j, (lr * (1.0 - j / 7.0), b1, b2, eps), _drawn_g(rng, n + PAD)))
    return _finish(dict(family="chain", n=n, p=p, m=m, v=v, seq=seq, label=label, **extra))


def adam_case_names():
    names = ["drawn_n%d_step%d" % (n, s) for n in ADAM_NS for s in STEPS]
    return names + ["first_step", "zero_grad", "tiny", "overflow", "nan_elem"] + ["chain_n%d_from%d" % (n, s) for n in CHAIN_NS for s in (1, 10 ** 6)]


def adam_case(name):
    """-> the runs of one named mi_adam case"""
    runs = []
    if name.startswith("drawn_"):
        n, step = int(name.split("_")[1][1:]), int(name.split("_")[2][4:])
        i, j = ADAM_NS.index(n), STEPS.index(step)
        for h, hp in enumerate(HPS):
            for warm in (0, 1):
                runs.append(_drawn_run((1, i, j, h, warm), n, step, hp, warm, "adam drawn n %d, step %d, (lr, b1, b2, eps) %s, %s moments" % (n, step, hp, "drawn" if warm else "zero")))
    elif name == "first_step":
        for h, hp in enumerate(HPS):
            rng = _rng(2, h)
            tot = SPECIAL_N + PAD
            g = (10.0 ** rng.uniform(0.0, 3.0, tot) * rng.choice([-1.0, 1.0], tot)).astype(f32)       # |g| >= 1 >= 1000 eps
            p, m, v = _base(rng, SPECIAL_N, False)
            runs.append(_finish(dict(family="first_step", n=SPECIAL_N, p=p, m=m, v=v, seq=[(1, hp, g)], label="adam first_step %s" % (hp,))))
    elif name == "zero_grad":
        for h, hp in enumerate(HPS):
            for j, step in enumerate((1, 1000)):
                rng = _rng(3, h, j)
                p, m, v = _base(rng, SPECIAL_N, True)
                runs.append(_finish(dict(family="zero_grad", n=SPECIAL_N, p=p, m=m, v=v, seq=[(step, hp, np.zeros(SPECIAL_N + PAD, f32))], label="adam zero_grad %s step %d" % (hp, step))))
    elif name == "tiny":
        for h, hp in enumerate(HPS):
            for j, step in enumerate((1, 1000)):
                rng = _rng(4, h, j)
                tot = SPECIAL_N + PAD
                g = (10.0 ** rng.uniform(-22.0, -19.0, tot) * rng.choice([-1.0, 1.0], tot)).astype(f32)
                p, m, v = _base(rng, SPECIAL_N, False)
                runs.append(_finish(dict(family="tiny", n=SPECIAL_N, p=p, m=m, v=v, seq=[(step, hp, g)], label="adam tiny %s step %d" % (hp, step))))
    elif name == "overflow":
        for h, hp in enumerate(CLIP_HPS):
            rng = _rng(5, h)
            g = _drawn_g(rng, SPECIAL_N + PAD)
            p, m, v = _base(rng, SPECIAL_N, True)
            at = np.unique(np.concatenate([[0, SPECIAL_N - 1, 63, 64], rng.integers(0, SPECIAL_N, 5)]))
            g[at] = (3e19 * rng.choice([-1.0, 1.0], at.size)).astype(f32)
            runs.append(_finish(dict(family="overflow", n=SPECIAL_N, p=p, m=m, v=v, seq=[(7, hp, g), (8, hp, g)], at=at, label="adam overflow %s" % (hp,))))
    elif name == "nan_elem":
        rng = _rng(6)
        g = _drawn_g(rng, SPECIAL_N + PAD)
        p, m, v = _base(rng, SPECIAL_N, True)
        at = 130
        g[at] = np.nan
        runs.append(_finish(dict(family="nan_elem", n=SPECIAL_N, p=p, m=m, v=v, seq=[(3, HP_PPO, g)], at=at, label="adam nan_elem")))
    elif name.startswith("chain_"):
        n, first = int(name.split("_")[1][1:]), int(name.split("_")[2][4:])
        for h, hp in enumerate(CLIP_HPS):
            runs.append(_chain_run((7, n, first % 1000, h), n, first, hp, "adam chain n %d from step %d %s" % (n, first, hp)))
    else:
        raise KeyError(name)
    return runs


def clip_case_names():
    names = ["drawn_n%d" % n for n in CLIP_NS]
    for fam in NORM_FAMILIES:
        names += ["%s_n%d" % (fam, n) for n in (HUGE_NS if fam == "huge" else CLIP_NS)]
    return names + ["nan_norm", "inf_norm"] + ["chain_n%d_from%d" % (n, s) for n in CHAIN_NS for s in (1, 10 ** 6)]


def one_hot_places(n, rng):
    """0, n - 1, the first and last element of the first, the last and two drawn 64-blocks, five drawn places"""
    nb = (n + 63) // 64
    blocks = [0, nb - 1] + [int(b) for b in rng.integers(0, nb, 2)]
    at = [0, n - 1]
    for b in blocks:
        at += [64 * b, min(64 * b + 63, n - 1)]
    at += [int(i) for i in rng.integers(0, n, 5)]
    out = []
    for i in at:
        if i not in out:
            out.append(i)
    return out


def clip_case(name):
    """-> the runs of one named mi_clip_adam case"""
    runs = []
    if name in ("nan_norm", "inf_norm"):
        rng = _rng(20, name == "inf_norm")
        n = SPECIAL_N
        g = _drawn_g(rng, n + PAD)
        p, m, v = _base(rng, n, True)
        at = 200
        g[at] = np.nan if name == "nan_norm" else np.inf
        return [_finish(dict(family=name, n=n, p=p, m=m, v=v, seq=[(3, HP_PPO, g)], at=at, max_norm=0.5, exact=True, label="clip " + name))]
    fam, n = name.rsplit("_n", 1)
    if fam.startswith("chain"):
        n, first = int(n.split("_")[0]), int(n.split("from")[1])
        for h, hp in enumerate(CLIP_HPS):
            runs.append(_chain_run((21, n, first % 1000, h), n, first, hp, "clip chain n %d from step %d %s" % (n, first, hp), max_norm=0.5, exact=False))
        return runs
    n = int(n)
    i = CLIP_NS.index(n)
    tot = n + PAD
    if fam == "drawn":
        for j, step in enumerate(CLIP_STEPS):
            for h, hp in enumerate(CLIP_HPS):
                for q, mx in enumerate(MAX_NORMS):
                    runs.append(_drawn_run((22, i, j, h, q), n, step, hp, (j + h + q) % 2, "clip drawn n %d, step %d, %s, max_norm %s" % (n, step, hp, mx), max_norm=mx, exact=False))
        return runs
    fi = NORM_FAMILIES.index(fam)
    rng = _rng(23, fi, i)
    step, hp = CLIP_STEPS[(i + fi) % 2], CLIP_HPS[(i // 2 + fi) % 2]
    p, m, v = _base(rng, n, (i + fi) % 3 != 0)
    gs = []
    if fam == "ones":
        gs.append(np.ones(tot, f32))
    elif fam == "one_hot":
        for at in one_hot_places(n, rng):
            g = np.zeros(tot, f32); g[at] = 3.0
            gs.append(g)
    elif fam == "dyadic":
        gs.append((rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], tot) / 16.0).astype(f32))
    elif fam == "huge":
        gs.append((1e30 * rng.choice([-1.0, 1.0], tot)).astype(f32))
    elif fam == "small":
        gs.append((1e-30 * rng.choice([-1.0, 1.0], tot)).astype(f32))
    elif fam in ("at_max_norm", "just_below"):
        g = np.zeros(tot, f32); g[int(rng.integers(0, n))] = 0.5 if fam == "at_max_norm" else 0.499999
        gs.append(g)
    elif fam == "zero":
        gs.append(np.zeros(tot, f32))
    else:
        raise KeyError(name)
    for r, g in enumerate(gs):
        runs.append(_finish(dict(family=fam, n=n, p=p.copy(), m=m.copy(), v=v.copy(), seq=[(step, hp, g)], max_norm=0.5, exact=fam in EXACT_FAMILIES,
                                 label="clip %s n %d run %d" % (fam, n, r))))
    return runs


def polyak_case_names():
    return ["tau%s_n%d" % (("%g" % t), n) for t in TAUS for n in POLYAK_NS]


def polyak_case(name):
    """-> dict(tau, n, t, p): at the general taus both vectors carry +0, -0 and a subnormal where they fit"""
    tau, n = name[3:].split("_n")
    tau, n = float(tau), int(n)
    rng = _rng(30, TAUS.index(tau), POLYAK_NS.index(n))
    tot = n + PAD
    t, p = rng.normal(0.0, 1.0, tot).astype(f32), rng.normal(0.0, 1.0, tot).astype(f32)
    if tau not in (0.0, 1.0):
        sub = f32(3e-41)
        if n == 1:
            p[0] = sub
        else:
            t[0], p[0] = 0.0, -0.0
            t[1], p[1] = -0.0, -0.0
            t[2], p[2] = -0.0, 0.0
            t[3], p[3] = 0.5, sub
            t[4], p[4] = -sub, 0.25
            t[5], p[5] = sub, -sub
    t[n:] = _pad_pattern(tot, n, 3)
    p[n:] = np.nan
    return dict(tau=tau, n=n, t=t, p=p, label="polyak " + name)
