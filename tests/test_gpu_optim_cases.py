"""mi_adam, mi_clip_adam and mi_polyak of libmirl.so on the placed cases of tests/_optim_cases.py (tests/test_optim_cases_cpu.py shows that each case has the property
it is named for, and that the assertions used here fail on every wrong reading in VARIANTS), through the C ABI.

  mi_adam        exp_avg and exp_avg_sq bit for bit against moments32 (the tiny family: within 2^-126, a flushed subnormal is allowed there and nowhere else), every
                 parameter within bound = 4 * 2^-23 |u| + 1/2 spacing(|want|) + 2^-148 of the float64 update, pads behind all three vectors untouched
  mi_clip_adam   grad_norm bit for bit against norm64 on the families whose sum of squares is exact, within one f32 spacing on drawn gradients; then the same three checks
                 with g * coef32(the device's own grad_norm, max_norm) as the gradient; max_norm = inf gives the bits of mi_adam; the NaN pad behind g would turn
                 any over-read into a NaN norm
  mi_polyak      polyak32 bit for bit; tau = 0 leaves the target, tau = 1 copies the parameters
  optim.Adam / ClipAdam over a chain case: the bits of the direct calls, one step counted per call

Observed maxima (the largest err / bound per family, the largest grad_norm error in f32 spacings, and the largest part of a parameter's error that its last rounding
cannot explain, in ulp of the update term: the figure FACTOR = 4 is about) go to optim_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest

import _optim_cases as C
from _c51_ref import results_dir

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

ADAM_NAMES = (["drawn_n%d_step%d" % (n, s) for n in (1, 255, 256, 257, 9155) for s in (1, 2, 10, 1000, 10 ** 6, 2 ** 31 + 5)]
              + ["first_step", "zero_grad", "tiny", "overflow", "nan_elem"] + ["chain_n%d_from%d" % (n, s) for n in (257, 9155) for s in (1, 10 ** 6)])
_CLIP_NS = (1, 63, 64, 65, 255, 256, 257, 9154, 9155, 9156, 16384, 16385, 32769)
CLIP_NAMES = (["%s_n%d" % (fam, n) for fam in ("drawn", "ones", "one_hot", "dyadic") for n in _CLIP_NS] + ["huge_n%d" % n for n in _CLIP_NS if n <= 9156]
              + ["%s_n%d" % (fam, n) for fam in ("small", "at_max_norm", "just_below", "zero") for n in _CLIP_NS] + ["nan_norm", "inf_norm"]
              + ["chain_n%d_from%d" % (n, s) for n in (257, 9155) for s in (1, 10 ** 6)])
POLYAK_NAMES = ["tau%s_n%d" % (t, n) for t in ("0", "0.005", "0.5", "1") for n in (1, 255, 257, 9155)]
STATS = {}                       # check_step's running figure: the part of a parameter's error its last rounding cannot explain, in ulp of the update term
VARIANT_NAMES = ["eps_inside_sqrt", "eps_scaled_by_rbc2", "no_bias_correction2", "bias_correction1_missing", "v_from_clipped_g_but_m_from_raw_g", "norm_in_f32",
                 "norm_drops_last_block", "norm_reads_to_multiple_of_64", "coef_without_1e-6", "coef_not_capped", "polyak_tau_swapped"]


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


class _Bufs:
    """device buffers per length, reused from run to run: p, g, m, v, a second set for the mi_adam twin of a max_norm = inf run, and the norm"""

    def __init__(self, dev):
        import torch

        self.torch, self.dev, self.by_len = torch, dev, {}
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)

    def get(self, tot):
        if tot not in self.by_len:
            self.by_len[tot] = {k: self.torch.empty(tot, dtype=self.torch.float32, device=self.dev) for k in ("p", "g", "m", "v", "p2", "m2", "v2")}
        return self.by_len[tot]

    def put(self, t, a):
        t.copy_(self.torch.from_numpy(np.ascontiguousarray(a, f32)))


@pytest.fixture(scope="module")
def bufs(dev):
    return _Bufs(dev)


def _record(family, ratio=None, norm_spacings=None, flushed=None, term_ulp=None):
    from deep_rl_amd import _native as N

    path = os.path.join(results_dir(), "optim_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    sid = N.lib().mi_source_id().decode()
    if d.get("source_id") != sid:
        d = {"source_id": sid}
    if ratio is not None:
        fam = d.setdefault("err_over_bound", {})
        fam[family] = max(fam.get(family, 0.0), float(ratio))
    if norm_spacings is not None:
        d["grad_norm_error_in_spacings"] = max(d.get("grad_norm_error_in_spacings", 0.0), float(norm_spacings))
    if term_ulp is not None:
        d["update_term_ulp_seen"] = max(d.get("update_term_ulp_seen", 0.0), float(term_ulp))
    if flushed is not None:
        label, count, of = flushed                    # per run: running the suite again overwrites, never adds
        d.setdefault("tiny_flushed_subnormals", {})[label] = {"flushed": int(count), "of_nonzero_subnormal": int(of)}
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _adam(N, dev, b, n, step, hp, which=("p", "g", "m", "v")):
    p, g, m, v = (b[k] for k in which)
    N.check(N.lib().mi_adam(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, step, hp[0], hp[1], hp[2], hp[3], N.stream_ptr(dev)), "mi_adam")


def _clip_adam(N, dev, b, n, step, hp, max_norm, norm):
    N.check(N.lib().mi_clip_adam(N.ptr(b["p"]), N.ptr(b["g"]), N.ptr(b["m"]), N.ptr(b["v"]), n, step, hp[0], hp[1], hp[2], hp[3], max_norm, N.ptr(norm),
                                 N.stream_ptr(dev)), "mi_clip_adam")


def _read(b, keys=("p", "m", "v")):
    return tuple(b[k].cpu().numpy() for k in keys)


def _run_adam(N, dev, bufs, run):
    """the run's steps through mi_adam, the device state carried and the reference teacher-forced from it -> the largest err / bound"""
    n = run["n"]
    b = bufs.get(n + C.PAD)
    for k in ("p", "m", "v"):
        bufs.put(b[k], run[k])
    before = (run["p"], run["m"], run["v"])
    m_free, v_free = run["m"][:n].copy(), run["v"][:n].copy()
    worst = 0.0
    for step, hp, g in run["seq"]:
        bufs.put(b["g"], g)
        _adam(N, dev, b, n, step, hp)
        got = _read(b)
        k = C.adam_consts(step, *hp)
        worst = max(worst, C.check_step(run, before, g, k, got, stats=STATS))
        assert np.array_equal(C.bits(b["g"].cpu().numpy()), C.bits(g))            # the gradient is read only
        m_free, v_free = C.moments32(g[:n], m_free, v_free, k)
        before = got
    if run["family"] != "tiny":                                                   # m and v do not depend on p: bit for bit over the whole chain, free-running
        ok = ~np.isnan(m_free)
        assert np.array_equal(C.bits(before[1][:n])[ok], C.bits(m_free)[ok]) and np.array_equal(C.bits(before[2][:n])[ok], C.bits(v_free)[ok])
    return worst, before


@pytest.mark.parametrize("name", ADAM_NAMES)
def test_adam_case(dev, bufs, name):
    from deep_rl_amd import _native as N

    for run in C.adam_case(name):
        worst, last = _run_adam(N, dev, bufs, run)
        n = run["n"]
        if run["family"] == "overflow":
            at = run["at"]
            assert np.all(np.isinf(last[2][at])) and np.array_equal(C.bits(last[0][at]), C.bits(run["p"][at])) and np.all(np.isfinite(last[1][:n]))
        if run["family"] == "nan_elem":
            for a in last:
                assert np.flatnonzero(np.isnan(a)).tolist() == [run["at"]]
        if run["family"] == "tiny":
            (step, hp, g), = run["seq"]
            _, v1 = C.moments32(g[:n], run["m"][:n], run["v"][:n], C.adam_consts(step, *hp))
            _record("tiny", flushed=(run["label"], ((v1 != 0) & (last[2][:n] == 0)).sum(), (v1 != 0).sum()))
        if run["family"] == "first_step":                                         # the property the family is named for, on the device itself
            (step, hp, g), = run["seq"]
            k = C.adam_consts(step, *hp)
            u, want = C.update64(run["p"][:n], *C.moments32(g[:n], run["m"][:n], run["v"][:n], k), k)
            want_lr = run["p"][:n].astype(f64) - hp[0] * np.sign(g[:n])          # +-lr, to within the bound and the eps / |g| the denominator keeps (+ the constants' roundings)
            assert np.all(np.abs(last[0][:n].astype(f64) - want_lr) <= C.bound(None, u, want) + hp[0] * (hp[3] / np.abs(g[:n]) + 1e-6)), run["label"]
            assert np.array_equal(np.sign(run["p"][:n].astype(f64) - last[0][:n]), np.sign(g[:n])), run["label"]     # every parameter moves, against its gradient (lr >= 5e-5 >> spacing(|p|))
        _record(run["family"], ratio=worst, term_ulp=STATS.get("term_ulp_seen"))


def _run_clip(N, dev, bufs, run):
    n, mx = run["n"], run["max_norm"]
    b = bufs.get(n + C.PAD)
    for k in ("p", "m", "v"):
        bufs.put(b[k], run[k])
    before = (run["p"], run["m"], run["v"])
    worst, spac = 0.0, 0.0
    for step, hp, g in run["seq"]:
        bufs.put(b["g"], g)
        if np.isinf(mx):
            for k in ("p", "m", "v"):
                b[k + "2"].copy_(b[k])
        bufs.norm.fill_(-7.0)
        _clip_adam(N, dev, b, n, step, hp, mx, bufs.norm)
        total = f32(bufs.norm.cpu().numpy()[0])
        got = _read(b)
        want = C.norm64(g, n)
        if np.isnan(want):
            assert np.isnan(total), run["label"]
        elif run["exact"]:
            assert C.bits(total) == C.bits(want), "%s: grad_norm %r, want %r" % (run["label"], total, want)
        else:
            e = abs(float(total) - float(want)) / float(np.spacing(want))
            assert e <= 1.0, "%s: grad_norm %r, want %r" % (run["label"], total, want)
            spac = max(spac, e)
        coef = C.coef32(total, mx)
        k = C.adam_consts(step, *hp)
        worst = max(worst, C.check_step(run, before, g, k, got, coef=coef, stats=STATS))
        if np.isinf(mx):                                                         # no clipping: the bits of mi_adam on the same inputs
            assert coef == 1
            _adam(N, dev, b, n, step, hp, which=("p2", "g", "m2", "v2"))
            twin = _read(b, ("p2", "m2", "v2"))
            assert all(np.array_equal(C.bits(x), C.bits(y)) for x, y in zip(got, twin)), run["label"]
        before = got
    return worst, spac, total, before


@pytest.mark.parametrize("name", CLIP_NAMES)
def test_clip_adam_case(dev, bufs, name):
    from deep_rl_amd import _native as N

    for run in C.clip_case(name):
        worst, spac, total, last = _run_clip(N, dev, bufs, run)
        n, fam = run["n"], run["family"]
        if fam in ("small", "just_below", "zero"):
            assert C.coef32(total, run["max_norm"]) == 1
        if fam in ("at_max_norm", "huge", "ones", "one_hot"):
            assert C.coef32(total, run["max_norm"]) < 1
        if fam == "zero":
            assert total == 0 and not any(np.isnan(a).any() for a in last)
        if fam == "nan_norm":
            assert all(np.all(np.isnan(a[:n])) for a in last)
        if fam == "inf_norm":
            assert total == np.inf
            for a in last:
                assert np.flatnonzero(np.isnan(a)).tolist() == [run["at"]]
        _record("clip_" + fam, ratio=worst, norm_spacings=spac, term_ulp=STATS.get("term_ulp_seen"))


@pytest.mark.parametrize("name", POLYAK_NAMES)
def test_polyak_case(dev, name):
    import torch

    from deep_rl_amd import _native as N

    c = C.polyak_case(name)
    n = c["n"]
    td, pd = torch.from_numpy(c["t"].copy()).to(dev), torch.from_numpy(c["p"].copy()).to(dev)
    N.check(N.lib().mi_polyak(N.ptr(td), N.ptr(pd), n, c["tau"], N.stream_ptr(dev)), "mi_polyak")
    got = td.cpu().numpy()
    assert np.array_equal(C.bits(got[n:]), C.bits(c["t"][n:])) and np.array_equal(C.bits(pd.cpu().numpy()), C.bits(c["p"]))
    assert np.array_equal(C.bits(got[:n]), C.bits(C.polyak32(c["t"][:n], c["p"][:n], c["tau"])))
    if c["tau"] == 0:
        assert np.array_equal(C.bits(got), C.bits(c["t"]))
    if c["tau"] == 1:
        assert np.array_equal(C.bits(got[:n]), C.bits(c["p"][:n]))


@pytest.mark.parametrize("first", [1, 10 ** 6])
def test_optimizer_classes_give_the_bits_of_the_direct_calls(dev, bufs, first):
    """deep_rl_amd.optim.Adam and ClipAdam over a chain case, param_groups[0]["lr"] reassigned between steps (ppo.py:107-108): the bits of the direct calls, and the
    step counter advances by one per call"""
    import types

    import torch

    from deep_rl_amd import _native as N
    from deep_rl_amd.optim import Adam, ClipAdam

    for api in ("adam", "clip"):
        run = (C.adam_case if api == "adam" else C.clip_case)("chain_n257_from%d" % first)[1]       # the hyper-parameters with nothing at their default
        n = run["n"]
        if api == "adam":
            _, direct = _run_adam(N, dev, bufs, run)
        else:
            _, _, total, direct = _run_clip(N, dev, bufs, run)
        _, hp0, _ = run["seq"][0]
        flat = torch.from_numpy(run["p"][:n].copy()).to(dev)
        if api == "adam":
            opt = Adam(flat, lr=hp0[0], betas=(hp0[1], hp0[2]), eps=hp0[3])
        else:
            opt = ClipAdam(types.SimpleNamespace(flat=flat), lr=hp0[0], betas=(hp0[1], hp0[2]), eps=hp0[3], max_grad_norm=run["max_norm"])
        assert opt.step_count == 0 and not opt.exp_avg.any() and not run["m"][:n].any() and not run["v"][:n].any()
        opt.step_count = first - 1
        for j, (step, hp, g) in enumerate(run["seq"]):
            opt.param_groups[0]["lr"] = hp[0]
            opt.step(torch.from_numpy(g[:n].copy()).to(dev))
            assert opt.step_count == step == first + j
        for got, want in ((flat, direct[0]), (opt.exp_avg, direct[1]), (opt.exp_avg_sq, direct[2])):
            assert np.array_equal(C.bits(got.cpu().numpy()), C.bits(want[:n]))
        if api == "clip":
            assert C.bits(opt.grad_norm.cpu().numpy()[0]) == C.bits(total)


@pytest.mark.parametrize("variant", VARIANT_NAMES)
def test_wrong_variants_would_be_seen(dev, bufs, variant):
    """the device's output on the variant's named case is outside the variant's own tolerance: the assertions above would fail on a kernel that computed it"""
    import torch

    from deep_rl_amd import _native as N

    spec = C.VARIANTS[variant]
    if spec["api"] == "polyak":
        c = C.polyak_case(spec["case"])
        n = c["n"]
        td, pd = torch.from_numpy(c["t"].copy()).to(dev), torch.from_numpy(c["p"].copy()).to(dev)
        N.check(N.lib().mi_polyak(N.ptr(td), N.ptr(pd), n, c["tau"], N.stream_ptr(dev)), "mi_polyak")
        assert not np.array_equal(C.bits(td.cpu().numpy()[:n]), C.bits(C.polyak32(c["t"][:n], c["p"][:n], c["tau"], variant)))
        return
    run = (C.adam_case if spec["api"] == "adam" else C.clip_case)(spec["case"])[C.VARIANT_RUN.get(variant, 0)]
    n = run["n"]
    (step, hp, g), = run["seq"][:1]
    run = dict(run, seq=run["seq"][:1])
    before = (run["p"], run["m"], run["v"])
    k = C.adam_consts(step, *hp)
    if spec["api"] == "adam":
        _, got = _run_adam(N, dev, bufs, run)
        coef = None
    else:
        _, _, total, got = _run_clip(N, dev, bufs, run)
        coef = C.coef32(total, run["max_norm"])
    if spec["kind"] == "norm":
        assert C.bits(total) != C.bits(C.norm64(g, n, variant))
        return
    if spec["kind"] == "coef":
        coef = C.coef32(total, run["max_norm"], variant)
    with pytest.raises(AssertionError):
        C.check_step(run, before, g, k, got, coef=coef, variant=None if spec["kind"] == "coef" else variant, lr=hp[0])
