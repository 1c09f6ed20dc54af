"""The PPO gradient kernel (deep_rl_amd/csrc/mi_grad_kernel.inc, compiled by mi_update.hip as grad_kernel_f32 and grad_kernel_bx) on the synthetic cases of
tests/_ppo_cases.py (validated on the CPU by tests/test_ppo_cases_cpu.py) against FLOAT64 AUTOGRAD: a saturated policy up to |l0 - l1| = 110 (the 1 + exp2(-|d|)
path, p == 0 in the entropy term, the one-head form d = l0 - l1 with dW3[1] = -dW3[0]), all four (sign A) x (below / above the clip) quadrants with ratios 0.05 ...
20, value rows placed ON dv == +-clip and on vl1 == vl2 bit for bit, constant and ill-conditioned advantages, a one-row minibatch, and minibatches of 2 ... 1,025
rows around the 16-row tile, the 8-wave workgroup and the 16-block young / old split grid (897 ... 1,024 rows; 1,025 falls back to plain striding) — through
PPOEngine with forced indices.  Every other PPO expectation in the suite comes from oracle/cpu_ref.c, which derives the same backward pass by hand as the kernel
does, or from the one golden trace of the reference run; this reference does not.

Every storage row outside the minibatch holds NaN, so a stray read shows in the result; every case runs under set_contraction("f32") and ("bf16x3") with the SAME
bounds (the rule of tests/test_gpu_contraction.py).  Bounds: _ppo_cases.BOUND = max(8 x the f32 oracle's measured distance from float64, the bar of
test_gpu_parity.py::test_minibatch_grad_vs_oracle_sizes), per family and figure; adv_illcond has loose ones of its own.  Nothing is excluded.
Observed maxima go to ppo_gpu_maxima.json in the tests' results directory (a copy is kept as profiles/ppo_gpu_maxima.json, the figures in docs/LEDGER.md)."""
import json
import os

import numpy as np
import pytest
import torch

import _ppo_cases as K
from _c51_ref import results_dir
from test_gpu_parity import _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request, dev):
    """the matrix pipe of the kernel's three 64 x 64 contractions: process-wide, back to "f32" afterwards whatever the test did"""
    import deep_rl_amd as D

    try:
        D.set_contraction(request.param)
        assert D.get_contraction() == request.param
        yield request.param
    finally:
        D.set_contraction("f32")


def _record(key, value):
    path = os.path.join(results_dir(), "ppo_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
    for k in K.FIGURES:
        fam[k] = max(fam.get(k, 0.0), value[k])
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _bits(t):
    return t.detach().cpu().numpy().copy().view(np.uint32)


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(dev, mode, i):
    c = K.make_case(i)
    fam, mb, e = c["family"], c["mb"], c["exp"]
    eng = _engine(dev, K.N, params=c["params"], T_=K.T, clip_coef=c["clip_coef"], ent_coef=K.ENT_COEF, vf_coef=K.VF_COEF)
    assert (eng.T, eng.N, eng.batch_size) == (K.T, K.N, K.ROWS)
    for name in ("observations", "actions", "log_probs", "advantages", "returns", "values"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.set_perm(c["perm"])
    eng.adv_stats(mb=mb, n_mb=1)
    eng.minibatch_grad(0, mb=mb)
    grads, terms = eng.grads.cpu().numpy().copy(), eng.loss_terms.cpu().numpy().copy()
    g_bits, t_bits = _bits(eng.grads), _bits(eng.loss_terms)
    eng.minibatch_grad(0, mb=mb)
    assert np.array_equal(_bits(eng.grads), g_bits) and np.array_equal(_bits(eng.loss_terms), t_bits), "a second identical launch differs"
    # ---- the advantage statistics the kernel normalises with
    sums = eng.adv_sums[0].cpu().numpy()
    assert K.adv_sums_check(c, sums) is None, (c["name"], K.adv_sums_check(c, sums), sums)
    # ---- NaN exactly where float64 has it: nowhere, but for the one-row minibatch's policy loss, total loss and actor gradient (ppo.py:169)
    if fam == "one_row":
        assert np.isnan(grads[:K.C_BASE]).all() and np.isnan(terms[[0, 3]]).all(), "mb == 1: the actor gradient, pg_loss and loss are NaN"
        assert np.isfinite(grads[K.C_BASE:]).all() and np.isfinite(terms[[1, 2]]).all()
    else:
        assert np.isfinite(grads).all() and np.isfinite(terms).all(), "NaN / inf in the result: a row outside the minibatch was read, or the arithmetic overflowed"
    fig = K.figures(e, dict(grads=grads, terms=terms))
    per_tensor = K.tensor_errors(grads.astype(np.float64), e["grads"])
    print(c["name"], mode, {k: float("%.3g" % v) for k, v in fig.items()}, {k: float("%.3g" % v) for k, v in per_tensor.items()}, terms, e["terms"])
    _record("%s/%s" % (c["name"], mode), dict(fig, family=fam, mb=mb))
    assert not K.within(fig, fam), (c["name"], mode, K.within(fig, fam), per_tensor)
    if fam == "adv_constant":      # A == 0 on the device as well: no policy loss at all
        assert terms[0] == 0
    if fam == "value_placed":      # W3 == 0: nothing reaches the critic's hidden layers
        assert not grads[K.CRITIC["W1"][0]:K.CRITIC["b2"][1]].any()
