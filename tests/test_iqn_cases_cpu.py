"""The synthetic cases of tests/_iqn_ref.py, on the CPU: each keeps the margins that stop a comparison from hiding a failure (no ReLU pre-activation within
NEAR_ZERO of 0, no |td error| within the kappa margin, no row with close action values) and together they reach what tests/test_gpu_iqn_cases.py claims of them:
terminated rows, successors across the ring's end, both Huber branches, both indicator values, and a batch larger than the gradient launch's slab count."""
import numpy as np
import pytest

import _iqn_ref as R


@pytest.fixture(scope="module")
def conditions():
    out = []
    for shp in R.CASES:
        c = R.make_case(*shp, R.CASE_SEEDS[shp])
        r64 = R.update(c["params"], c["target_params"], c["ring"], c["inds"], c["taus"], c["next_taus"], c["tau_dashes"], dtype=np.float64)
        out.append((shp, c, r64, R.case_conditions(c, r64)))
    return out


def test_shapes_are_the_issues_and_one_exceeds_the_slab_count():
    from deep_rl_amd import _native_iqn as K
    assert R.CASES[:4] == ((1, 1, 2), (5, 3, 7), (33, 2, 40), (32, 1, 300))
    assert max(b for b, _n, _s in R.CASES) > K.MAX_SLABS and set(R.CASE_SEEDS) == set(R.CASES)


def test_every_case_keeps_its_margins(conditions):
    for shp, c, r64, cond in conditions:
        print(shp, cond)
        assert cond["min_preact"] > R.NEAR_ZERO, shp
        assert cond["min_kappa"] > cond["kappa_margin"], shp
        assert cond["close_rows"] == 0, shp
        assert np.isfinite(r64["grads"]).all() and np.abs(r64["grads"]).max() > 0
        assert c["inds"].max() < c["ring"][1].size and c["taus"].max() < 1.0 and c["taus"].min() >= 0.0


def test_cases_reach_what_they_claim(conditions):
    tot = {k: sum(cond[k] for _s, _c, _r, cond in conditions) for k in ("terminated_rows", "wraps", "quad", "lin", "neg", "pos")}
    print(tot)
    assert all(cond["wraps"] >= 1 for _s, _c, _r, cond in conditions)                       # every case has a successor across the ring's end
    assert all(cond["terminated_rows"] >= 1 for shp, _c, _r, cond in conditions if shp[0] > 1)
    assert min(tot["quad"], tot["lin"], tot["neg"], tot["pos"]) >= 1000                     # both Huber branches, both indicator values
    for shp, _c, _r, cond in conditions:                                                     # ... mixed INSIDE rows: a quarter of a case's rows hold all four kinds
        assert cond["mixed_rows"] >= max(1, shp[0] // 4) and min(cond["quad"], cond["lin"], cond["neg"], cond["pos"]) >= 100, (shp, cond)
    # every layer has units on and units off, and gradient reaches every tensor
    for shp, _c, r64, _cond in conditions:
        fw = r64["fw"]
        for n in ("z1", "z2", "z3", "zc", "z"):
            on = (fw[n] > 0).mean()
            assert 0.1 < on < 0.9, (shp, n, on)
        # the GPU test compares every tensor against its OWN largest gradient element, so none hides behind the output layer's; each must be a real signal:
        # far above what f32 rounding of the largest gradient could fake (2^-24 max |g|)
        g = R.unpack(r64["grads"], np.float64)
        gmax = np.abs(r64["grads"]).max()
        assert all(np.abs(g[k]).max() > 1e-5 * gmax for k in R.ORDER), (shp, {k: np.abs(g[k]).max() / gmax for k in R.ORDER})
    shp, c, r64, _cond = conditions[0]
    assert shp in R.REALISTIC and np.abs(c["params"][R.OFF["FB1"]:R.OFF["FB1"] + 32]).max() == 0   # the one-row case has reference-style parameters (zero extractor biases)


def test_restatement_modes_agree_on_a_case(conditions):
    shp, c, r64, _cond = conditions[1]
    r32 = R.update(c["params"], c["target_params"], c["ring"], c["inds"], c["taus"], c["next_taus"], c["tau_dashes"], dtype=np.float32)
    scale = max(1.0, np.abs(r64["current"]).max())
    assert np.abs(r32["current"] - r64["current"]).max() <= R.MEASURED_QUANT_REL * scale * 4
    assert abs(float(r32["loss"]) - r64["loss"]) <= R.MEASURED_LOSS_REL * abs(r64["loss"]) and np.abs(r32["grads"] - r64["grads"]).max() <= R.MEASURED_GRAD_REL * np.abs(r64["grads"]).max()


def test_philox_tau_draws_lie_on_torch_rands_grid():
    t = R.tau_draws(7, 3, np.arange(5), 64, 10)
    assert t.shape == (5, 64) and t.dtype == np.float32 and t.min() >= 0 and t.max() < 1 and np.array_equal(t * 16777216.0, np.round(t * 16777216.0))
    assert len(np.unique(t)) == t.size and not np.array_equal(t, R.tau_draws(7, 3, np.arange(5), 64, 12))
    i = R.index_draws(7, 3, 32, 1000)
    assert i.min() >= 0 and i.max() < 1000
