"""tests/_ppo_cases.py validated on the CPU: the cases meet their conditions with no row left out and reach what they claim (clip quadrants, saturation bands,
bit-for-bit placed value rows, NaN-poisoned storage); the f32 oracle's own forward puts every row on the same side of every branch as float64; the f32 oracle
(oracle/cpu_ref.c) is measured against the float64 autograd reference per family and figure and _ppo_cases.MEASURED is tied to that measurement; each of the four
known-wrong variants of the reference is separated from the right one by >= 10 x the bound of a named family; and a torch FLOAT32 run of the same formulas stays
within the device bounds on the tight families — so when tests/test_gpu_ppo_cases.py fails, a reader knows whether oracle or device is the outlier."""
import numpy as np
import pytest
import torch

import _ppo_cases as K

f32 = np.float32
CASES = range(len(K.SPECS))
_case = lambda name: K.make_case(K.NAMES.index(name))   # noqa: E731


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref

    cpu_ref.lib().ref_set_num_threads(8)
    return cpu_ref


@pytest.fixture(scope="module")
def oracle(R):
    """the oracle's results on every case, computed once: {name: got}"""
    return {K.make_case(i)["name"]: K.oracle_eval(R, K.make_case(i)) for i in CASES}


# ---- conditions and reach -----------------------------------------------------------------------------------------------------------
def test_families_sizes_and_seeds():
    assert [s[2] for s in K.SPECS if s[1] == "plain"] == [2, 5, 16, 17, 33, 128, 129, 897, 1024, 1025]
    assert {s[1]: set() for s in K.SPECS}.keys() == set(K.MEASURED) == set(K.BOUND)
    assert sorted((s[2], s[4]) for s in K.SPECS if s[1] == "saturated") == [(17, 0), (17, 2), (33, 1), (33, 3)]       # one case per band, both sizes
    assert [(s[2], s[3]) for s in K.SPECS if s[1] == "value_placed"] == [(8, 0.25), (24, 0.25)]
    assert [s[2] for s in K.SPECS if s[1] == "adv_constant"] == [2, 17] and [s[4] for s in K.SPECS if s[1] == "adv_illcond"] == [1e3, 1e5]
    for i in CASES:
        assert K.find_seed(i, tries=K.SEEDS[i] + 1) == K.SEEDS[i]      # SEEDS holds the FIRST seed that meets the conditions: nothing was picked by its results


@pytest.mark.parametrize("i", CASES, ids=K.NAMES)
def test_case_meets_its_conditions_with_no_row_left_out(i):
    c = K.make_case(i)
    k, e, mb, idx = c["cond"], c["exp"], c["mb"], c["idx"]
    print(c["name"], k, e["terms"])
    assert K.conditions_met(c)
    # the indices: no repetition, first and last row, and the permutation the engine is given
    assert idx.dtype == np.int32 and len(np.unique(idx)) == mb == k["rows"] and (K.ROWS - 1) in idx and (mb == 1 or 0 in idx)
    assert np.array_equal(c["perm"][:mb], idx) and np.array_equal(np.sort(c["perm"]), np.arange(K.ROWS))
    # the poison: NaN in every row outside idx and in the whole bootstrap row, finite data inside CartPole's range in the rows of idx
    inside = np.zeros(K.ROWS, bool); inside[idx] = True
    for name in ("observations", "log_probs", "advantages", "returns", "values"):
        a = c[name]
        assert a.dtype == f32 and a.shape[:2] == (K.T + 1, K.N) and np.isnan(a[K.T]).all()
        flat = a[:K.T].reshape(K.ROWS, -1)
        assert np.isnan(flat[~inside]).all() and np.isfinite(flat[inside]).all()
    assert (np.abs(c["observations"][:K.T].reshape(K.ROWS, 4)[idx]) <= np.array(K.OBS_RANGE, f32)).all()
    assert set(np.unique(c["actions"])) <= {0, 1}
    # a loss is compared relatively only where |ref| >= 1/3, far above 0.01; everything else is on the absolute floor
    fin = np.isfinite(e["terms"])
    assert K.TERM_FLOOR >= 0.01 and (fin.all() or c["family"] == "one_row")
    if c["family"] == "one_row":
        assert np.isnan(e["grads"][:K.C_BASE]).all() and np.isfinite(e["grads"][K.C_BASE:]).all() and np.array_equal(fin, [False, True, True, False])
        assert np.isnan(e["A"]).all()
    else:
        assert np.isfinite(e["grads"]).all() and np.abs(e["grads"][:K.C_BASE]).max() > 0 and np.abs(e["grads"][K.C_BASE:]).max() > 0
    if c["family"] != "value_placed":
        assert k["ratio_gap"] > K.ratio_margin(c["family"]) and k["dv_gap"] > K.V_MARGIN and k["vl_gap"] >= K.VL_MARGIN


@pytest.mark.parametrize("name", [s[0] for s in K.SPECS if s[1] != "value_placed"])
def test_the_f32_oracle_takes_every_branch_as_float64_does(name, R):
    """the margins do their work: ratio against 1 +- clip, dv against +- clip and (outside the value clip) vl1 against vl2 fall on the same side in the oracle's f32
    forward as in float64, in every row — no row needs an exclusion.  (value_placed sits ON the boundaries: test_value_placed_rows_are_exact_in_f32.)"""
    c = _case(name)
    e, o = c["exp"], K.oracle_forward(R, c)
    print(name, np.abs(o["ratio"] / e["ratio"] - 1).max(), np.abs(o["dv"] - e["dv"]).max(), np.abs((o["vl1"] - o["vl2"]) - (e["vl1"] - e["vl2"])).max())
    clip = f32(c["clip_coef"])
    lo, hi = f32(1) - clip, f32(1) + clip
    assert np.array_equal(o["ratio"] < lo, e["ratio"] < float(lo)) and np.array_equal(o["ratio"] > hi, e["ratio"] > float(hi))
    assert np.abs(o["ratio"] / e["ratio"] - 1).max() < 0.2 * K.ratio_margin(c["family"])
    assert np.array_equal(o["dv"] < -clip, e["dv"] < -float(clip)) and np.array_equal(o["dv"] > clip, e["dv"] > float(clip))
    assert np.abs(o["dv"] - e["dv"]).max() < 0.2 * K.V_MARGIN
    out = np.abs(e["dv"]) > float(clip)
    assert np.array_equal((o["vl1"] > o["vl2"])[out], (e["vl1"] > e["vl2"])[out]) and np.abs((o["vl1"] - o["vl2"]) - (e["vl1"] - e["vl2"])).max() < 0.2 * K.VL_MARGIN


def test_quadrants_are_all_present():
    c = _case("quadrants_33")
    k, e = c["cond"], c["exp"]
    print(k["quadrants"], k["inside"], e["ratio"].min(), e["ratio"].max())
    assert min(k["quadrants"]) >= 3 and k["inside"] >= 3 and sum(k["quadrants"]) + k["inside"] == 33
    assert 0.049 < e["ratio"].min() < 0.056 and 18.0 < e["ratio"].max() < 20.1 and np.abs(np.log(e["ratio"])).max() <= 3.0 + 1e-6
    assert (np.abs(e["A"]) > 0.1).all()                                   # no row's quadrant hangs on the sign of a rounding error


@pytest.mark.parametrize("name", [n for n in K.NAMES if n.startswith("saturated")])
def test_saturation_bands(name, R):
    c = _case(name)
    k, e = c["cond"], c["exp"]
    lo, hi = K.BANDS[K.SPECS[K.NAMES.index(name)][4]]
    print(name, k["max_d"], k["unlikely"], k["min_p"])
    assert lo <= k["max_d"] <= hi and k["unlikely"] >= 2 and k["top_row_unlikely"] and k["max_log_ratio"] <= 0.3 + 1e-5
    top = np.abs(e["d"]).argmax()
    assert abs(e["new_lp"][top] + k["max_d"]) < 1e-2                     # the top row's action has log-prob -max |l0 - l1|
    assert np.isfinite(c["log_probs"][:K.T].reshape(-1)[c["idx"]]).all() and e["ratio"].max() < 1.36      # no ratio overflows in f32
    if hi == 130.0:
        assert np.exp(-k["max_d"]) < np.finfo(f32).tiny                   # p of the unlikely action: below f32's normal range
        nl, p, ent = R.categorical(R.actor(c["params"], c["observations"][:K.T].reshape(-1, 4)[c["idx"]]))
        assert np.isfinite(nl).all() and np.isfinite(ent).all() and (p.min(axis=1)[top] < np.finfo(f32).tiny)


@pytest.mark.parametrize("name", ["value_placed_8", "value_placed_24"])
def test_value_placed_rows_are_exact_in_f32(name, R):
    """every placed equality holds bit for bit in float64, in the torch f32 restatement and in the oracle's f32 forward"""
    c = _case(name)
    mb, clip = c["mb"], f32(K.VALUE_CLIP)
    pat = np.arange(mb) % 8
    assert sorted(np.bincount(pat)) == [mb // 8] * 8
    adv = c["advantages"][:K.T].reshape(-1)[c["idx"]]
    assert adv.astype(np.float64).sum() == 0 and (adv == 0).sum() >= 2 and (c["exp"]["A"] == 0).sum() == (adv == 0).sum()
    want_dv = np.array([1.0 - K.VALUE_ROWS[k][0] for k in pat])
    for ev in (c["exp"], K.evaluate(c, torch.float32), K.oracle_forward(R, c)):
        assert (ev["v"] == 1.0).all() and np.array_equal(ev["dv"], want_dv)
        assert (ev["dv"][pat == 0] == clip).all() and (ev["dv"][pat == 1] == -clip).all() and (ev["dv"][pat == 2] == 0).all()
        tie = np.isin(pat, (0, 1, 2, 3, 4, 7))
        assert (ev["vl1"][tie] == ev["vl2"][tie]).all() and (ev["vl1"][pat == 5] < ev["vl2"][pat == 5]).all() and (ev["vl1"][pat == 6] > ev["vl2"][pat == 6]).all()
        assert (ev["vl1"][pat == 7] == 0).all() and (ev["vl1"][np.isin(pat, (3, 4))] == 0.375 ** 2).all()
    # the expected sub-gradients, stated directly: d (sum of max(vl1, vl2)) / dv per pattern (2 d1 through an end point of the clamp, d1 at a tie with the clipped
    # branch outside, 0 where the clipped branch wins), hence d loss / d b3 = vf_coef 0.5 / 8 x their sum
    r03 = float(f32(0.3))
    per_row = np.array([2 * (1 - r03), 2 * (1 - 2.0), 2 * 0.5, 0.375, -0.375, 0.0, 2 * 0.5, 0.0])
    db3 = float(f32(K.VF_COEF)) * 0.5 * per_row.sum() / 8
    assert abs(c["exp"]["grads"][K.CRITIC["b3"][0]] - db3) < 1e-15 and abs(db3 - 0.043749999) < 1e-9
    g = c["exp"]["grads"]
    assert not g[K.CRITIC["W1"][0]:K.CRITIC["b2"][1]].any()               # W3 == 0: nothing reaches the critic's hidden layers


@pytest.mark.parametrize("name", ["adv_constant_2", "adv_constant_17"])
def test_constant_advantages_leave_the_entropy_gradient_alone(name):
    c = _case(name)
    e = c["exp"]
    adv = c["advantages"][:K.T].reshape(-1)[c["idx"]]
    assert (adv == f32(0.1)).all() and (e["A"] == 0).all() and e["terms"][0] == 0
    ent_only = K.evaluate(c, variant="no_entropy_grad")["grads"][:K.C_BASE]
    assert not ent_only.any() and np.abs(e["grads"][:K.C_BASE]).max() > 1e-5


@pytest.mark.parametrize("name", ["adv_illcond_1e3", "adv_illcond_1e5"])
def test_illconditioned_advantages(name):
    c = _case(name)
    adv = c["advantages"][:K.T].reshape(-1)[c["idx"]].astype(np.float64)
    want = K.SPECS[K.NAMES.index(name)][4]
    assert 0.6 * want < adv.mean() / adv.std(ddof=1) < 1.6 * want and "adv_illcond" not in K.TIGHT


# ---- the bounds are tied to the measurement -----------------------------------------------------------------------------------------
def test_oracle_against_float64_pins_the_bounds(oracle):
    worst = {}
    for i in CASES:
        c = K.make_case(i)
        fig = K.figures(c["exp"], oracle[c["name"]])
        print("%-18s" % c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
        w = worst.setdefault(c["family"], dict.fromkeys(K.FIGURES, 0.0))
        for k, v in fig.items():
            w[k] = max(w[k], v)
    assert set(worst) == set(K.MEASURED)
    assert K.BAR == dict(terms=3e-5, grad_actor=2e-5, grad_critic=2e-5, tensor=1e-3)
    for fam, w in worst.items():
        print("%-14s" % fam, {k: float("%.3g" % v) for k, v in w.items()})
        for k, v in w.items():
            assert v <= 1.5 * K.MEASURED[fam][k], (fam, k, v)                    # the stored values cover the measurement (bound / 8 x 1.5)
            assert v >= K.MEASURED[fam][k] / 1.5, (fam, k, v)                    # and no constant sits far above it
            assert K.BOUND[fam][k] == max(8 * K.MEASURED[fam][k], K.BAR[k])
        if fam in K.TIGHT and fam != "saturated":
            assert max(w["grad_actor"], w["grad_critic"]) <= 2e-6, fam           # the bar, not 8 x the oracle, is the bound of these families
    assert K.BOUND["saturated"]["grad_actor"] <= 2e-4 and K.BOUND["adv_illcond"]["grad_critic"] == 2e-5


def test_one_row_is_nan_where_float64_is(oracle):
    """mb == 1: the oracle's NaN pattern is the reference's (figures() would give inf otherwise) — pg_loss, the loss and the whole actor gradient"""
    g = oracle["one_row_1"]
    assert np.isnan(g["grads"][:K.C_BASE]).all() and np.isfinite(g["grads"][K.C_BASE:]).all() and np.array_equal(np.isnan(g["terms"]), [True, False, False, True])
    fig = K.figures(_case("one_row_1")["exp"], g)
    assert all(np.isfinite(v) for v in fig.values()) and not K.within(fig, "one_row")
    wrong = dict(grads=np.zeros(K.NP), terms=np.zeros(4))                        # a finite answer is infinitely far away
    assert K.figures(_case("one_row_1")["exp"], wrong)["grad_actor"] == np.inf


def test_a_stray_read_is_visible(R):
    """an index outside the case's rows pulls the NaN poison into the result, and figures() reports it as inf"""
    c = dict(_case("plain_17"))
    c["idx"] = c["idx"].copy()
    c["idx"][16] = c["perm"][17]
    got = K.oracle_eval(R, c)
    assert np.isnan(got["grads"]).any()
    assert K.figures(_case("plain_17")["exp"], got)["grad_critic"] == np.inf


@pytest.mark.parametrize("weight", [0.0, 2.0], ids=["dropped", "doubled"])
def test_a_dropped_or_doubled_row_exceeds_the_bounds(weight):
    """129 rows with ONE row left out of the sums, or counted twice (means and advantage statistics still over 129), for every one of the 129 rows: at least one
    figure leaves its bound.  A row whose policy AND value gradient are clipped away moves only the loss terms (and the entropy gradient), rightly; the typical
    row moves some tensor by more than the per-tensor bound, as the docstring's 1 / 129 says.  The lone row of the ninth tile has no value gradient (its clipped
    branch wins) and 0.11 of the largest actor gradient element."""
    c = _case("plain_129")
    tensor = []
    for row in range(129):
        w = np.ones(129); w[row] = weight
        fig = K.figures(c["exp"], K.evaluate(c, row_weight=w))
        tensor.append(fig["tensor"])
        assert K.within(fig, "plain"), (row, fig)
        if row == 128:
            print(fig)
            assert fig["grad_critic"] == 0 and fig["grad_actor"] > 0.1
    over = int((np.array(tensor) > K.BOUND["plain"]["tensor"]).sum())
    print("rows over the tensor bound:", over, "median", np.median(tensor), "least", min(tensor))
    assert over >= 120 and np.median(tensor) > 5 * K.BOUND["plain"]["tensor"]


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,name,figure", [
    ("tie_to_unclipped", "value_placed_8", "grad_critic"), ("tie_to_unclipped", "value_placed_24", "grad_critic"),
    ("clamp_open", "value_placed_8", "grad_critic"), ("clamp_open", "value_placed_24", "grad_critic"),
    ("biased_std", "plain_2", "grad_actor"), ("biased_std", "plain_5", "grad_actor"),
    ("no_entropy_grad", "adv_constant_2", "grad_actor"), ("no_entropy_grad", "adv_constant_17", "grad_actor")])
def test_teeth(variant, name, figure):
    """a wrong reading of ppo.py lies >= 10 x the family's bound away from the right one, in the named figure"""
    c = _case(name)
    fig = K.figures(c["exp"], K.evaluate(c, variant=variant))
    print(variant, name, {k: float("%.3g" % v) for k, v in fig.items()}, "bound", K.BOUND[c["family"]][figure])
    assert fig[figure] >= 10 * K.BOUND[c["family"]][figure]
    assert set(K.VARIANTS) == {"tie_to_unclipped", "clamp_open", "biased_std", "no_entropy_grad"}


# ---- the float32 run of the reference -----------------------------------------------------------------------------------------------
# (case, figure) at which torch's plain f32 evaluation misses the device bound against float64 BY ITSELF: {case: {figure: torch f32 against float64}}, measured.
# Cause: torch.mean of seventeen f32(0.1) taken in f32 is 0.100000009 (one ulp above 0.1f), so every A is -7.5e-9 / (std + 1e-8) = -0.42 instead of 0 and a policy
# gradient appears where there is none.  ppo.py:169 in f32 has this property; the oracle and the kernel take the sum, the mean and the variance in DOUBLE (ref_adv_stats,
# mi_adv_stats) and give A == 0, as float64 does: the oracle is 1.5e-7 / 7.7e-7 from float64 on the same figures.  Two equal f32 sum exactly, so adv_constant_2 is clean.
TORCH_F32_IS_THE_OUTLIER = {"adv_constant_17": {"terms": 1.23, "grad_actor": 153.0, "tensor": 1720.0}}


def test_torch_float32_stays_within_the_device_bounds(oracle):
    """the same formulas evaluated by torch in float32 (its own summation orders, tanh, exp and log) against float64, under the DEVICE bounds, on every tight case:
    the bounds leave room for an honest f32 evaluation that is neither the oracle nor the kernel.  The one exception is pinned with its cause above, with the
    oracle inside 1.5 / 8 of its bound there."""
    seen = {}
    for i in CASES:
        c = K.make_case(i)
        if c["family"] not in K.TIGHT:
            continue
        fig = K.figures(c["exp"], K.evaluate(c, torch.float32))
        print("%-18s" % c["name"], {k: float("%.3g" % v) for k, v in fig.items()})
        over = K.within(fig, c["family"])
        if over:
            o64 = K.figures(c["exp"], oracle[c["name"]])
            for k in over:
                assert o64[k] <= 1.5 * K.MEASURED[c["family"]][k], (c["name"], k, over[k], o64[k])
                seen.setdefault(c["name"], {})[k] = fig[k]
    print(seen)
    assert {n: set(v) for n, v in seen.items()} == {n: set(v) for n, v in TORCH_F32_IS_THE_OUTLIER.items()}
    for n, v in TORCH_F32_IS_THE_OUTLIER.items():
        for k, x in v.items():
            assert x / 1.5 <= seen[n][k] <= 1.5 * x
    a32 = K.evaluate(_case("adv_constant_17"), torch.float32)["A"]
    assert (np.abs(a32) > 0.1).all() and (K.evaluate(_case("adv_constant_2"), torch.float32)["A"] == 0).all()
