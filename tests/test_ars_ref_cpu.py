"""The CPU restatement of Augmented Random Search (tests/_ars_ref.py) on its own: what tests/test_gpu_ars*.py rest on is shown here without a GPU — each wrong
reading of include/mi_ars.h changes M on the inputs those tests use, the controller reaches the limit and the zero policy falls early on their env ids, the mixed
case mixes, every placed update case has the property it is named for, every normaliser comparison is well conditioned, and one seed of the learning fixture is
reproduced."""
import json
import os

import numpy as np
import pytest

import _ars_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def R():
    import __graft_entry__  # noqa: F401  (puts the repository root on sys.path)
    from deep_rl_amd import _native_ars  # noqa: F401  (the feature under test: its binding must exist for any of this to matter)
    from oracle import cpu_ref
    if not os.path.exists(os.path.join(ROOT, "oracle", "libcpu_ref.so")):
        cpu_ref.build()
    return cpu_ref


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def chains(R):
    """the reference chains of the GPU tests' longest run (5 iterations) on the reference's own draw: (N, b, normalize) -> (state, returns)"""
    return {(N, b, nz): A.chain(R, N, b, max(A.CHAIN_ITERATIONS), normalize=nz) for N, b in A.CHAIN_SHAPES for nz in (True, False)}


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_each_wrong_variant_changes_the_policy_on_the_chain_inputs(R, chains, variant):
    changed = {}
    for (N, b, nz), (st, _ret) in chains.items():
        wrong, _ = A.chain(R, N, b, max(A.CHAIN_ITERATIONS), normalize=nz, variant=variant)
        changed[(N, b, nz)] = not np.array_equal(_bits(wrong["M"]), _bits(st["M"]))
    if variant == "stats_before_episodes":   # without the normaliser the observations' statistics reach nothing
        assert all(changed[k] for k in changed if k[2]) and not any(changed[k] for k in changed if not k[2])
    elif variant == "tie_to_higher_index":   # needs a tie at the cut: the larger chain has one with and without the normaliser
        assert changed[(8, 4, True)] and changed[(8, 4, False)]
    else:
        assert all(changed.values()), changed


def test_update_variants_change_the_placed_cases_they_bear_on():
    c = A.placed_cases()["ties_straddle_cut"]
    good = A.update(c["state"], c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"])
    for v in ("top_by_plus_only", "sigma_all_returns", "sample_deviation", "tie_to_higher_index"):
        bad = A.update(c["state"], c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"], variant=v)
        assert not np.array_equal(_bits(bad["M"]), _bits(good["M"])), v


def test_controller_reaches_the_limit_and_the_zero_policy_falls_early(R):
    st = dict(A.fresh_state(), M=np.array(A.controller()))
    for e in A.evaluate(R, st, max(A.EVAL_EPISODES)):
        assert e["length"] == 500 and e["truncated"] == 1 and e["ret"] == 500.0
    # the controller under the training keys too (noise 0: both signs play M itself), at the largest N it runs at
    for e in A.episodes(R, st, np.zeros((A.CONTROLLER_MAX_N, 8), f32), f32(0.0)):
        assert e["length"] == 500 and e["truncated"] == 1
    for e in A.evaluate(R, A.fresh_state(), max(A.EVAL_EPISODES)) + A.episodes(R, A.fresh_state(), np.zeros((max(A.SHAPES), 8), f32), f32(0.0)):
        assert e["length"] < 50 and e["truncated"] == 0 and not e["actions"].any()   # M = 0: a tie at every step, action 0


def test_mixed_case_puts_a_waves_lanes_on_very_different_lengths():
    m = A.mixed_case()
    assert m is not None and m["noise"] == f32(m["factor"] * 16.0 * 1.0)
    lens = [e["length"] for e in m["episodes"]]
    assert len(lens) == 16 and any(e["truncated"] for e in m["episodes"]) and min(lens) < 100 and max(lens) == 500


def test_random_policy_shapes_have_both_actions_and_short_episodes(R):
    """above CONTROLLER_MAX_N the GPU tests run M = 0 with NOISE: random linear policies, in whose episodes both actions occur and which are short on average (a
    few balance the pole: the replay's cost is the mean)"""
    st = A.fresh_state()
    eps = A.episodes(R, st, A.draw(R, A.SEED, max(A.SHAPES), 0), A.NOISE)
    acts = np.concatenate([e["actions"] for e in eps])
    assert 0 < acts.mean() < 1 and len(acts) < 100 * len(eps) and len({e["length"] for e in eps}) > 3


def test_every_placed_case_has_the_property_it_is_named_for():
    P = A.placed_cases()
    up = lambda c, **kw: A.update(c["state"], c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"], **kw)   # noqa: E731
    for b in range(1, 9):
        c = P["all_equal_b%d" % b]
        assert c["b"] == b and len(set(c["returns"].tolist())) == 1
        new = up(c)
        assert np.array_equal(_bits(new["M"]), _bits(c["state"]["M"])) and new["k"] == c["state"]["k"] + 1 and not np.array_equal(new["stats"], c["state"]["stats"])
        assert A.select(c["returns"], b).nonzero()[0].tolist() == list(range(b))   # all keys tie: the lowest indices
    c = P["ties_straddle_cut"]
    key = c["returns"].reshape(-1, 2).max(1)
    sel = A.select(c["returns"], c["b"])
    cut = np.sort(key)[::-1][c["b"] - 1]
    assert (key == cut).sum() == 3 and (sel & (key == cut)).sum() == 2 and sel.nonzero()[0].tolist() == [1, 2, 5]
    assert A.select(c["returns"], c["b"], "tie_to_higher_index").nonzero()[0].tolist() == [1, 5, 6]
    assert P["b_1"]["b"] == 1 and A.select(P["b_1"]["returns"], 1).sum() == 1 and P["b_N"]["b"] == P["b_N"]["N"] == 8 and A.select(P["b_N"]["returns"], 8).all()
    assert P["N_1"]["N"] == 1 and P["N_1"]["b"] == 1
    for name in ("ties_straddle_cut", "b_1", "b_N", "N_1", "N_4096"):
        assert not np.array_equal(_bits(up(P[name])["M"]), _bits(P[name]["state"]["M"])), name
    c = P["equal_pairs_selected"]
    r, sel = c["returns"].reshape(-1, 2), A.select(c["returns"], c["b"])
    assert (r[sel, 0] == r[sel, 1]).all() and len(set(r[sel, 0].tolist())) > 1 and (r[~sel, 0] != r[~sel, 1]).all()
    assert np.array_equal(_bits(up(c)["M"]), _bits(c["state"]["M"])) and (c["state"]["M"] != 0).all()
    c = P["N_4096"]
    assert c["N"] == 4096 == len(c["deltas"]) and 1 < c["b"] < 4096 and A.select(c["returns"], c["b"]).sum() == c["b"]
    for c in P.values():
        assert c["returns"].min() >= 1 and c["returns"].max() <= 500 and (c["returns"] == np.round(c["returns"])).all() and (c["partials"][:, 0] == c["returns"]).all()


def test_every_normaliser_comparison_is_well_conditioned(R, chains):
    """the GPU tests compare norm within relative 1e-9: a cancellation factor <= 1e3 on 2^-53 and a dozen roundings stays below 1e-12"""
    for c in A.placed_cases().values():
        new = A.update(c["state"], c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"])
        assert (A.conditioning(new["stats"]) <= 1e3).all() and (A.conditioning(new["stats"]) >= 1).all(), c["name"]
        assert (new["norm"][4:] > 0).all()
    for (N, b, nz), _ in chains.items():
        st = A.fresh_state()
        for t in range(max(A.CHAIN_ITERATIONS)):   # after every iteration a GPU chain can stop at
            st, _ret, _eps = A.iterate(R, st, N, b, normalize=nz)
            assert (A.conditioning(st["stats"]) <= 1e3).all(), (N, b, nz, t)


def test_the_draw_is_standard_normal_and_keyed_without_N(R):
    z = A.normal64(R, A.SEED, 64, 3)
    assert abs(z.mean()) < 0.15 and 0.85 < z.std() < 1.15 and np.isfinite(z).all()
    assert np.array_equal(A.normal64(R, A.SEED, 3, 3), z[:3])
    assert not np.array_equal(A.normal64(R, A.SEED, 3, 4), z[:3]) and not np.array_equal(A.normal64(R, A.SEED + 1, 3, 3), z[:3])


def test_one_seed_of_the_learning_fixture_is_reproduced(R):
    import importlib.util
    spec = importlib.util.spec_from_file_location("capture_ars_ref", os.path.join(ROOT, "tools", "capture_ars_ref.py"))
    cap = importlib.util.module_from_spec(spec); spec.loader.exec_module(cap)
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ars_ref_learning.json")))
    assert (fx["n_directions"], fx["n_top"], fx["iterations"], fx["last"], fx["eval_episodes"]) == (cap.N_DIRECTIONS, cap.N_TOP, cap.ITERATIONS, cap.LAST, cap.EVAL_EPISODES)
    assert fx["seeds"] == list(range(1, 25)) and len(fx["train_last_mean"]) == 24 == len(fx["greedy_mean"])
    seed = 5
    train, greedy = cap.run_seed(seed)
    assert train == fx["train_last_mean"][seed - 1] and greedy == fx["greedy_mean"][seed - 1]
    mean = sum(fx["train_last_mean"]) / 24
    sd = (sum((v - mean) ** 2 for v in fx["train_last_mean"]) / 23) ** 0.5
    assert fx["mean"] == mean and fx["sd"] == sd and fx["floor"] == mean - 3.0 * sd and fx["greedy_min"] == min(fx["greedy_mean"])
    assert set(fx) == {"n_directions", "n_top", "step_size", "noise", "normalize", "iterations", "last", "eval_episodes", "seeds", "train_last_mean", "greedy_mean",
                       "mean", "sd", "floor", "greedy_min"}   # results and the settings they were taken at, nothing else
