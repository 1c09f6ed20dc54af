"""mi_ars_update on placed inputs (tests/_ars_ref.placed_cases; tests/test_ars_ref_cpu.py shows that each case has the property it is named for): M, stats and k
bit for bit against the CPU restatement, norm within relative 1e-9 — all returns equal for every b (M unchanged), ties straddling the cut, b = 1 and b = N, N = 1,
r+ = r- on every selected direction with sigma_R > 0 (M unchanged), and N = 4,096 once."""
import numpy as np
import pytest
import torch

import _ars_gpu as G
import _ars_ref as A

pytestmark = pytest.mark.gpu
NAMES = ["all_equal_b%d" % b for b in range(1, 9)] + ["ties_straddle_cut", "b_1", "b_N", "N_1", "equal_pairs_selected", "N_4096"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def K():
    from deep_rl_amd import _native_ars
    return _native_ars


def test_the_list_of_cases_is_the_references():
    assert NAMES == list(A.placed_cases())


@pytest.mark.parametrize("name", NAMES)
def test_placed_update_case(dev, K, name):
    c = A.placed_cases()[name]
    for normalize in (True, False):
        want = A.update(c["state"], c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"], normalize=normalize)
        ds = G.DevState(dev, c["state"])
        G.run_update(K, dev, ds, c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"], normalize)
        got = ds.read()
        G.check_state(got, want)
        if not normalize:
            assert np.array_equal(G.bits(got["norm"]), G.bits(np.asarray(c["state"]["norm"])))
        else:
            assert not np.array_equal(got["norm"], c["state"]["norm"])
        if name.startswith("all_equal") or name == "equal_pairs_selected":
            assert np.array_equal(G.bits(got["M"]), G.bits(c["state"]["M"]))
        else:
            assert not np.array_equal(G.bits(got["M"]), G.bits(c["state"]["M"]))


def test_wrong_variants_would_be_seen_on_the_tie_case(dev, K):
    """the device's M on the tie case is none of the wrong readings' M"""
    c = A.placed_cases()["ties_straddle_cut"]
    ds = G.DevState(dev, c["state"])
    G.run_update(K, dev, ds, c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"])
    got = ds.read()["M"]
    for v in ("top_by_plus_only", "sigma_all_returns", "sample_deviation", "tie_to_higher_index"):
        bad = A.update(c["state"], c["returns"], c["deltas"], c["partials"], c["b"], c["step_size"], variant=v)
        assert not np.array_equal(G.bits(got), G.bits(bad["M"])), v
