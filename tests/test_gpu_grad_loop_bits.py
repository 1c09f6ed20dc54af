"""The gradient launch against the bits of the build before its tile loop was reorganised (tests/golden/ppo_grad_parent_bits.npz; cases, tile counts per wave and
the recording recipe: tests/_ppo_grad_bits.py).  Minibatches of 1, 15, 16, 17, 32, 37, 256 and 1,151 rows of a T = 128, N = 9 storage whose other rows hold NaN
(the ragged tile alone, full tiles alone, both), 131,072 rows of an N = 1,024 storage (11 and 5 tiles per wave) and 73,723 rows of it (6 and 3 tiles per wave, the
last tile ragged), each under both contraction modes: gradient, loss terms and the slab sum's block sums of squares are compared as bit patterns with torch.equal
— there is no tolerance.  One launch per case."""
import numpy as np
import pytest
import torch

import _ppo_cases as K
import _ppo_grad_bits as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    with np.load(B.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def engines(dev):
    """one engine per storage width; the N = 1,024 storage is filled once, the N = 9 one per minibatch size"""
    made = {}

    def get(n_envs, mb):
        if n_envs not in made:
            made[n_envs] = B.make_engine(dev, n_envs)
            if n_envs == B.BIG_N:
                B.load(made[n_envs], B.storage(n_envs, K.T * n_envs))
        if n_envs == K.N:
            B.load(made[n_envs], B.storage(n_envs, mb))
        return made[n_envs]

    return get


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("n_envs,mb", B.CASES, ids=["n%d_mb%d" % c for c in B.CASES])
def test_grad_launch_bits_equal_parent(dev, golden, engines, n_envs, mb, mode):
    import deep_rl_amd as D

    if n_envs == B.BIG_N:   # the tile counts per wave the case is about hold on the 256-workgroup grid of an MI355X
        assert torch.cuda.get_device_properties(dev).multi_processor_count == 256
    eng = engines(n_envs, mb)
    try:
        D.set_contraction(mode)
        got = B.launch(eng, mb)
    finally:
        D.set_contraction("f32")
    for what, bits in got.items():
        want = golden[B.key(n_envs, mb, mode, what)]
        signed = np.int32 if bits.dtype == np.uint32 else np.int64
        same = torch.equal(torch.from_numpy(bits.view(signed)), torch.from_numpy(want.view(signed)))
        assert same, (n_envs, mb, mode, what, int((bits != want).sum()), "elements differ from the recorded build %s" % golden["source_id"])
