"""Cases and the recording recipe of tests/test_gpu_grad_loop_bits.py — TEST INFRASTRUCTURE.

The gradient launch (grad_kernel + grad_reduce_kernel, deep_rl_amd/csrc/mi_grad_kernel.inc and mi_update.hip) must return, bit for bit, what the build BEFORE the
tile loop was reorganised returned (a main loop of full tiles, at most one guarded trailing tile per wave, re-laid LDS, 32-bit gather offsets): the
fixture tests/golden/ppo_grad_parent_bits.npz holds that build's gradient (9,155 f32), four loss terms and the 144 block sums of squares of the slab sum
(`norm_parts`, f64) for every case below under both contraction modes, as raw bit patterns (a one-row minibatch has a NaN actor gradient; NaN == NaN in bits).

The recipe.  On a checkout of the commit before that change, built as usual, on an MI355X:
    python tests/_ppo_grad_bits.py tests/golden/ppo_grad_parent_bits.npz
(this file and tests/_ppo_cases.py, which it imports, copied over if that commit does not have them; they touch nothing but the public engine API).

The cases.  Storage as in tests/_ppo_cases.py (T = 128, N = 9; its init, observation range, old log-prob / value / return construction from a float64 forward
pass, NaN in every row outside the minibatch and in the bootstrap row): one storage per minibatch size 1, 15, 16, 17, 32, 37, 256, 1,151 — one ragged tile alone;
full tiles alone; full tiles and a ragged one in the same launch (up to 72 tiles on 18 workgroups: at these sizes a wave has one tile, full or ragged).  And one storage
of N = 1,024 (131,072 rows, all of them valid, a random permutation): the whole of it = 8,192 tiles, and its first 73,723 rows = 4,608 tiles, the last one ragged.
The tile assignment of grad_body on the 256 workgroups of an MI355X (half = 4 x 128 waves per net and age): rounds = ceil(tiles / 512), the older waves take
(11 rounds + 8) / 16 of them — 8,192 tiles: 16 rounds, 11 and 5 tiles per wave (the production split; odd counts); 4,608 tiles: 9 rounds, 6 and 3 tiles per wave
(an even count >= 4 beside an odd one, and the ragged tile as the third of its wave)."""
import os
import sys

import numpy as np
import torch

import _ppo_cases as K

SMALL_MB = (1, 15, 16, 17, 32, 37, 256, 1151)
BIG_N = 1024
BIG_MB = (K.T * BIG_N, 73723)
CASES = tuple((K.N, mb) for mb in SMALL_MB) + tuple((BIG_N, mb) for mb in BIG_MB)
MODES = ("f32", "bf16x3")
CLIP = 0.2
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_grad_parent_bits.npz")
# where grad_reduce_kernel leaves the block sums of squares inside the workspace (mi_update.hip: ws_norm_parts): behind the (GRAD_MAX_BLOCKS - GRAD_SPARE_SLABS)
# slabs of PART_STRIDE floats and the two spare optimizer-state sets (NORM_PARTS_OFF = 6 STATE_STRIDE floats); NORM_BLOCKS doubles
NORM_PARTS_BYTE = 4 * ((1024 - 16) * 4624 + 6 * 9216)
NORM_BLOCKS = 144


def params(n_envs):
    return K.init_params(np.random.default_rng([7, n_envs]))


def storage(n_envs, valid):
    """-> dict(perm [T n_envs] i32, and the six storage arrays [T + 1, n_envs, ...]): `valid` rows (the first `valid` entries of perm, among them row 0 and the last
    row) hold a plain case of tests/_ppo_cases.py under params(n_envs), every other row NaN"""
    rows = K.T * n_envs
    rng = np.random.default_rng([11, n_envs, valid])
    if valid == 1:
        idx = np.array([rows - 1])
    else:
        idx = np.concatenate([[0, rows - 1], 1 + rng.permutation(rows - 2)[:valid - 2]])
        rng.shuffle(idx)
    perm = np.concatenate([idx, np.setdiff1d(np.arange(rows), idx)]).astype(np.int32)
    obs = (rng.uniform(-1, 1, (valid, 4)) * np.array(K.OBS_RANGE)).astype(K.f32)
    actions = rng.integers(0, 2, valid).astype(np.int64)
    _, lp, v = K._forward64(params(n_envs), obs, actions)
    vals = dict(observations=obs, log_probs=lp - rng.uniform(-0.3, 0.3, valid), advantages=rng.normal(0.3, 1.5, valid),
                values=v + rng.uniform(-0.5, 0.5, valid), returns=v + rng.normal(0, 1, valid))
    s = dict(perm=perm)
    for k, val in vals.items():
        a = np.full((K.T + 1, n_envs) + val.shape[1:], np.nan, K.f32)
        a[:K.T].reshape((rows,) + val.shape[1:])[idx] = val.astype(K.f32)
        s[k] = a
    s["actions"] = np.zeros((K.T + 1, n_envs), np.int64)
    s["actions"][:K.T].reshape(rows)[idx] = actions
    return s


def load(eng, s):
    for name in ("observations", "actions", "log_probs", "advantages", "returns", "values"):
        getattr(eng, name).copy_(torch.from_numpy(s[name]))
    eng.set_perm(s["perm"])


def launch(eng, mb):
    """one gradient launch on the first mb rows of the permutation -> {grads u32 [9155], terms u32 [4], norm_parts u64 [144]}: bit patterns"""
    eng.adv_stats(mb=mb, n_mb=1)
    eng.minibatch_grad(0, mb=mb)
    torch.cuda.synchronize()
    parts = eng.workspace[NORM_PARTS_BYTE:NORM_PARTS_BYTE + 8 * NORM_BLOCKS].clone().view(torch.int64)
    return dict(grads=eng.grads.cpu().numpy().view(np.uint32).copy(), terms=eng.loss_terms.cpu().numpy().view(np.uint32).copy(),
                norm_parts=parts.cpu().numpy().view(np.uint64).copy())


def key(n_envs, mb, mode, what):
    return "n%d_mb%d_%s_%s" % (n_envs, mb, mode, what)


def make_engine(dev, n_envs):
    from test_gpu_parity import _engine

    return _engine(dev, n_envs, params=params(n_envs), T_=K.T, clip_coef=CLIP, ent_coef=K.ENT_COEF, vf_coef=K.VF_COEF)


def record(path):
    import deep_rl_amd as D

    dev = torch.device("cuda", 0)
    out = {}
    engines = {}
    try:
        for n_envs, mb in CASES:
            eng = engines.setdefault(n_envs, make_engine(dev, n_envs))
            load(eng, storage(n_envs, mb if n_envs == K.N else K.T * n_envs))
            for mode in MODES:
                D.set_contraction(mode)
                for what, bits in launch(eng, mb).items():
                    out[key(n_envs, mb, mode, what)] = bits
    finally:
        D.set_contraction("f32")
    from deep_rl_amd import _native

    out["source_id"] = np.array(_native.lib().mi_source_id().decode())   # the build the bits were recorded from
    np.savez_compressed(path, **out)
    print("recorded %d arrays -> %s" % (len(out), path))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
