"""mdqn_grad_kernel, mdqn_target_kernel and mdqn_reduce_kernel (deep_rl_amd/csrc/mi_mdqn.hip) on the synthetic rings of tests/_mdqn_cases.py (validated on the CPU by
tests/test_mdqn_cases_cpu.py) against FLOAT64 AUTOGRAD over the paper's own form of the target (tests/_mdqn_ref.py), through MunchausenDQNEngine with forced
indices: one row in the last slot of a two-slot ring, 5 rows, one row more than the gradient launch has workgroups, a batch whose workgroups walk three rows, heads
of 30 with bonuses clipped, inside and exactly 0, tau = 1, a tau at which the soft-max is a hard max, alpha 0 and 1, whole batches with live == 0 and live == 1, gamma
0 and 1, a target head that ties bit for bit, pre-activations of exactly 0, and the case on which every output is Double DQN's.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_mdqn_ref.BOUND = max(8 x the float32 torch evaluation's measured distance from float64, the bar the suite holds DQN to).  No case and no row is excluded, action
comparisons included.  Observed maxima go to mdqn_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _dqn_cases as D
import _mdqn_cases as K
import _mdqn_ref as X

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def make_engine(dev, n, slots, params=None, target=None, seed=1, base=0, batch_size=128, cls=None, **kw):
    """MunchausenDQNEngine (or `cls`) as the script builds it: two plain QNetworks and deep_rl_amd.Adam at optim.Adam's defaults"""
    import deep_rl_amd as A

    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    torch.manual_seed(seed)
    q, tq = A.QNetwork(env), A.QNetwork(env)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    return (cls or A.MunchausenDQNEngine)(env, q, tq, A.Adam(q, lr=X.LR), slots=slots, batch_size=batch_size, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).copy().view(np.uint32)


def record(key, value):
    path = os.path.join(X.results_dir(), "mdqn_gpu_maxima.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    if "family" in value:
        fam = d.setdefault("family_maxima", {}).setdefault(value["family"], {})
        for k in X.FIGURES:
            if k in value:
                fam[k] = max(fam.get(k, 0.0), value[k])
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _engine(dev, c, cls=None):
    (N, S) = c["ring"]
    kw = {} if cls is not None else c["hp"]
    eng = make_engine(dev, N, S, params=c["params"], target=c["target"], batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0, cls=cls, **kw)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S                                    # min(global_step, slots) * N: every transition of the ring is stored
    return eng


FLOATS = ("grads", "loss", "target_values", "current", "bonus", "soft_value")


def _result(eng):
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target=_np(eng.target_values).astype(np.float64),
               current=_np(eng.current).astype(np.float64), bonus=_np(eng.bonus).astype(np.float64), soft_value=_np(eng.soft_value).astype(np.float64),
               next_actions=_np(eng.next_actions).astype(np.int64))
    return got, [_bits(getattr(eng, n)) for n in FLOATS] + [_np(eng.next_actions).copy()]


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(dev, i):
    c = K.make_case(i)
    fam, e = c["family"], c["exp"]
    alpha, tau, clip_lo = (f32(c["hp"][k]) for k in ("alpha", "tau", "clip_lo"))
    eng = _engine(dev, c)
    assert (eng.N, eng.slots, eng.batch_size, eng.gamma) == (c["ring"][0], c["ring"][1], c["mb"], c["gamma"])
    assert (eng.alpha, eng.tau, eng.clip_lo) == (c["hp"]["alpha"], c["hp"]["tau"], c["hp"]["clip_lo"])
    eng.sample(c["idx"])
    eng.target()
    alone = [_bits(eng.target_values), _bits(eng.bonus), _bits(eng.soft_value), _np(eng.next_actions).copy()]
    assert not _np(eng.grads).any() and not _np(eng.current).any()                       # mi_md_target writes its four outputs and nothing else
    eng.grad()
    got, bits = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(alone, [bits[2], bits[4], bits[5], bits[6]])), "mi_md_target is not the gradient launch's first pass"
    eng.grad()
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "next_actions differ on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    fig = X.figures(e, got, fam)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=c["mb"]))
    assert set(fig) == set(X.FIGURES)
    assert not X.within(fig, fam), (c["name"], X.within(fig, fam))
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    # the clamp: a row the float64 reference clips holds clip_lo itself, none lies outside [clip_lo, 0]
    bonus32 = _np(eng.bonus)
    assert (bonus32 <= 0).all() and (bonus32 >= clip_lo).all() and np.array_equal(bonus32 == clip_lo, e["slp"] < float(clip_lo))
    if fam == "clip":
        assert np.array_equal(bonus32 == 0, e["bonus"] == 0) and (bonus32 == 0).sum() >= 1 and (bonus32 == clip_lo).sum() >= 3
    if fam == "target_tie":                                # a bit-for-bit tie: action 0, ln pi = -ln 2 for both actions
        assert not got["next_actions"].any()
        assert np.abs(got["bonus"] - max(-float(tau) * np.log(2.0), float(clip_lo))).max() <= X.BOUND[fam]["bonus"] and len(np.unique(bonus32)) == 1
    if c["tau_rule"] == "underflow":                       # expf underflows to 0: the soft value IS the target network's larger action value, to the bit
        from deep_rl_amd import _native_ddqn as DQ
        N, S = c["ring"]
        xn = torch.from_numpy(c["observations"].reshape(-1, 4)[D.successor(c["idx"], N, S)]).to(dev).contiguous()
        qt = torch.empty((c["mb"], 2), dtype=torch.float32, device=dev)
        DQ.check(DQ.lib().mi_ddqn_forward(DQ.ptr(eng.target_network.flat), DQ.ptr(xn), c["mb"], DQ.ptr(qt), eng._s()), "mi_ddqn_forward")
        assert np.array_equal(_bits(eng.soft_value), _bits(qt.max(dim=1).values)), "soft_value is not the target network's maximum where the soft-max underflows"
    if fam == "ddqn_identity":                             # alpha = 0, a hard max, synced networks: Double DQN bit for bit
        import deep_rl_amd as A
        dd = _engine(dev, c, cls=A.DoubleDQNEngine)
        dd.sample(c["idx"])
        dd.grad()
        for name in ("grads", "loss", "target_values", "current", "next_actions"):
            assert np.array_equal(_np(getattr(eng, name)).view(np.uint32), _np(getattr(dd, name)).view(np.uint32)), "%s is not DoubleDQNEngine.grad()'s" % name
    if c["name"] == "terminal_all_9":                      # live == 0 in every row: another target vector moves the bonus, not the bootstrap
        eng.target_network.load_flat(np.random.default_rng(99).normal(0, 1, X.NP).astype(np.float32))
        eng.grad()
        got3, _ = _result(eng)
        assert np.abs(got3["bonus"] - got["bonus"]).max() > 1e-3, "the bonus is masked by terminated"
        r = c["rewards"].reshape(-1)[D.successor(c["idx"], *c["ring"])].astype(np.float64)
        for g in (got, got3):                              # target - alpha * bonus is the reward: within one rounding of the sum r + alpha * bonus
            assert np.abs((g["target"] - float(alpha) * g["bonus"]) - r).max() <= 2.0 ** -23 * (np.abs(r).max() + 1.0)
        assert np.isfinite(got3["soft_value"]).all() and np.abs(got3["soft_value"] - got["soft_value"]).max() > 1e-3
    # train_step(idx) from fresh optimizer state: the same gradient bit for bit, parameters that are one Adam step on it
    step = _engine(dev, c)
    step.train_step(c["idx"])
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "train_step's outputs are not grad()'s bits"
    p = c["params"].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    X.adam_step(p, got["grads"], m, v, 1)
    after = _np(step.q.flat)
    assert step.optimizer.step_count == 1 and step.update_index == 1
    assert np.abs(after - p).max() <= 1e-6                 # (the bound of tests/test_gpu_ddqn_cases.py: a step of at most lr in f32, p - step rounded once)
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits
