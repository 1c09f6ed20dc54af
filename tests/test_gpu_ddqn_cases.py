"""ddqn_grad_kernel, ddqn_target_kernel and ddqn_reduce_kernel (deep_rl_amd/csrc/mi_ddqn.hip) on the synthetic rings of tests/_ddqn_cases.py (validated on the CPU by
tests/test_ddqn_cases_cpu.py) against FLOAT64 AUTOGRAD (tests/_ddqn_ref.py), through DoubleDQNEngine with forced indices: one row in the last slot of a two-slot
ring, 5 rows, one row more than the gradient launch has workgroups, a batch whose workgroups walk three rows, target == online bit for bit, an online head that ties
bit for bit, whole batches with live == 0 and live == 1, gamma 0 and 1, action values of 30, pre-activations of exactly 0.

Everything the batch does not reference holds NaN (observations, rewards), 2 (actions) or 1 (terminated), so a stray read shows in the result.  Bounds:
_ddqn_ref.BOUND = max(8 x the float32 torch evaluation's measured distance from float64, the bar the suite holds DQN to).  No case and no row is excluded, action
comparisons included.  Observed maxima go to ddqn_gpu_maxima.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest
import torch

import _ddqn_cases as K
import _ddqn_ref as X
import _dqn_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def make_engine(dev, n, slots, params=None, target=None, seed=1, base=0, batch_size=128, **kw):
    """DoubleDQNEngine as the script builds it: two plain QNetworks and deep_rl_amd.Adam at optim.Adam's defaults"""
    import deep_rl_amd as A

    env = A.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    torch.manual_seed(seed)
    q, tq = A.QNetwork(env), A.QNetwork(env)
    tq.load_state_dict(q.state_dict())
    if params is not None:
        q.load_flat(params)
    if target is not None:
        tq.load_flat(target)
    return A.DoubleDQNEngine(env, q, tq, A.Adam(q, lr=X.LR), slots=slots, batch_size=batch_size, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).copy().view(np.uint32)


def record(key, value):
    path = os.path.join(X.results_dir(), "ddqn_gpu_maxima.json")
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


def _engine(dev, c):
    (N, S) = c["ring"]
    eng = make_engine(dev, N, S, params=c["params"], target=c["target"], batch_size=c["mb"], gamma=c["gamma"], max_episodes_logged=0)
    for name in ("observations", "actions", "rewards", "terminated"):
        getattr(eng, name).copy_(torch.from_numpy(c[name]))
    eng.global_step = S                                    # min(global_step, slots) * N: every transition of the ring is stored
    return eng


def _result(eng):
    got = dict(grads=_np(eng.grads).astype(np.float64), loss=float(eng.loss.item()), target=_np(eng.target_values).astype(np.float64),
               current=_np(eng.current).astype(np.float64), next_actions=_np(eng.next_actions).astype(np.int64))
    return got, [_bits(eng.grads), _bits(eng.loss), _bits(eng.target_values), _bits(eng.current), _np(eng.next_actions).copy()]


@pytest.mark.parametrize("i", range(len(K.SPECS)), ids=K.NAMES)
def test_case_against_float64(dev, i):
    c = K.make_case(i)
    fam, e = c["family"], c["exp"]
    eng = _engine(dev, c)
    assert (eng.N, eng.slots, eng.batch_size, eng.gamma) == (c["ring"][0], c["ring"][1], c["mb"], c["gamma"])
    eng.sample(c["idx"])
    eng.target()
    alone = (_np(eng.next_actions).copy(), _bits(eng.target_values))
    eng.grad()
    got, bits = _result(eng)
    assert np.array_equal(alone[0], got["next_actions"]) and np.array_equal(alone[1], bits[2]), "mi_ddqn_target is not the gradient launch's first pass"
    eng.grad()
    _, bits2 = _result(eng)
    assert all(np.array_equal(a, b) for a, b in zip(bits, bits2)), "a second identical launch differs"
    for k, v in got.items():
        assert np.isfinite(v).all(), "NaN / inf in %s: something outside the batch's rows and successors was read, or the arithmetic overflowed" % k
    assert np.array_equal(got["next_actions"], e["next_actions"]), "a* differs on rows %s" % np.flatnonzero(got["next_actions"] != e["next_actions"])
    if fam == "online_tie":
        assert not got["next_actions"].any()               # torch.argmax: a bit-for-bit tie goes to action 0
    obs = np.concatenate([c["observations"].reshape(-1, 4)[c["idx"]], c["observations"].reshape(-1, 4)[D.successor(c["idx"], *c["ring"])]])
    got["q"], got["q_ref"] = _np(eng.forward(torch.from_numpy(obs))).astype(np.float64), X.forward(c["params"], obs)
    fig = X.figures(e, got, fam)
    print(c["name"], {k: float("%.3g" % v) for k, v in fig.items()}, got["loss"], e["loss"])
    record(c["name"], dict(fig, family=fam, mb=c["mb"]))
    assert set(fig) == set(X.FIGURES)
    assert not X.within(fig, fam), (c["name"], X.within(fig, fam))
    zero = e["grads"] == 0
    assert not got["grads"][zero].any(), "the float64 gradient is exactly 0 in %d elements; the device's is not in %d of them" % (zero.sum(), np.count_nonzero(got["grads"][zero]))
    if fam == "synced":                                    # Double DQN == DQN: the C oracle's plain DQN within the bar the suite holds DQN to
        from oracle import cpu_ref as R
        og, ol = R.dqn_td_grads(c["params"], c["params"], D.storage(R, c), c["idx"], gamma=c["gamma"])
        assert np.abs(got["grads"] - og).max() <= D.BAR["dqn"]["grad"] * np.abs(og).max() and abs(got["loss"] - ol) <= D.BAR["dqn"]["loss"] * abs(ol)
    if c["name"] == "terminal_all_9":                      # live == 0 in every row: another target vector, the same bits
        eng.target_network.load_flat(np.random.default_rng(99).normal(0, 1, X.NP).astype(np.float32))
        eng.grad()
        _, bits3 = _result(eng)
        assert all(np.array_equal(a, b) for a, b in zip(bits[:4], bits3[:4])), "the target net reaches a batch whose successors are all terminated"
        assert np.array_equal(bits[4], bits3[4])           # (a* is the online network's: it does not move either)
    # train_step(idx) from fresh optimizer state: the same gradient bit for bit, parameters that are one Adam step on it
    step = _engine(dev, c)
    step.train_step(c["idx"])
    _, sbits = _result(step)
    assert all(np.array_equal(a, b) for a, b in zip(bits, sbits)), "train_step's gradient / loss / target / current are not grad()'s bits"
    p = c["params"].astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    X.adam_step(p, got["grads"], m, v, 1)
    after = _np(step.q.flat)
    assert step.optimizer.step_count == 1 and step.update_index == 1
    assert np.abs(after - p).max() <= 1e-6                 # (the bound of tests/test_gpu_qrdqn_cases.py: a step of at most lr in f32, p - step rounded once)
    assert np.array_equal(after[zero].view(np.uint32), c["params"][zero].view(np.uint32))   # a parameter whose gradient is exactly 0 keeps its bits
