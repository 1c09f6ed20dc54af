"""The C51 fixtures against the numpy restatement of include/mi_c51.h (tests/_c51_ref.py), on the CPU: the figures the device bounds are derived from."""
import numpy as np
import pytest

from oracle import cpu_ref as R
import _c51_ref as X

f32 = np.float32


@pytest.fixture(scope="module")
def trace():
    return X.load_trace()


@pytest.fixture(scope="module")
def ringv(trace):
    return X.ring(trace)


@pytest.fixture(scope="module")
def ckpts():
    return {k: X.load_ckpt(k) for k in X.CHECKPOINTS}


def test_fixture_self_checks(trace, ckpts):
    t = trace
    assert len(t["actions"]) == 20_000 and t["obs"].shape == (20_000, 4) and t["obs"].dtype == f32
    assert t["batch_inds"].shape == (1001, 128) and t["batch_inds"].dtype == np.int32 and len(t["loss"]) == 1001
    gs = 10_000 + 10 * np.arange(1001)
    assert (t["batch_inds"] >= 0).all() and (t["batch_inds"] < gs[:, None]).all()          # randint(global_step) (c51.py:124)
    assert len(t["episode_return"]) == 1504 and abs(t["loss"][-1] - 3.4029) < 5e-5
    assert t["init_params"].shape == (X.NPARAMS,) and int(t["greedy"].sum()) == 14_223
    assert tuple(t["checkpoints"]) == X.CHECKPOINTS and len(X.CHECKPOINTS) <= 8
    assert {0, 1000} <= set(X.CHECKPOINTS) and {50, 51} <= set(X.CHECKPOINTS)             # first, last, the pair around the target sync at global_step 10,500
    has_term = False
    for k, c in ckpts.items():
        assert int(c["update"][0]) == k and int(c["global_step"][0]) == 10_000 + 10 * k
        assert np.array_equal(c["batch_inds"], t["batch_inds"][k]) and c["loss"][0] == t["loss"][k]
        assert np.abs(c["target_probs"].sum(-1) - 1).max() < 1e-5 and np.abs(c["probs"].sum(-1) - 1).max() < 1e-5
        assert all(v.dtype.kind in "fiu" for v in c.values())
        has_term |= bool(c["batch_terminated"].any())
    assert has_term
    # the target network at a checkpoint is the online network of the last sync (c51.py:166-167): update 0 runs on the initial copy, 1 / 50 behind the sync at 10,000
    assert np.array_equal(ckpts[0]["target_params"], t["init_params"]) and np.array_equal(ckpts[0]["params_before"], t["init_params"])
    assert np.array_equal(ckpts[1]["target_params"], ckpts[0]["params_after"]) and np.array_equal(ckpts[50]["target_params"], ckpts[1]["target_params"])
    assert np.array_equal(ckpts[51]["target_params"], ckpts[50]["params_after"])
    assert np.array_equal(ckpts[1]["params_before"], ckpts[0]["params_after"]) and np.array_equal(ckpts[51]["params_before"], ckpts[50]["params_after"])


def test_atoms_are_the_references():
    import torch
    assert np.array_equal(torch.linspace(-100, 100, steps=101).numpy(), X.ATOMS)


def test_ring_replay_is_bit_exact(trace, ringv):
    """re-stepping the oracle CartPole under the fixture's actions and resets reproduces all 20,000 observations and terminated flags"""
    t = trace
    fr = X.forced_resets(t)
    env = R.VecCartPole(1, seed=1)
    o = env.reset(t["reset_states"][0].reshape(1, 4))
    obs, actions, rewards, term = ringv
    assert np.array_equal(o[0], obs[0])
    got_obs = np.empty((20_000, 4), f32); got_term = np.empty(20_000, np.uint8)
    lines = []
    for g in range(20_000):
        o, _r, d, tr, fret, _fl = env.step(np.array([int(t["actions"][g])]), forced_reset=fr[g].reshape(1, 4))
        got_obs[g] = o[0]; got_term[g] = d[0] and not tr[0]
        if d[0]:
            lines.append((g + 1, float(fret[0])))
    assert np.array_equal(got_obs, obs[1:]) and np.array_equal(got_term, term[1:])
    assert [s for s, _ in lines] == t["episode_global_step"].tolist() and np.array_equal(np.array([r for _, r in lines], f32), t["episode_return"])
    assert (rewards[1:] == 1).all()


def test_restatement_against_every_checkpoint(trace, ringv, ckpts):
    """f32 restatement against the reference's own f32 evaluation: the MEASURED_* figures of tests/_c51_ref.py (each device bound is 8 x its figure)"""
    fig = dict(probs=0.0, target_probs=0.0, q=0.0, loss=0.0, grad=0.0)
    for k, c in ckpts.items():
        Xb, A, Xn, Rw, Tm = X.batch_of(ringv, c["batch_inds"])
        assert np.array_equal(Tm, c["batch_terminated"])
        a32, m32, q32 = X.target(c["target_params"], Xn, Rw, Tm)
        a64, m64, q64 = X.target(c["target_params"], Xn, Rw, Tm, dtype=np.float64)
        far = np.abs(q64[:, 0] - q64[:, 1]) >= X.CLOSE_Q
        assert (~far).mean() <= X.MAX_EXCLUDED
        assert np.array_equal(a32[far], c["next_actions"][far]) and np.array_equal(a64[far], c["next_actions"][far])
        fig["q"] = max(fig["q"], np.abs(q32 - q64).max())
        same = a32 == c["next_actions"]
        fig["target_probs"] = max(fig["target_probs"], np.abs(m32 - c["target_probs"])[same].max())
        p = X.probs_q(c["params_before"], Xb)[0][np.arange(128), A]
        fig["probs"] = max(fig["probs"], np.abs(p - c["probs"]).max())
        # loss and gradient from the reference's own target_probs: what the device's second pass is compared on
        loss, g, _p = X.loss_grad(c["params_before"], Xb, A, c["target_probs"])
        fig["loss"] = max(fig["loss"], abs(float(loss) - c["loss"][0]) / abs(c["loss"][0]))
        fig["grad"] = max(fig["grad"], np.abs(g - c["grads"]).max() / np.abs(c["grads"]).max())
        loss64, g64, _p = X.loss_grad(c["params_before"], Xb, A, c["target_probs"], dtype=np.float64)
        assert abs(loss64 - c["loss"][0]) / abs(c["loss"][0]) < 1e-6 and np.abs(g64 - c["grads"]).max() / np.abs(c["grads"]).max() < 1e-5
    print("measured:", {n: "%.3g" % v for n, v in fig.items()})
    for name, const in (("probs", X.MEASURED_PROBS_ABS), ("target_probs", X.MEASURED_TARGET_PROBS_ABS), ("q", X.MEASURED_Q_ABS), ("loss", X.MEASURED_LOSS_REL),
                        ("grad", X.MEASURED_GRAD_REL)):
        assert const / 2 <= fig[name] <= const, (name, fig[name], const)   # the constants ARE the measurement (rounded up)


def test_projection_is_bit_exact_given_the_references_next_probs(ringv, ckpts):
    """given identical next_probs the projected distribution is a pure function of them, the 101-fold collision of terminated rows included"""
    import torch
    n_term = n_int = 0
    for k, c in ckpts.items():
        _Xb, _A, Xn, Rw, Tm = X.batch_of(ringv, c["batch_inds"])
        W1, b1, W2, b2, W3, b3 = [torch.from_numpy(w.copy()) for w in X.unpack(c["target_params"])]
        with torch.no_grad():   # the reference's network evaluated by torch itself (nn.Linear is x @ W.T + b): the very next_probs of c51.py:141-145
            h = torch.relu(torch.nn.functional.linear(torch.from_numpy(Xn), W1, b1))
            h = torch.relu(torch.nn.functional.linear(h, W2, b2))
            probs = torch.softmax(torch.nn.functional.linear(h, W3, b3).reshape(-1, 2, 101), dim=-1)
            q = torch.sum(probs * torch.from_numpy(X.ATOMS), dim=-1)
            a = torch.argmax(q, -1)
            nxt = probs[torch.arange(128), a].numpy()
        assert np.array_equal(a.numpy(), c["next_actions"])
        m, li, ui, b = X.project(nxt, Rw, Tm)
        assert np.array_equal(m, c["target_probs"])
        assert b.min() >= 1 and b.max() <= 100                      # the clamp of :135 is never active in the real run
        n_term += int(Tm.sum()); n_int += int((li == ui).sum())
        assert ((li == ui).sum(1)[Tm == 0] == 2).all()              # b = 1 at j = 0 and b = 100 at j = 100
    assert n_term > 0 and n_int > 0


def greedy_cases(trace, ringv, k):
    """the greedy decisions that ran on parameters a checkpoint holds: steps [g0 - 10, g0) on params_before, [g0, g0 + 10) on params_after -> [(params, steps)]"""
    c = X.load_ckpt(k)
    g0 = 10_000 + 10 * k
    greedy = np.flatnonzero(trace["greedy"])
    return [(c["params_before"], greedy[(greedy >= g0 - 10) & (greedy < g0)]), (c["params_after"], greedy[(greedy >= g0) & (greedy < g0 + 10)])]


def test_close_action_values_are_rare_in_the_references_run(trace, ringv):
    """the exclusion rule of the action comparisons leaves out at most 1 % of the reference's own greedy decisions, and outside it float64 decides as the reference"""
    obs = ringv[0]
    n = close = 0
    for k in X.CHECKPOINTS:
        for params, steps in greedy_cases(trace, ringv, k):
            if len(steps) == 0:
                continue
            q = X.forward64(params, obs[steps])[1]
            far = np.abs(q[:, 0] - q[:, 1]) >= X.CLOSE_Q
            assert np.array_equal((q[:, 1] > q[:, 0])[far], trace["actions"][steps][far] == 1)
            n += len(steps); close += int((~far).sum())
    assert n >= 50 and close <= X.MAX_EXCLUDED * n
