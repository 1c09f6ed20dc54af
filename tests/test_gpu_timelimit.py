"""The 500-step TimeLimit inside the acting kernels — dqn_act4_kernel (mi_dqn.hip, through DQNEngine's lazy-statistics and logged entries, the dueling engine's
packed image and PERDQNEngine's PER = true instantiation), c51_act_kernel (mi_c51.hip) and iqn_act_kernel (mi_iqn.hip) — against the CPU oracle.

Every comparison is exact (np.array_equal; the oracle runs its device-matched sin/cos): ring, carried observation, fp64 env state, `elapsed`, per-call statistics
and the episode log.  The cases and their expectations come from tests/_timelimit_cases.py; tests/test_timelimit_cases_cpu.py shows on the CPU that they hold the
edges (truncation on the first / a middle / the last step of a launch, termination at length exactly 500 and 499, two truncations of one env, short episodes beside
long ones) and that `terminated := done`, a limit of 499 or 501, or an `elapsed` that survives a termination would change these expectations.

What each run compared goes to timelimit_gpu_compared.json in the tests' results directory."""
import json
import os

import numpy as np
import pytest

import _timelimit_cases as T

pytestmark = pytest.mark.gpu

ALGO = {"dqn_lazy": "dqn", "dqn_log": "dqn", "dueling": "dueling", "per": "dqn", "per_lazy": "dqn", "c51": "c51", "iqn": "iqn"}
DQN_FAMILY = ("dqn_lazy", "dqn_log", "dueling", "per", "per_lazy")
FIELDS = ("observations", "actions", "rewards", "terminated")


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def R():
    from oracle import cpu_ref
    return cpu_ref


def _np(t):
    return t.detach().cpu().numpy()


_COMPARED = {}


def _record(test, kind, case, envs=None):
    import _c51_ref as X
    k = case.counts(envs)
    rec = _COMPARED.setdefault(test, {}).setdefault(kind, {"runs": 0, "truncations": 0, "terminated_at_500": 0, "terminated_at_499": 0, "envs_truncated_twice": 0})
    rec["runs"] += 1
    for f in ("truncations", "terminated_at_500", "terminated_at_499", "envs_truncated_twice"):
        rec[f] += k[f]
    path = os.path.join(X.results_dir(), "timelimit_gpu_compared.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(_COMPARED)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)
    print("compared", test, kind, json.dumps(k))


def _make(dev, kind, n, slots, seed=5, base=300, params=None, greedy=False):
    """an engine of `kind` over n envs; params: the flat parameter vector (default: zeros — the teacher-forced paths run no forward); greedy: epsilon 0 from step 0"""
    import torch

    import deep_rl_amd as D
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed, env_id_base=base)
    algo = ALGO[kind]
    if algo in ("dqn", "dueling"):
        Net = D.DuelingQNetwork if algo == "dueling" else D.QNetwork
        q, tgt = Net(env), Net(env)
        q.load_flat(np.zeros(q.flat.numel(), np.float32) if params is None else params)
        tgt.load_state_dict(q.state_dict())
        Eng = {"dueling": D.DuelingDQNEngine, "per": D.PERDQNEngine, "per_lazy": D.PERDQNEngine}.get(kind, D.DQNEngine)
        kw = dict(learning_starts=0, start_e=0.0, end_e=0.0) if greedy else {}
        return Eng(env, q, tgt, D.ClipAdam(q, lr=2.5e-4, eps=1e-8), slots=slots, max_episodes_logged=4096 if kind in ("dqn_log", "per") else 0, **kw)
    if algo == "c51":
        q, tgt = D.C51QNetwork(env, n_atoms=101), D.C51QNetwork(env, n_atoms=101)
        q.load_flat(np.zeros(q.flat.numel(), np.float32) if params is None else params)
        tgt.load_state_dict(q.state_dict())
        kw = dict(start_e=0.0, end_e=0.0) if greedy else {}
        return D.C51Engine(env, q, tgt, D.Adam(q, lr=2.5e-4, eps=0.01 / 128), slots=slots, max_episodes_logged=8192, **kw)
    import _iqn_ref as Q
    p = torch.from_numpy(np.zeros(Q.NPARAMS, np.float32) if params is None else np.asarray(params, np.float32).copy()).to(dev)
    kw = dict(final_epsilon=0.0, epsilon_decay_steps=1, learning_starts=0) if greedy else {}
    return D.IQNEngine(env, p, p.clone(), D.Adam(p, lr=5e-5, eps=1e-2 / 32), slots=slots, max_episodes_logged=8192, **kw)


def _check_ring(eng, case, G, slots, tag):
    want = case.ring(G, slots)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(eng, f)), want[f]), (tag, G, f)


def _snapshot(eng):
    st, el = eng.env.get_state()
    snap = dict(observation=_np(eng.observation).copy(), state=_np(st), elapsed=_np(el), stats=eng.episode_stats.tolist())
    if eng.max_ep:
        snap["log"] = eng.drain_episodes()
    return snap


def _check_call(snap, case, g0, k, tag):
    """what one call left behind: carried observation, fp64 state and `elapsed` in the env handle, the launch statistics, the episode log"""
    g = g0 + k
    assert np.array_equal(snap["observation"], case.obs[g]), (tag, g, "observation")
    assert np.array_equal(snap["state"], case.state[g]), (tag, g, "state")
    assert np.array_equal(snap["elapsed"], case.elapsed[g]), (tag, g, "elapsed", snap["elapsed"], case.elapsed[g])
    assert snap["stats"][:3] == case.stats(g0, k), (tag, g, "episode_stats", snap["stats"], case.stats(g0, k))
    if "log" in snap:
        cnt, eps = snap["log"]
        assert cnt == case.stats(g0, k)[0] and eps == case.episodes(g0, k), (tag, g, "episode log")


def _run_forced(eng, case, call_list, slots, ring_every_call, tag, g0=0):
    """teacher-forced: the case's actions (and its reset states in the forced form) through eng.act in calls of call_list, everything compared after every call"""
    import torch
    g = g0
    for k in call_list:
        fr = None if case.forced_resets is None else torch.from_numpy(case.forced_resets[g:g + k])
        eng.act(k, forced_actions=torch.from_numpy(case.actions[g:g + k]), forced_resets=fr)
        _check_call(_snapshot(eng), case, g, k, tag)
        g += k
        assert eng.global_step == g
        if ring_every_call:
            _check_ring(eng, case, g, slots, tag)
    _check_ring(eng, case, g, slots, tag)
    return g


def _start(eng, case):
    assert np.array_equal(_np(eng.reset()), case.obs[0])


# ---- a. teacher-forced acting -------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
@pytest.mark.parametrize("kind", list(ALGO))
def test_teacher_forced_acting_at_the_limit(dev, kind, forced, schedule):
    """1,100 steps of the scripted cases (37 envs for the DQN family: three 16-env workgroups with a ragged tail; 5 envs for C51 / IQN).  One run on a ring that holds
    the whole run, compared at the end; one on 16 slots (the ring wraps ~70 times), compared after every call.  (PER: 64 slots, 17 wraps — a PER acting call
    marks the rows it writes and must be shorter than the ring, mi_per_act_steps: n_steps in [1, slots).)"""
    case = T.get("dqn37" if kind in DQN_FAMILY else "n5", forced)
    call_list = T.calls(schedule, case.steps)
    small = 64 if kind in ("per", "per_lazy") else 16
    assert max(call_list) > 16 or schedule == "7"      # a call of 49 / 50 steps laps the 16-slot ring three times by itself
    for slots, every in ((case.steps + 1, False), (small, True)):
        eng = _make(dev, kind, case.n, slots)
        _start(eng, case)
        _run_forced(eng, case, call_list, slots, every, (kind, forced, schedule, slots))
        if slots > case.steps:      # the stored flag is `terminated`, not `done`: the two differ exactly on the truncated steps
            differ = _np(eng.terminated)[1:] != case.done.astype(np.uint8)
            assert np.array_equal(differ, case.trunc) and differ.sum() == case.counts()["truncations"] >= 2
        _record("a_teacher_forced", kind, case)


# ---- b. several envs per workgroup --------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", T.SCHEDULES)
@pytest.mark.parametrize("forced", [False, True], ids=["keyed", "forced"])
@pytest.mark.parametrize("kind", ["c51", "iqn"])
def test_two_envs_per_workgroup(dev, kind, forced, schedule):
    """1,030 envs on a grid capped at 1,024 workgroups: workgroups 0 - 5 walk envs (w, 1024 + w), twelve long-episode envs with different outcomes.  All 1,030 envs are
    compared (the twelve and every other one); the launch statistics are sums over all of them."""
    case = T.get("n1030", forced)
    assert case.n > 1024 and all(case.kinds[i] in T.LONG_KINDS for i in T.SHARED_1030)
    slots, every = (16, True) if schedule == "7" else (case.steps + 1, False)
    eng = _make(dev, kind, case.n, slots)
    _start(eng, case)
    _run_forced(eng, case, T.calls(schedule, case.steps), slots, every, (kind, forced, schedule, slots))
    _record("b_two_envs_per_workgroup", kind, case, T.SHARED_1030)


# ---- c. the production branch at epsilon 0 ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dqn_lazy", "dqn_log", "dueling", "per", "c51", "iqn"])
def test_greedy_controller_runs_into_the_limit(dev, R, kind):
    """FORCED = false: a hand-built controller network (q_1 - q_0 = K w . obs) acts greedily for 1,100 steps.  The device's own actions are replayed on the oracle:
    ring, flags, statistics, log and `elapsed` exact; the action is (q_1 > q_0) of a float64 forward wherever the two values are at least the project's close-value
    distance apart (at most 1 % left out); at least one env is truncated twice."""
    algo = ALGO[kind]
    n, steps = (37 if kind in DQN_FAMILY else 5), 1100
    slots = steps + 1
    params = T.CONTROLLERS[algo](T.CONTROLLER_K)
    eng = _make(dev, kind, n, slots, params=params, greedy=True)
    g_first = slots if algo == "iqn" else 0      # IQN's epsilon is 1 at global step 0 whatever the schedule: start one ring length later (the same slots)
    eng.global_step = g_first
    eng.reset()
    snaps, call_list = [], T.calls("49+50", steps)
    for k in call_list:
        eng.act(k)
        snaps.append(_snapshot(eng))
    assert eng.global_step == g_first + steps
    actions = _np(eng.actions)[:steps]
    assert set(np.unique(actions).tolist()) == {0, 1}
    case = T.replay(R, n, 5, 300, actions)
    g = 0
    for k, snap in zip(call_list, snaps):
        _check_call(snap, case, g, k, kind)
        g += k
    _check_ring(eng, case, steps, slots, kind)
    k = case.counts()
    assert k["envs_truncated_twice"] >= 1 and k["truncations"] >= 2, k
    q = T.q64(algo, params, case.obs[:-1].reshape(-1, 4))
    far = np.abs(q[:, 1] - q[:, 0]) >= T.close_q(algo)
    assert (~far).mean() <= 0.01, int((~far).sum())
    assert np.array_equal(actions.reshape(-1)[far], (q[:, 1] > q[:, 0]).astype(np.int64)[far])
    print(kind, "greedy decisions", far.size, "left out", int((~far).sum()))
    _record("c_greedy", kind, case)


# ---- d. checkpoint inside a long episode --------------------------------------------------------------------------
def _checkpoint_inside_a_long_episode(make, case, nparams, path, label):
    """the body of the test below for any ring engine; make(n, slots, params=None) builds one (tests/test_gpu_qrdqn_cases.py runs it on QRDQNEngine)"""
    import torch

    from deep_rl_amd import checkpoint
    assert {T.K0, T.K1A, T.K1B} <= set(case.kinds.tolist()) and case.trunc[499].any() and not case.trunc[300:499].any()
    slots = 64
    rng = np.random.default_rng(3)
    a = make(case.n, slots, params=rng.normal(0, 0.05, nparams).astype(np.float32))
    _start(a, case)
    _run_forced(a, case, T.calls("50", 300), slots, False, (label, "before"))
    path = checkpoint.save(path, a)
    b = make(case.n, slots)
    b.reset()
    b.act(13, forced_actions=torch.zeros((13, case.n), dtype=torch.int64))
    assert not np.array_equal(_np(b.env.get_state()[1]), case.elapsed[300])
    checkpoint.load(path, b)
    assert b.global_step == 300 and np.array_equal(_np(b.q.flat), _np(a.q.flat)) and np.array_equal(_np(b.env.get_state()[1]), case.elapsed[300])
    for eng, tag in ((a, "uninterrupted"), (b, "resumed")):
        assert _run_forced(eng, case, T.calls("50", 320), slots, True, (label, tag), g0=300) == 620
    for f in FIELDS + ("observation",):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), f
    for x, y in zip(a.env.get_state(), b.env.get_state()):
        assert np.array_equal(_np(x), _np(y))


@pytest.mark.parametrize("kind", ["dqn_log", "c51", "iqn"])
def test_checkpoint_inside_a_long_episode(dev, kind, tmp_path):
    """saved at global step 300, loaded into a fresh engine (zeroed parameters; its env first driven somewhere else: other state, `elapsed`, episode and step
    counters) and continued to step 620: ring, `elapsed`, log and statistics equal the uninterrupted run bit for bit, and the truncation comes at step 500.
    (checkpoint.load refuses an env of another seed by design — the keys of every later reset belong to the seed — so the fresh engine's env has the same seed.)"""
    case = T.get("dqn37" if kind in DQN_FAMILY else "n5", False)
    _checkpoint_inside_a_long_episode(lambda n, slots, params=None: _make(dev, kind, n, slots, params=params), case,
                                      {"dqn": 10934, "c51": 27934, "iqn": 44898}[ALGO[kind]], str(tmp_path / kind), kind)


# ---- e. reset() inside an episode ---------------------------------------------------------------------------------
_RESET_CASES = {}


def _reset_case(R, n):
    if n not in _RESET_CASES:
        sim = T.Sim(R, n, 5, 300)
        o = sim.reset()
        for g in range(820):
            if g == 300:
                o = sim.reset()
            o = sim.step(T.rule(o))
        _RESET_CASES[n] = sim.case()
    return _RESET_CASES[n]


def _reset_inside_an_episode(make, case, label):
    """the body of the test below for any ring engine; make(n, slots) builds one"""
    assert case.truncation_steps() == [(799, e) for e in range(case.n)] and (case.fin_len[799] == 500).all() and (case.elapsed[500] == 200).all()
    slots = 64
    eng = make(case.n, slots)
    _start(eng, case)
    # the record holds the observation reset() left in front of step 300; the one the 300th step produced is checked here
    import torch
    g = 0
    for k in T.calls("50", 300):
        eng.act(k, forced_actions=torch.from_numpy(case.actions[g:g + k]))
        g += k
    assert (_np(eng.env.get_state()[1]) == 300).all()
    assert np.array_equal(_np(eng.reset()), case.obs[300]) and (_np(eng.env.get_state()[1]) == 0).all()
    _run_forced(eng, case, T.calls("50", 520), slots, True, (label, "after reset"), g0=300)


@pytest.mark.parametrize("kind", ["dqn_lazy", "dqn_log", "c51", "iqn"])
def test_reset_inside_an_episode_restarts_the_limit(dev, R, kind):
    """300 balanced steps, reset(), 520 more: no truncation at step 500, every env truncated 500 steps after the reset, as the oracle's reset() has it"""
    case = _reset_case(R, 37 if kind in DQN_FAMILY else 5)
    _reset_inside_an_episode(lambda n, slots: _make(dev, kind, n, slots), case, kind)
    _record("e_reset", kind, case)
