#!/usr/bin/env python3
"""Greedy policy evaluation throughput on one MI355X: prints ONE JSON line and writes it to --out (default profiles/eval_bench.json; "" writes nothing).

Per head kind of libmirl_eval.so, at E = 1 and E = 4,096 episodes of the controller networks of tests/_eval_ref.py (every episode runs the full 500 steps): the
HIP-event time of ONE mi_ev_episodes launch as the median [min, max] of ``--windows`` windows — a window is the mean over its launches, synchronised at the window
edges only — and from the median episodes/s, env-steps/s and nanoseconds per env step.
``ddqn_act_same_run``: for comparison, in the same process directly behind, the GREEDY acting chunk of mi_ddqn_act_steps (epsilon 0, no learning_starts, the DQN
controller, 50 steps per launch) at 1 and 4,096 envs, timed the same way.  An evaluation step stores no ring row and draws nothing, so per env step at the same
env count it is read against that launch.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deep_rl_amd as D  # noqa: E402
from deep_rl_amd import _native_ddqn as KD, _native_ev as K  # noqa: E402

import _eval_ref as E  # noqa: E402  (the controller networks)

STEPS = 500
CHUNK = 50


def spread(xs, nd=1):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def timed(launch, n_windows, iters, warmup):
    """-> the per-launch microseconds of n_windows windows of `iters` launches each"""
    for _ in range(warmup):
        launch()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            launch()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def figures(us, episodes, steps_per_episode):
    med = statistics.median(us)
    return {"launch_us": spread(us), "episodes_per_s": round(episodes * 1e6 / med, 1), "env_steps_per_s": round(episodes * steps_per_episode * 1e6 / med),
            "ns_per_env_step": round(1e3 * med / (episodes * steps_per_episode), 3)}


def bench_kind(dev, kind, n, args):
    params = torch.from_numpy(np.array(E.controller(kind))).to(dev)
    lengths = torch.zeros(n, dtype=torch.int32, device=dev)
    returns = torch.zeros(n, dtype=torch.float32, device=dev)
    lo, hi = E.DEFAULT_SUPPORT.get(kind, (0.0, 1.0))
    a = K.EVArgs(K.ptr(params), K.ptr(returns), K.ptr(lengths), None, None, None, None, None, args.seed, 1 << 40, E.KIND_ID[kind], n, 0, lo, hi, 0)
    s = K.stream_ptr(dev)

    def launch():
        K.check(K.lib().mi_ev_episodes(a, s), "mi_ev_episodes")

    us = timed(launch, args.windows, args.iters_large if n > 64 else args.iters_small, 2)
    r = figures(us, n, STEPS)
    r["every_episode_ran_500_steps"] = bool((lengths == STEPS).all().item())
    return r


def bench_ddqn_act(dev, n, args):
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=args.seed)
    q, t = D.QNetwork(env), D.QNetwork(env)
    q.load_flat(E.T.controller_dqn(E.T.CONTROLLER_K)); t.load_state_dict(q.state_dict())
    eng = D.DoubleDQNEngine(env, q, t, D.Adam(q, lr=2.5e-4), slots=64, learning_starts=0, start_e=0.0, end_e=0.0, max_episodes_logged=0)
    eng.reset()
    us = timed(lambda: eng.act(CHUNK), args.windows, (args.iters_large if n > 64 else args.iters_small) * (STEPS // CHUNK), 2 * (STEPS // CHUNK))
    r = figures(us, n, CHUNK)
    r.pop("episodes_per_s")
    r["steps_per_launch"] = CHUNK
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters-small", type=int, default=20, help="launches per window at E = 1")
    ap.add_argument("--iters-large", type=int, default=5, help="launches per window at E = 4,096")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"bench": "eval", "device": torch.cuda.get_device_name(0), "eval_source_id": K.source_id(), "ddqn_source_id": KD.source_id(), "windows": args.windows,
           "launches_per_window": {"E1": args.iters_small, "E4096": args.iters_large}, "seed": args.seed, "default_workgroups": K.DEFAULT_WORKGROUPS,
           "workload": "controller networks, every episode 500 steps", "sync": "window edges only"}
    for kind in E.KINDS:
        res[kind] = {"E1": bench_kind(dev, kind, 1, args), "E4096": bench_kind(dev, kind, 4096, args)}
    res["ddqn_act_same_run"] = {"n1": bench_ddqn_act(dev, 1, args), "n4096": bench_ddqn_act(dev, 4096, args)}
    res["ns_per_env_step_vs_ddqn_act"] = {kind: {"E1": round(res[kind]["E1"]["ns_per_env_step"] / res["ddqn_act_same_run"]["n1"]["ns_per_env_step"], 3),
                                                 "E4096": round(res[kind]["E4096"]["ns_per_env_step"] / res["ddqn_act_same_run"]["n4096"]["ns_per_env_step"], 3)}
                                          for kind in E.KINDS}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
