#!/usr/bin/env python3
"""REINFORCE throughput on one MI355X: prints ONE JSON line.

For N = 1 and N = 4,096 envs (``--envs``): env-steps/s and updates/s of ``ReinforceEngine.update()`` as the median of ``--windows`` windows of ``--updates``
updates after ``--warmup`` updates, synchronised at the window edges only (the per-update sum of the episode lengths is accumulated on the device).  Throughput
depends on the episode length, and the policy improves while it is timed, so two kinds of window are measured and each reports its mean episode length:
  fixed     learning rate 0: the parameters stay the seeded initial ones, every window sees the same length distribution
  learning  the script's learning rate, windows in sequence (episodes lengthen from window to window)
``per_kernel_us``: HIP-event times of the four pieces called one by one (rollout, returns, grad = slab launch + slab sum, Adam through libmirl's mi_adam) at fixed
parameters, median over the updates of one window (``per_kernel_us_after_learning``: the same behind the learning windows, at their episode lengths).  The baseline to read it against is the unmodified reference on one CPU core at its own shape
(``tools/capture_reinforce_ref.py --time-only``); there is no earlier version of this path to compare with.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import deep_rl_amd as D  # noqa: E402
from deep_rl_amd import _native as N, _native_pg as PG  # noqa: E402


def make(n, seed, lr):
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed)
    torch.manual_seed(seed)
    agent = D.DropoutPolicy(env)
    opt = D.Adam(agent, lr=lr)
    return D.ReinforceEngine(env, agent, opt)


def windows(eng, n_windows, updates):
    out = []
    for _ in range(n_windows):
        steps = torch.zeros((), dtype=torch.int64, device=eng.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(updates):
            eng.update()
            steps += eng.lengths.sum()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        s = int(steps)
        out.append({"updates_per_s": updates / dt, "env_steps_per_s": s / dt, "mean_episode_length": s / (updates * eng.num_envs)})
    med = lambda k: statistics.median(w[k] for w in out)   # noqa: E731
    return {"median_updates_per_s": round(med("updates_per_s"), 1), "median_env_steps_per_s": round(med("env_steps_per_s")),
            "mean_episode_length_per_window": [round(w["mean_episode_length"], 1) for w in out],
            "env_steps_per_s_per_window": [round(w["env_steps_per_s"]) for w in out]}


def per_kernel(eng, updates):
    names = ("rollout", "returns", "grad", "adam")
    calls = (eng.rollout, eng.compute_returns, eng.grad, eng.optimizer_step)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in names] for _ in range(updates)]
    for u in range(updates):
        for k, call in enumerate(calls):
            ev[u][k][0].record(); call(); ev[u][k][1].record()
    torch.cuda.synchronize()
    return {nm: round(statistics.median(ev[u][k][0].elapsed_time(ev[u][k][1]) for u in range(updates)) * 1e3, 1) for k, nm in enumerate(names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,4096")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    res = {"bench": "reinforce", "device": torch.cuda.get_device_name(0), "pg_source_id": PG.source_id(), "mirl_source_id": N.lib().mi_source_id().decode(),
           "windows": args.windows, "updates_per_window": args.updates, "warmup_updates": args.warmup, "seed": args.seed, "sync": "window edges only"}
    for n in [int(x) for x in args.envs.split(",")]:
        fixed = make(n, args.seed, 0.0)
        for _ in range(args.warmup):
            fixed.update()
        r = {"fixed": windows(fixed, args.windows, args.updates), "per_kernel_us": per_kernel(fixed, args.updates)}
        learn = make(n, args.seed, 1e-2)
        for _ in range(args.warmup):
            learn.update()
        r["learning"] = windows(learn, args.windows, args.updates)
        r["per_kernel_us_after_learning"] = per_kernel(learn, args.updates)   # the same four pieces at the episode lengths of the last window
        r["finite"] = bool(torch.isfinite(learn.agent.flat).all())
        res["n%d" % n] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
