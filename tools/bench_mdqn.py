#!/usr/bin/env python3
"""Munchausen DQN throughput on one MI355X: prints ONE JSON line and writes it to --out (default profiles/mdqn_bench.json; "" writes nothing).

The method and the shapes of tools/bench_ddqn.py (its ``windows`` / ``per_launch`` are imported, not restated): for each (envs, slots) of ``--shapes`` (default: the
script's shape 1 env x 100,001 slots, and 4,096 envs x 256 slots) at batch 128: env-steps/s, updates/s and microseconds per iteration of the script's loop — one
iteration = 10 env steps of every env (one launch, libmirl_ddqn.so's) + one update (two launches, libmirl_mdqn.so's), the target sync every 50th — as the median of
``--windows`` windows of ``--iters`` iterations after ``--warmup`` iterations, synchronised at the window edges only, and ``per_launch_us``: HIP-event times of the
loop's three launches.
``ddqn_same_run``: the same figures of DoubleDQNEngine, measured by the same code in the same process directly behind each Munchausen shape.  The figure of interest
is ``gradient_launch_vs_ddqn``: the median gradient launch against Double DQN's.  Both launches evaluate three torsos per batch row between the same three barriers;
Munchausen DQN adds two expf / logf pairs per row in every thread and two more output stores.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import bench_ddqn as B  # noqa: E402
import deep_rl_amd as D  # noqa: E402
from deep_rl_amd import _native as N, _native_ddqn as KD, _native_md as K  # noqa: E402


def make(cls, n, slots, batch, total, seed):
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed)
    torch.manual_seed(seed)
    q = D.QNetwork(env); t = D.QNetwork(env); t.load_state_dict(q.state_dict())
    opt = D.Adam(q, lr=2.5e-4)
    eng = cls(env, q, t, opt, slots=slots, batch_size=batch, learning_starts=100, total_timesteps=total, max_episodes_logged=0)   # (bench_ddqn.py's arguments)
    eng.reset()
    return eng


def measure(cls, n, slots, args, total_iters):
    eng = make(cls, n, slots, args.batch, 10 * total_iters, args.seed)
    for _ in range(args.warmup):
        B.iteration(eng)
    r = B.windows(eng, args.windows, args.iters)
    r["per_launch_us"] = B.per_launch(eng, args.iters)
    r["finite"] = bool(torch.isfinite(eng.q.flat).all())
    r["loss"] = float(eng.loss.item())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x100001,4096x256")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "mdqn_bench.json"))
    args = ap.parse_args()
    res = {"bench": "mdqn", "device": torch.cuda.get_device_name(0), "mdqn_source_id": K.source_id(), "ddqn_source_id": KD.source_id(),
           "mirl_source_id": N.lib().mi_source_id().decode(), "batch": args.batch, "windows": args.windows, "iterations_per_window": args.iters,
           "warmup_iterations": args.warmup, "seed": args.seed, "alpha_tau_clip_lo": [0.9, 0.03, -1.0],
           "iteration": "10 env steps of every env (1 launch) + 1 update (2 launches)", "sync": "window edges only", "ddqn_same_run": {}, "gradient_launch_vs_ddqn": {}}
    total_iters = args.warmup + (args.windows + 1) * args.iters
    for shape in args.shapes.split(","):
        n, slots = [int(x) for x in shape.split("x")]
        key = "n%d_slots%d" % (n, slots)
        res[key] = measure(D.MunchausenDQNEngine, n, slots, args, total_iters)
        torch.cuda.empty_cache()
        res["ddqn_same_run"][key] = measure(D.DoubleDQNEngine, n, slots, args, total_iters)
        torch.cuda.empty_cache()
        res["gradient_launch_vs_ddqn"][key] = round(res[key]["per_launch_us"]["gradient_launch"]["median"] /
                                                    res["ddqn_same_run"][key]["per_launch_us"]["gradient_launch"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
