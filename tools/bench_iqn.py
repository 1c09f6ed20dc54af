#!/usr/bin/env python3
"""IQN throughput on one MI355X: prints ONE JSON line and writes it to --out (default profiles/iqn_bench.json; "" writes nothing).

For each (envs, slots) of ``--shapes`` (default: the script's shape 1 env x 50,001 slots, and 4,096 envs x 256 slots) at batch 32: env-steps/s, updates/s and
microseconds per iteration of the script's loop — one iteration = 4 env steps of every env (one launch) + one update (two launches), the target sync every 125th
— as the median of ``--windows`` windows of ``--iters`` iterations after ``--warmup`` iterations, synchronised at the window edges only; the spread (min, max)
is reported beside the median, and the host's enqueue time per iteration (a loop whose enqueue time is all of its time is host-bound).  Exploration runs at
the script's final epsilon of 0.01 (learning_starts 0, a decay of one step), so all but one step in a hundred evaluate the networks.
``per_launch_us``: HIP-event times of the loop's three launches (acting chunk; gradient launch; slab sum + Adam — the last two split by an event that
mi_iqn_update records between its launches), median and spread over the iterations of one window.
``gradient_launch_matrix_floor_us``: the gradient launch's matrix work — per batch row (32 + 64 + 64 target / online forward rows + 64 recomputed + 2 x 64
backward rows) x 512 x 64 fused multiply-adds in the head — at the chip's f32 MFMA rate (157.3 TFLOP/s), the time below which no f32 version can go.
Read it against the reference's statements on one CPU core (``tools/capture_iqn_ref.py --time-only``) and ``tools/bench_c51.py`` from the same run.
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
from deep_rl_amd import _native as N, _native_iqn as K  # noqa: E402


def make(n, slots, batch, seed):
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed)
    torch.manual_seed(seed)
    nets = [(D.FeaturesExtractor(env), D.CosineEmbeddingNetwork(64, 64, device=dev), D.QuantileNetwork(2, 64, device=dev)) for _ in range(2)]
    p, t = D.pack(*nets[0]), D.pack(*nets[1])
    t.copy_(p)
    opt = D.Adam(p, lr=5e-5, eps=1e-2 / batch)
    eng = D.IQNEngine(env, p, t, opt, slots=slots, batch_size=batch, final_epsilon=0.01, epsilon_decay_steps=1, learning_starts=0, max_episodes_logged=0)
    eng.reset()
    return eng


def iteration(eng):
    eng.act(4); eng.train_step()
    if eng.global_step % 500 == 0:
        eng.sync_target()


def spread(xs, nd=1):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def windows(eng, n_windows, iters):
    us, enq = [], []
    for _ in range(n_windows):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(iters):
            iteration(eng)
        t1 = time.perf_counter()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        us.append(1e6 * dt / iters); enq.append(1e6 * (t1 - t0) / iters)
    med = statistics.median(us)
    return {"us_per_iteration": spread(us), "host_enqueue_us_per_iteration": spread(enq), "updates_per_s": round(1e6 / med, 1),
            "env_steps_per_s": round(4 * eng.N * 1e6 / med)}


def per_launch(eng, iters):
    """HIP-event time of each of the loop's three launches: the acting chunk, and the update's two, split by the event mi_iqn_update records between them."""
    names = ("act_4_steps", "gradient_launch", "slab_sum_adam")
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
    for row in ev:
        row[2].record()   # (a torch event gets its handle on its first record)
    for u in range(iters):
        a0, a1, mid, end = ev[u]
        a0.record(); eng.act(4); a1.record()
        eng.mid_event = mid.cuda_event
        eng.train_step(); end.record()   # gradient_launch counts from the acting chunk's end: nothing else is enqueued between them
    eng.mid_event = None
    torch.cuda.synchronize()
    pairs = ((0, 1), (1, 2), (2, 3))
    return {nm: spread([ev[u][i].elapsed_time(ev[u][j]) * 1e3 for u in range(iters)]) for nm, (i, j) in zip(names, pairs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x50001,4096x256")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "iqn_bench.json"))
    args = ap.parse_args()
    res = {"bench": "iqn", "device": torch.cuda.get_device_name(0), "iqn_source_id": K.source_id(), "mirl_source_id": N.lib().mi_source_id().decode(),
           "batch": args.batch, "windows": args.windows, "iterations_per_window": args.iters, "warmup_iterations": args.warmup, "seed": args.seed,
           "iteration": "4 env steps of every env (1 launch) + 1 update (2 launches)", "sync": "window edges only",
           "gradient_launch_matrix_floor_us": round(args.batch * (32 + 64 + 64 + 64 + 2 * 64) * 512 * 64 * 2 / 157.3e12 * 1e6, 2)}
    for shape in args.shapes.split(","):
        n, slots = [int(x) for x in shape.split("x")]
        eng = make(n, slots, args.batch, args.seed)
        for _ in range(args.warmup):
            iteration(eng)
        r = windows(eng, args.windows, args.iters)
        r["per_launch_us"] = per_launch(eng, args.iters)
        r["finite"] = bool(torch.isfinite(eng.q.flat).all())
        r["loss"] = float(eng.loss.item())
        res["n%d_slots%d" % (n, slots)] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
