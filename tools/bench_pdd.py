#!/usr/bin/env python3
"""Prioritized dueling Double DQN throughput on one MI355X: prints ONE JSON line and writes it to --out (default profiles/pdd_bench.json; "" writes nothing).

The method of tools/bench_ddqn.py.  For each replay mode (prioritized, uniform) and each (envs, slots) of ``--shapes`` (default: the script's shape 1 env x 100,001
slots, and 4,096 envs x 256 slots) at batch 128: env-steps/s, updates/s and microseconds per iteration of the script's loop — one iteration = 10 env steps of every
env + one update, the target sync every 50th — as the median of ``--windows`` windows of ``--iters`` iterations after ``--warmup`` iterations, synchronised at the
window edges only; the spread (min, max) is reported beside the median, and the host's enqueue time per iteration (a loop whose enqueue time is all of its time is
host-bound).  Uniform: 3 launches per iteration (acting; gradient; slab sum + Adam).  Prioritized: 6 — libmirl's mark behind the acting launch, its sampler in front
of the update and its priority scatter behind it.  Exploration runs at the script's schedule stretched over the measured steps, so greedy and exploring steps are
both in the timed mix.
``per_launch_us``: HIP-event times over the iterations of one window, median and spread: ``act_10_steps`` (prioritized: the acting launch + the mark),
``gradient_launch`` (from the acting's end to the event mi_pdd_update records between its launches — prioritized: the sampler is in it) and ``slab_sum_adam``
(prioritized: + the scatter).
``same_run``: the JSON lines of ``tools/bench_ddqn.py --no-compare`` and of ``tools/bench_dqn.py --variant per`` at both shapes, each run as a fresh child process
directly behind this measurement — the figures this library is read against, taken on the same device in the same run (--no-compare leaves them out).
Read it also against the plain torch script on one CPU core (``tools/capture_pdd_ref.py --time-only``).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import deep_rl_amd as D  # noqa: E402
from deep_rl_amd import _native as N, _native_pdd as K  # noqa: E402


def make(n, slots, batch, total, seed, prioritized):
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed)
    torch.manual_seed(seed)
    q = D.DuelingQNetwork(env); t = D.DuelingQNetwork(env); t.load_state_dict(q.state_dict())
    opt = D.Adam(q, lr=2.5e-4)
    eng = D.PDDDQNEngine(env, q, t, opt, slots=slots, batch_size=batch, learning_starts=100, total_timesteps=total, max_episodes_logged=0,   # (bench_dqn.py's learning_starts)
                         prioritized=prioritized)
    eng.reset()
    return eng


def iteration(eng):
    eng.act(10); eng.train_step()
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
            "env_steps_per_s": round(10 * eng.N * 1e6 / med)}


def per_launch(eng, iters):
    """HIP-event times of the loop's parts: the acting chunk (+ mark), and the update's two halves, split by the event mi_pdd_update records between its launches."""
    names = ("act_10_steps", "gradient_launch", "slab_sum_adam")
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
    for row in ev:
        row[2].record()   # (a torch event gets its handle on its first record)
    for u in range(iters):
        a0, a1, mid, end = ev[u]
        a0.record(); eng.act(10); a1.record()
        eng.mid_event = mid.cuda_event
        eng.train_step(); end.record()
    eng.mid_event = None
    torch.cuda.synchronize()
    pairs = ((0, 1), (1, 2), (2, 3))
    return {nm: spread([ev[u][i].elapsed_time(ev[u][j]) * 1e3 for u in range(iters)]) for nm, (i, j) in zip(names, pairs)}


def child(argv):
    """the JSON line of another bench tool, run as a fresh process"""
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, os.path.join(here, argv[0])] + argv[1:], capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("%s failed: %s" % (argv[0], p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x100001,4096x256")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-compare", action="store_true", help="leave out the Double DQN and PER runs")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pdd_bench.json"))
    args = ap.parse_args()
    res = {"bench": "pdd", "device": torch.cuda.get_device_name(0), "pdd_source_id": K.source_id(), "mirl_source_id": N.lib().mi_source_id().decode(),
           "batch": args.batch, "windows": args.windows, "iterations_per_window": args.iters, "warmup_iterations": args.warmup, "seed": args.seed,
           "iteration": {"uniform": "10 env steps of every env (1 launch) + 1 update (2 launches)",
                         "prioritized": "10 env steps of every env (1 launch) + mark (1) + sampler (1) + 1 update (2) + priority scatter (1)"},
           "sync": "window edges only"}
    total_iters = args.warmup + (args.windows + 1) * args.iters
    eng = None
    for mode in ("prioritized", "uniform"):
        res[mode] = {}
        for shape in args.shapes.split(","):
            n, slots = [int(x) for x in shape.split("x")]
            eng = make(n, slots, args.batch, 10 * total_iters, args.seed, mode == "prioritized")
            for _ in range(args.warmup):
                iteration(eng)
            r = windows(eng, args.windows, args.iters)
            r["per_launch_us"] = per_launch(eng, args.iters)
            r["finite"] = bool(torch.isfinite(eng.q.flat).all())
            r["loss"] = float(eng.loss.item())
            res[mode]["n%d_slots%d" % (n, slots)] = r
    if not args.no_compare:
        del eng
        torch.cuda.empty_cache()
        res["same_run"] = {"ddqn": child(["bench_ddqn.py", "--no-compare", "--out", ""]),
                           "per": {"n1_slots100001": child(["bench_dqn.py", "--variant", "per", "--envs", "1", "--slots", "100001"]),
                                   "n4096_slots256": child(["bench_dqn.py", "--variant", "per"])}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
