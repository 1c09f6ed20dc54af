#!/usr/bin/env python3
"""Rainbow throughput on one MI355X: prints ONE JSON line and writes it to --out (default profiles/rainbow_bench.json; "" writes nothing).

The method of tools/bench_noisy.py at the same two shapes (1 env x 100,001 slots, 4,096 envs x 256 slots), batch 128, n_step 3, the support 0 .. 100 and both replay
modes, in two variants: ``noisy`` (every greedy step and every update draws its heads; epsilon 0) and ``noisy_off`` (noisy = 0, epsilon 0: the same all-greedy
acting without the draw — the difference is what the per-step draw of 321 factors and the forming of 153 effective rows cost).  Per variant: env-steps/s,
updates/s and microseconds per iteration of the script's loop — one iteration = 10 env steps of every env + one update, the target sync every 50th — as the median
of ``--windows`` windows of ``--iters`` iterations after ``--warmup`` iterations, synchronised at the window edges only, with the spread and the host's enqueue time
beside it.
``per_launch_us``: HIP-event times over the iterations of one window, median and spread: ``act_10_steps``, ``gradient_launch`` (from the acting's end to the event
mi_rb_update records between its launches — prioritized: the sampler is in it; the three passes are in it) and ``slab_sum_adam`` (36,774 elements; prioritized: +
the scatter).
``same_run``: the JSON lines of ``tools/bench_noisy.py --no-compare`` and ``tools/bench_c51.py`` run as fresh child processes directly behind this measurement on
the same device (--no-compare leaves them out); ``vs_noisy_and_c51`` puts the medians side by side.
Read it also against the plain torch script on one CPU core (``tools/capture_rainbow_ref.py --time-only``).
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
from deep_rl_amd import _native as N, _native_rb as K  # noqa: E402


VARIANTS = {"noisy": dict(noisy=True), "noisy_off": dict(noisy=False)}


def make(n, slots, batch, total, seed, prioritized, variant):
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed)
    torch.manual_seed(seed)
    q = D.RainbowQNetwork(env); t = D.RainbowQNetwork(env); t.load_state_dict(q.state_dict())
    opt = D.Adam(q, lr=2.5e-4)
    eng = D.RainbowEngine(env, q, t, opt, slots=slots, batch_size=batch, learning_starts=100, total_timesteps=total, max_episodes_logged=0,   # (bench_dqn.py's learning_starts)
                          prioritized=prioritized, n_step=3, v_min=0.0, v_max=100.0, **VARIANTS[variant])
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
    """HIP-event times of the loop's parts: the acting chunk (+ mark), and the update's two halves, split by the event mi_rb_update records between its launches."""
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
    ap.add_argument("--no-compare", action="store_true", help="leave out the noisy / C51 runs")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rainbow_bench.json"))
    args = ap.parse_args()
    res = {"bench": "rainbow", "support": [0.0, 100.0], "n_atoms": 51, "device": torch.cuda.get_device_name(0), "rainbow_source_id": K.source_id(), "n_step": 3, "mirl_source_id": N.lib().mi_source_id().decode(),
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
            for variant in VARIANTS:
                eng = make(n, slots, args.batch, 10 * total_iters, args.seed, mode == "prioritized", variant)
                for _ in range(args.warmup):
                    iteration(eng)
                r = windows(eng, args.windows, args.iters)
                r["per_launch_us"] = per_launch(eng, args.iters)
                r["finite"] = bool(torch.isfinite(eng.q.flat).all())
                r["loss"] = float(eng.loss.item())
                r["mean_horizon"] = round(float(eng.horizon.float().mean().item()), 2)
                res[mode].setdefault("n%d_slots%d" % (n, slots), {})[variant] = r
    if not args.no_compare:
        del eng
        torch.cuda.empty_cache()
        common = ["--out", "", "--batch", str(args.batch), "--windows", str(args.windows), "--iters", str(args.iters), "--warmup", str(args.warmup), "--seed", str(args.seed)]
        same = res["same_run"] = {"noisy": child(["bench_noisy.py", "--no-compare", "--shapes", args.shapes] + common),
                                  "c51": child(["bench_c51.py", "--shapes", args.shapes] + common)}   # (C51: uniform replay, one-step, 101 atoms, 27,934 parameters)
        med = lambda r, part: r["per_launch_us"][part]["median"]   # noqa: E731
        parts = ("act_10_steps", "gradient_launch", "slab_sum_adam")
        res["vs_noisy_and_c51"] = {mode: {shape: {part: dict({"noisy_lib_noisy": med(same["noisy"][mode][shape]["noisy"], part),
                                                              "noisy_lib_off": med(same["noisy"][mode][shape]["noisy_off"], part)},
                                                             **({"c51": med(same["c51"][shape], part)} if mode == "uniform" and shape in same["c51"] else {}),
                                                             **{"rainbow_" + k: med(v, part) for k, v in by.items()})
                                                  for part in parts}
                                          for shape, by in res[mode].items()} for mode in ("prioritized", "uniform")}
        res["draw_cost_us_per_10_steps"] = {mode: {shape: round(med(by["noisy"], "act_10_steps") - med(by["noisy_off"], "act_10_steps"), 1) for shape, by in res[mode].items()}
                                            for mode in ("prioritized", "uniform")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
