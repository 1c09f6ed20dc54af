#!/usr/bin/env python3
"""The learning yardstick of Augmented Random Search: the CPU restatement of include/mi_ars.h (tests/_ars_ref.py) with its OWN float64 draw, run at the script's
defaults (N = 8 directions, all of them selected, step size 0.02, noise 0.03, normaliser on) for 24 seeds and 40 iterations on the CPU oracle's CartPole.

Per seed it records the mean training return of the last 10 iterations and the mean greedy return of evaluate(100); then the mean, the (sample) standard deviation
and floor = mean - 3 sd of the former and the smallest of the latter.  tests/test_gpu_ars_script.py holds the device's six-seed mean to that floor and each seed's
greedy mean to that smallest value; tests/test_ars_ref_cpu.py re-runs one seed against the file.  The file holds results only.

    python tools/capture_ars_ref.py [--seeds 24] [--jobs 8]        -> tests/golden/ars_ref_learning.json
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
N_DIRECTIONS, N_TOP, ITERATIONS, LAST, EVAL_EPISODES = 8, 8, 40, 10, 100


def run_seed(seed):
    """-> (mean training return of the last LAST iterations, mean greedy return) of one seed at the script's defaults (training env ids from 0, as ARSEngine's)"""
    import _ars_ref as A
    from oracle import cpu_ref as R

    state, returns = A.chain(R, N_DIRECTIONS, N_TOP, ITERATIONS, seed=seed, base=0)
    greedy = A.evaluate(R, state, EVAL_EPISODES, seed=1, base=A.EVAL_BASE)
    return float(returns[-LAST:].astype("float64").mean()), float(sum(e["ret"] for e in greedy) / len(greedy))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ars_ref_learning.json"))
    args = ap.parse_args()
    seeds = list(range(1, args.seeds + 1))
    with multiprocessing.Pool(args.jobs) as pool:
        rows = pool.map(run_seed, seeds)
    train = [r[0] for r in rows]
    mean = sum(train) / len(train)
    sd = (sum((v - mean) ** 2 for v in train) / (len(train) - 1)) ** 0.5
    out = dict(n_directions=N_DIRECTIONS, n_top=N_TOP, step_size=0.02, noise=0.03, normalize=1, iterations=ITERATIONS, last=LAST, eval_episodes=EVAL_EPISODES,
               seeds=seeds, train_last_mean=train, greedy_mean=[r[1] for r in rows], mean=mean, sd=sd, floor=mean - 3.0 * sd, greedy_min=min(r[1] for r in rows))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("mean %.3f sd %.3f floor %.3f greedy_min %.3f -> %s" % (mean, sd, out["floor"], out["greedy_min"], args.out))


if __name__ == "__main__":
    main()
