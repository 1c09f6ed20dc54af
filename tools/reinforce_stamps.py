#!/usr/bin/env python3
"""How long is ONE step of pg_episode_kernel?  Reads the stamps of the -DPG_STAMPS diagnostic build of libmirl_pg.so: wave 0 of workgroup 0 stores the 100 MHz
wall clock at every 16th step of its episode (csrc/mi_reinforce.hip, PG_STAMP).  Prints one JSON line: ns per step at N = 1 (one wave on the chip: the bare
latency of the dependent chain) and at N = 4,096 (4 waves per SIMD share the issue slots).  Build the diagnostic library first:

    cd deep_rl_amd/csrc && hipcc $(FLAGS of the Makefile) -DPG_STAMPS -shared mi_reinforce.hip -o build_pg_stamps/libmirl_pg.so

and run with MIRL_PG_SO=deep_rl_amd/csrc/build_pg_stamps/libmirl_pg.so.  Teacher-forced with a balancing rule's actions are not needed: the stamps cover whatever
length env 0's episode has; with the seeded initial policy that is 1-3 stamp intervals, so the tool plays --episodes episodes and pools the intervals."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import deep_rl_amd as D  # noqa: E402
from deep_rl_amd import _native_pg as PG  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,4096")
    ap.add_argument("--episodes", type=int, default=40)
    args = ap.parse_args()
    L = PG.lib()
    if not hasattr(L, "mi_debug_pg_stamps"):
        raise SystemExit("%s is not a -DPG_STAMPS build (see the module docstring)" % PG.SO_PATH)
    out = {"tool": "reinforce_stamps", "so": os.path.basename(os.path.dirname(PG.SO_PATH)), "clock_mhz": 100}
    for n in [int(x) for x in args.envs.split(",")]:
        env = D.make("CartPole-v1", num_envs=n, device="cuda:0", seed=1)
        torch.manual_seed(1)
        agent = D.DropoutPolicy(env)
        eng = D.ReinforceEngine(env, agent, D.Adam(agent, lr=1e-2))
        per_step = []
        for _ in range(args.episodes):
            eng.rollout()
            torch.cuda.synchronize()
            k = int(eng.lengths[0]) - 1 >> 4       # stamps 0..k were written by this episode
            st = (C.c_ulonglong * 64)()
            assert L.mi_debug_pg_stamps(st) == 0
            per_step += [(st[i + 1] - st[i]) * 10.0 / 16 for i in range(k)]
        out["n%d" % n] = {"intervals": len(per_step), "ns_per_step_median": round(statistics.median(per_step), 1) if per_step else None,
                          "ns_per_step_min": round(min(per_step), 1) if per_step else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
