#!/usr/bin/env python3
"""The seeded byte-for-byte sequence of a ring-replay library (C51, IQN, QR-DQN, Double DQN, Munchausen DQN, prioritized dueling Double DQN and its n-step and noisy
forms): what a refactor of mi_ring.h / mi_torso.h / mi_dueling.h / mi_qhead.h / mi_*.hip must leave unchanged.

    tools/ring_ab_hashes.py --algo c51|iqn|qrdqn|ddqn|mdqn|pdd|nstep|noisy --envs N --slots S --batch B --out FILE   [--prioritized 0|1] [--n-step N] [--noisy 0|1]

One process, one library set (the ones ``MIRL_C51_SO`` / ``MIRL_IQN_SO`` / ``MIRL_QR_SO`` / ``MIRL_DDQN_SO`` / ``MIRL_MDQN_SO`` / ``MIRL_PDD_SO`` / ``MIRL_NS_SO`` /
``MIRL_NZ_SO`` name, else the built ones; the n-step and the noisy engine act through libmirl_pdd.so, the Munchausen engine through libmirl_ddqn.so), no retry.  It runs
  1 reset   2 act(64)   3 act(7) with forced actions and resets (IQN: forced taus and taus_out too)   4 six train_step()s with deep_rl_amd.Adam
  5 sample(indices) + target() + grad() + optimizer.step   6 sync_target   7 act(64) at the epsilon floor
and after every stage writes the sha256 of the raw bytes of every tensor: the ring, the env's fp64 state and TimeLimit counters, the carried observation,
episode_stats, the drained episodes, batch_inds, next_actions, the target and current tensors, the taus, grads, loss, both parameter vectors and Adam's moments;
for pdd / nstep / noisy also td_abs, the n-step horizon and, prioritized, weights, priorities and max_priority; for mdqn also bonus and soft_value (alpha 0.9, tau 0.03,
clip -1).  Stage 3 is forced for every algorithm but nstep and mdqn, which have no acting kernel of their own.  ``--noisy 0`` runs the mean network under the epsilon schedule, ``--noisy 1`` the noise with epsilon 0.
FILE holds nothing but the stages (no library id, no time), so two runs are compared with ``cmp``; the library's id goes to stdout.
The schedule puts stage 2 on the decaying epsilon (Double DQN and IQN: its first 16 steps before learning_starts) and stage 7 on the floor.
"""
import argparse
import hashlib
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import deep_rl_amd as D  # noqa: E402

DECAY_STEPS, LEARNING_STARTS = 70, 16   # stages 2 and 3 take steps 0 .. 70, stage 7 steps 71 .. 134


def make(algo, n, slots, batch, seed, prioritized=True, n_step=3, noisy=True):
    """-> (engine, the names of the algorithm's own tensors)"""
    dev = torch.device("cuda", 0)
    env = D.make("CartPole-v1", num_envs=n, device=dev, seed=seed)
    torch.manual_seed(seed)
    log = 64 * n   # an env ends at most one episode per step: no call overflows the log, so which episodes it holds does not depend on the order of the workgroups
    if algo == "iqn":
        from deep_rl_amd import _native_iqn as K
        nets = [(D.FeaturesExtractor(env), D.CosineEmbeddingNetwork(64, 64, device=dev), D.QuantileNetwork(2, 64, device=dev)) for _ in range(2)]
        p, t = D.pack(*nets[0]), D.pack(*nets[1])
        t.copy_(p)
        eng = D.IQNEngine(env, p, t, D.Adam(p, lr=5e-5, eps=1e-2 / batch), slots=slots, batch_size=batch, final_epsilon=0.01, epsilon_decay_steps=DECAY_STEPS,
                          learning_starts=LEARNING_STARTS, max_episodes_logged=log)
        return eng, K, ("taus", "current_action_quantiles", "target_action_quantiles")
    if algo in ("pdd", "nstep", "noisy"):   # the dueling networks tools/bench_pdd.py, bench_nstep.py and bench_noisy.py build
        net, engine, K, kw = {
            "pdd": (D.DuelingQNetwork, D.PDDDQNEngine, "_native_pdd", {}),
            "nstep": (D.DuelingQNetwork, D.NStepDQNEngine, "_native_ns", {"n_step": n_step}),
            "noisy": (D.NoisyDuelingQNetwork, D.NoisyDQNEngine, "_native_nz", dict(n_step=n_step, noisy=noisy, **({} if noisy else {"start_e": 1.0, "end_e": 0.05}))),
        }[algo]
        q = net(env); t = net(env); t.load_state_dict(q.state_dict())
        eng = engine(env, q, t, D.Adam(q, lr=2.5e-4), slots=slots, batch_size=batch, learning_starts=LEARNING_STARTS, total_timesteps=2 * DECAY_STEPS,
                     exploration_fraction=0.5, max_episodes_logged=log, prioritized=prioritized, **kw)
        own = ("current", "target_values", "td_abs") + (("horizon",) if hasattr(eng, "horizon") else ()) + (("weights", "priorities", "max_priority") if prioritized else ())
        return eng, getattr(__import__("deep_rl_amd." + K), K), own
    net, engine, K, own, kw = {
        "c51": (D.C51QNetwork, D.C51Engine, "_native_c51", ("probs", "target_probs"), {}),
        "qrdqn": (D.QRQNetwork, D.QRDQNEngine, "_native_qr", ("current", "target_quantiles"), {}),
        "ddqn": (D.QNetwork, D.DoubleDQNEngine, "_native_ddqn", ("current", "target_values"), {"learning_starts": LEARNING_STARTS}),
        "mdqn": (D.QNetwork, D.MunchausenDQNEngine, "_native_md", ("current", "target_values", "bonus", "soft_value"),
                 {"learning_starts": LEARNING_STARTS, "alpha": 0.9, "tau": 0.03, "clip_lo": -1.0}),
    }[algo]
    q = net(env); t = net(env); t.load_state_dict(q.state_dict())
    eng = engine(env, q, t, D.Adam(q, lr=2.5e-4, eps=0.01 / batch), slots=slots, batch_size=batch, total_timesteps=2 * DECAY_STEPS, exploration_fraction=0.5,
                 max_episodes_logged=log, **kw)
    return eng, getattr(__import__("deep_rl_amd." + K), K), own


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def snapshot(eng, own, extra):
    state, elapsed = eng.env.get_state()
    count, eps = eng.drain_episodes()
    drained = b"".join(struct.pack("<iifi", e, s, r, ln) for (e, s, r, ln) in eps)
    h = {"env_state": sha(state), "env_elapsed": sha(elapsed), "episodes_drained": hashlib.sha256(struct.pack("<i", count) + drained).hexdigest(),
         "params": sha(eng.q.flat), "target_params": sha(eng.target_network.flat), "exp_avg": sha(eng.optimizer.exp_avg), "exp_avg_sq": sha(eng.optimizer.exp_avg_sq)}
    for name in ("observations", "actions", "rewards", "terminated", "observation", "episode_stats", "batch_inds", "next_actions", "grads", "loss") + tuple(own):
        h[name] = sha(getattr(eng, name))
    for name, t in extra.items():
        h[name] = sha(t)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", required=True, choices=("c51", "iqn", "qrdqn", "ddqn", "mdqn", "pdd", "nstep", "noisy"))
    ap.add_argument("--envs", type=int, required=True)
    ap.add_argument("--slots", type=int, required=True)
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prioritized", type=int, choices=(0, 1), default=1, help="pdd / nstep / noisy: prioritized (1) or uniform (0) replay")
    ap.add_argument("--n-step", type=int, default=3, help="nstep / noisy")
    ap.add_argument("--noisy", type=int, choices=(0, 1), default=1, help="noisy")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    eng, K, own = make(args.algo, args.envs, args.slots, args.batch, args.seed, bool(args.prioritized), args.n_step, bool(args.noisy))
    print("library", K.SO_PATH, K.source_id(), flush=True)
    n, iqn = args.envs, args.algo == "iqn"
    gen = torch.Generator().manual_seed(args.seed)
    stages, extra = [], {}

    def stage(name):
        torch.cuda.synchronize()
        stages.append({"stage": name, "sha256": snapshot(eng, own, extra)})

    eng.reset(); stage("1 reset")
    eng.act(64); stage("2 act(64)")
    forced = {"forced_actions": torch.randint(0, 2, (7, n), generator=gen, dtype=torch.int64),
              "forced_resets": (torch.rand((7, n, 4), generator=gen, dtype=torch.float64) - 0.5) * 0.1}
    if iqn:
        forced["forced_taus"] = torch.rand((7, n, K.N_QUANT), generator=gen, dtype=torch.float32)
        forced["taus_out"] = extra["taus_out"] = torch.zeros((7, n, K.N_QUANT), dtype=torch.float32, device=eng.device)
    if args.algo in ("nstep", "mdqn"):   # their acting is libmirl_pdd.so's / libmirl_ddqn.so's: --algo pdd / ddqn covers the forced launch
        forced = {}
    eng.act(7, **forced); stage("3 act(7) forced")
    for _ in range(6):
        eng.train_step()
    stage("4 six train_step()s")
    eng.sample(torch.randint(0, eng._upper(), (args.batch,), generator=gen, dtype=torch.int64))
    eng.target(); eng.grad(); eng.optimizer.step(eng.grads); stage("5 sample(indices) + target() + grad() + optimizer.step")
    eng.sync_target(); stage("6 sync_target")
    eng.act(64); stage("7 act(64) at the epsilon floor")
    with open(args.out, "w") as f:
        json.dump({"algo": args.algo, "envs": n, "slots": args.slots, "batch": args.batch, "seed": args.seed, "stages": stages}, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "stages", len(stages), "tensors per stage", len(stages[0]["sha256"]))


if __name__ == "__main__":
    main()
