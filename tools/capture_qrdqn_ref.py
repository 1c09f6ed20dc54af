#!/usr/bin/env python3
"""Golden vectors of QR-DQN on CartPole-v1 (TEST INFRASTRUCTURE ONLY; never runs on a GPU machine).

The reference has NO qrdqn.py.  Torch itself stands in for it: ``qrdqn_torch`` below is the algorithm of include/mi_qr.h written as a plain single-file torch
program in this project's own words — autograd, ``optim.Adam``, one CPU thread, the env of oracle/gym_shim — with the loop, the seeding order, the storage and the
print line of the reference family's replay scripts (its c51.py) and the head and loss replaced: Linear(84, 2 * 64) -> Unflatten(2, 64), fixed fractions
tau_i = (2 i + 1) / 128, the paper's quantile-Huber loss with kappa = 1 (0.5 u^2 inside, |u| - 0.5 outside), greedy actions from the mean of the quantiles.

Output, arrays of dtype kind f / i / u only, every file below 1 MiB (which is why the 50,000-step run is spread over three files):
  tests/golden/qrdqn_ref_trace.npz        seed 1: initial parameters, all 50,000 actions, terminated flags, reset states, the greedy / random split, all 4,001
                                          losses, the printed episode lines, the fractions
  tests/golden/qrdqn_ref_trace_obs.npz    the 50,000 f32 observations the env returned
  tests/golden/qrdqn_ref_trace_inds.npz   all 4,001 batch_inds as u16 (an index is < 50,000)
  tests/golden/qrdqn_ref_ckpt<k>.npz      updates 0, 1 (around the target sync at global_step 10,000), 50, 51 (around the one at 10,500), 2,000 and 4,000: parameters,
                                          target parameters, Adam moments before, the batch, current, target, next_actions, loss, autograd gradient, parameters after
  --learning [--seeds 32] [--jobs 8]      tests/golden/qrdqn_learning_stats.npz: episodic returns of seeds 1..32 with offsets and last-tenth means
  --time-only                             the uninstrumented script on one CPU core: env steps per second (the baseline tools/bench_qrdqn.py is read against)
"""
import argparse, multiprocessing as mp, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "gym_shim")
CHECKPOINTS = (0, 1, 50, 51, 2000, 4000)   # update k runs at global_step 10,000 + 10 k; the target syncs at multiples of 500 BEHIND that step's update
HP = dict(total_timesteps=50_000, learning_starts=10_000, start_e=1.0, end_e=0.05, exploration_fraction=0.5, train_frequency=10, batch_size=128, gamma=0.99,
          learning_rate=2.5e-4, target_network_frequency=500, n_quantiles=64, kappa=1.0)


def qrdqn_torch(seed=1, on_update=None, on_act=None, out=print, **over):
    """The stand-in script.  on_update(k, locals) is called before and after optimizer.step(); on_act(global_step, greedy) per env step."""
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import gym, torch
    from torch import nn, optim
    hp = dict(HP, **over)
    T, B, NQ, kappa, gamma = hp["total_timesteps"], hp["batch_size"], hp["n_quantiles"], hp["kappa"], hp["gamma"]
    slope = (hp["end_e"] - hp["start_e"]) / (hp["exploration_fraction"] * T)
    taus = (2 * torch.arange(NQ, dtype=torch.float32) + 1) / (2 * NQ)

    def make_net():
        return nn.Sequential(nn.Linear(4, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU(), nn.Linear(84, 2 * NQ), nn.Unflatten(-1, (2, NQ)))

    env = gym.wrappers.RecordEpisodeStatistics(gym.make("CartPole-v1"))
    env.seed(seed); np.random.seed(seed); torch.manual_seed(seed); env.action_space.seed(seed)
    q_network = make_net()
    optimizer = optim.Adam(q_network.parameters(), lr=hp["learning_rate"], eps=0.01 / B)
    target_network = make_net()
    target_network.load_state_dict(q_network.state_dict())
    observations = torch.zeros((T + 1, 4)); actions = torch.zeros(T + 1, dtype=torch.long)
    rewards = torch.zeros(T + 1); terminated = torch.zeros(T + 1, dtype=torch.bool)
    observation = torch.tensor(env.reset())
    observations[0] = observation
    k = 0
    for global_step in range(T):
        epsilon = max(slope * global_step + hp["start_e"], hp["end_e"])
        greedy = not (np.random.random() < epsilon)
        if greedy:
            with torch.no_grad():
                action = torch.argmax(q_network(observation).mean(dim=-1), -1)
        else:
            action = torch.tensor(env.action_space.sample())
        if on_act:
            on_act(global_step, greedy)
        actions[global_step] = action
        obs_np, reward, done, info = env.step(action.numpy())
        if done:
            obs_np = env.reset()
        observation = torch.tensor(obs_np)
        g = global_step + 1
        observations[g] = observation; rewards[g] = reward
        terminated[g] = done and not info.get("TimeLimit.truncated", False)
        if "episode" in info:
            out(f"global_step={g}, episodic_return={info['episode']['r']}")
        if g >= hp["learning_starts"]:
            if g % hp["train_frequency"] == 0:
                batch_inds = np.random.randint(g, size=B)
                b_terminated = terminated[batch_inds + 1]
                with torch.no_grad():
                    nq = target_network(observations[batch_inds + 1])
                    next_actions = torch.argmax(nq.mean(dim=-1), -1)
                    lg = gamma * torch.logical_not(b_terminated).float()
                    target = rewards[batch_inds + 1].unsqueeze(1) + lg.unsqueeze(1) * nq[torch.arange(B), next_actions]
                current = q_network(observations[batch_inds])[torch.arange(B), actions[batch_inds]]
                u = target.unsqueeze(1) - current.unsqueeze(2)                       # [B][i][j]
                au = u.abs()
                huber = torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))
                w = (taus.view(1, NQ, 1) - (u.detach() < 0).float()).abs()
                loss = (w * huber).sum(dim=(1, 2)).mean() / NQ
                optimizer.zero_grad()
                loss.backward()
                if on_update:
                    on_update(k, "before", locals())
                optimizer.step()
                if on_update:
                    on_update(k, "after", locals())
                k += 1
            if g % hp["target_network_frequency"] == 0:
                target_network.load_state_dict(q_network.state_dict())
    env.close()


def flat(params, grad=False):
    import torch
    with torch.no_grad():
        return torch.cat([(p.grad if grad else p).detach().reshape(-1) for p in params]).numpy().copy()


def run_lines(seed, **kw):
    lines = []; t0 = time.time()
    qrdqn_torch(seed, out=lines.append, **kw)
    wall = time.time() - t0
    steps = np.array([int(ln.split(",")[0].split("=")[1]) for ln in lines], np.int64)
    rets = np.array([float(ln.split("episodic_return=")[1]) for ln in lines], np.float64)
    return steps, rets, wall


def capture_trace(out_dir):
    sys.path.insert(0, SHIM)
    import gym, torch
    torch.set_num_threads(1)
    log = {"reset": [], "reset_at": [], "action": [], "obs": [], "terminated": []}

    def sink(event, p):
        if event == "reset":
            log["reset"].append(p["state"]); log["reset_at"].append(len(log["action"]))
        else:
            log["action"].append(p["action"]); log["obs"].append(p["obs"]); log["terminated"].append(p["terminated"])

    gym.register_trace_sink(sink)
    greedy = np.zeros(HP["total_timesteps"], np.uint8)
    rec = {"init": None, "inds": [], "loss": [], "ckpt": {}}

    def on_act(g, is_greedy):
        greedy[g] = 1 if is_greedy else 0

    def on_update(k, when, L):
        params = list(L["q_network"].parameters())
        if when == "before":
            assert L["g"] == 10_000 + 10 * k and k == len(rec["loss"])
            rec["inds"].append(np.asarray(L["batch_inds"]).copy()); rec["loss"].append(float(L["loss"].detach()))
            if k in CHECKPOINTS:
                st = L["optimizer"].state
                mom = [(st[p]["exp_avg"], st[p]["exp_avg_sq"]) if p in st and "exp_avg" in st[p] else (torch.zeros_like(p), torch.zeros_like(p)) for p in params]
                rec["ckpt"][k] = {
                    "update": np.array([k], np.int32), "global_step": np.array([L["g"]], np.int32),
                    "batch_inds": np.asarray(L["batch_inds"]).astype(np.int32), "loss": np.array([float(L["loss"].detach())], np.float64),
                    "params_before": flat(params), "target_params": flat(list(L["target_network"].parameters())),
                    "exp_avg_before": torch.cat([m.reshape(-1) for m, _ in mom]).numpy().copy(),
                    "exp_avg_sq_before": torch.cat([v.reshape(-1) for _, v in mom]).numpy().copy(),
                    "target": L["target"].numpy().copy(), "next_actions": L["next_actions"].numpy().astype(np.int32),
                    "current": L["current"].detach().numpy().copy(), "grads": flat(params, grad=True),
                    "batch_terminated": L["b_terminated"].numpy().astype(np.uint8),
                }
        elif k in CHECKPOINTS:
            rec["ckpt"][k]["params_after"] = flat(params)

    orig_init = torch.optim.Adam.__init__

    def p_init(self, params, *a, **kw):
        params = list(params); rec["init"] = flat(params)
        return orig_init(self, params, *a, **kw)

    torch.optim.Adam.__init__ = p_init
    try:
        steps, rets, wall = run_lines(1, on_update=on_update, on_act=on_act)
    finally:
        torch.optim.Adam.__init__ = orig_init
    T = len(log["action"])
    assert T == 50_000 and len(rec["loss"]) == 4001 and sorted(rec["ckpt"]) == sorted(CHECKPOINTS)
    assert any(c["batch_terminated"].any() for c in rec["ckpt"].values()), "no checkpoint batch holds a terminated row"
    inds = np.stack(rec["inds"])
    assert inds.min() >= 0 and inds.max() < 65536
    files = {
        "qrdqn_ref_trace.npz": {
            "hparams": np.array([0.99, 2.5e-4, 0.01 / 128, 1, 0.05, 0.5, 50_000, 10_000, 10, 128, 500, 1, 64, 1.0], np.float64),   # gamma, lr, Adam eps, start_e,
            # end_e, exploration_fraction, total_timesteps, learning_starts, train_frequency, batch_size, target_network_frequency, seed, n_quantiles, kappa
            "init_params": rec["init"].astype(np.float32),
            "taus": ((2 * np.arange(64, dtype=np.float32) + 1) / np.float32(128)).astype(np.float32),
            "reset_states": np.array(log["reset"], np.float64), "reset_at": np.array(log["reset_at"], np.int32),   # reset r happened after reset_at[r] steps
            "actions": np.array(log["action"], np.int8), "terminated": np.array(log["terminated"], np.uint8), "greedy": greedy,
            "loss": np.array(rec["loss"], np.float64), "checkpoints": np.array(CHECKPOINTS, np.int32),
            "episode_global_step": steps.astype(np.int32), "episode_return": rets.astype(np.float32), "ref_wall_seconds": np.array([wall]),
        },
        "qrdqn_ref_trace_obs.npz": {"obs": np.array(log["obs"], np.float32)},
        "qrdqn_ref_trace_inds.npz": {"batch_inds": inds.astype(np.uint16)},
    }
    for k, c in rec["ckpt"].items():
        files["qrdqn_ref_ckpt%d.npz" % k] = {n: (v.astype(np.float32) if v.dtype.kind == "f" and n != "loss" else v) for n, v in c.items()}
    sizes = []
    for name, arrs in files.items():
        assert all(v.dtype.kind in "fiu" for v in arrs.values())
        p = os.path.join(out_dir, name)
        np.savez_compressed(p, **arrs)
        sizes.append(os.path.getsize(p))
    assert max(sizes) < (1 << 20), sizes
    print("torch QR-DQN: %d env steps, %d episodes, %d updates (%d greedy steps), final loss %.4f, %.1f s -> %s: %s KB" % (
        T, len(steps), len(rec["loss"]), int(greedy.sum()), rec["loss"][-1], wall, out_dir, ", ".join("%.0f" % (s / 1024) for s in sizes)))


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def _run_seed(seed):
    import torch
    torch.set_num_threads(1)
    steps, rets, wall = run_lines(seed)
    return seed, steps, rets, wall


def capture_learning(out_path, seeds, jobs):
    by_seed = {}
    with mp.get_context("spawn").Pool(jobs, maxtasksperchild=1) as pool:
        for seed, steps, rets, wall in pool.imap_unordered(_run_seed, list(range(1, seeds + 1))):
            by_seed[seed] = (steps, rets)
            print("seed %3d: %4d episodes, last-tenth mean %7.2f (%.0f s)" % (seed, len(rets), last_tenth(rets), wall), flush=True)
    trace = os.path.join(GOLD, "qrdqn_ref_trace.npz")
    if os.path.exists(trace):   # seed 1 must be the run the trace fixture holds
        g = np.load(trace)
        assert np.array_equal(g["episode_global_step"], by_seed[1][0]) and np.allclose(g["episode_return"], by_seed[1][1])
    order = sorted(by_seed)
    out = {
        "qrdqn_seeds": np.array(order, np.int32),
        "qrdqn_offsets": np.cumsum([0] + [len(by_seed[s][1]) for s in order]).astype(np.int64),
        "qrdqn_episode_global_step": np.concatenate([by_seed[s][0] for s in order]).astype(np.int32),
        "qrdqn_episode_return": np.concatenate([by_seed[s][1] for s in order]).astype(np.float32),
        "qrdqn_last_tenth_mean": np.array([last_tenth(by_seed[s][1]) for s in order], np.float64),
    }
    np.savez_compressed(out_path, **out)
    lt = out["qrdqn_last_tenth_mean"]
    print("last-tenth means: mean %.2f, seed-to-seed sd %.2f -> %s (%.0f KB)" % (lt.mean(), lt.std(ddof=1), out_path, os.path.getsize(out_path) / 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.learning:
        return capture_learning(args.out or os.path.join(GOLD, "qrdqn_learning_stats.npz"), args.seeds, args.jobs)
    if args.time_only:
        import torch
        torch.set_num_threads(1)
        steps, rets, wall = run_lines(1)
        print('{"torch_qrdqn_cpu_1core": {"env_steps": %d, "episodes": %d, "wall_s": %.2f, "env_steps_per_s": %.0f}}' % (50_000, len(steps), wall, 50_000 / wall))
    else:
        capture_trace(args.out or GOLD)


if __name__ == "__main__":
    main()
