#!/usr/bin/env python3
"""The learning yardstick of Munchausen DQN on CartPole-v1 (TEST INFRASTRUCTURE ONLY; never runs on a GPU machine).

The reference has NO munchausen_dqn.py.  Torch itself stands in for it: ``mdqn_torch`` below is the algorithm of include/mi_mdqn.h written as a plain single-file
torch program in this project's own words — ``nn.Sequential``, autograd, ``optim.Adam``, one CPU thread, the env of oracle/gym_shim — with the loop, the seeding
order, the storage and the print line of the reference family's DQN script and the TD target replaced by the paper's: the target network's scaled, clipped
log-policy of the stored action is added to the reward, and the bootstrap is its soft value at the successor.  It is the counterpart of tools/capture_ddqn_ref.py.

Output:
  (default) [--seeds 24] [--jobs 8]   tests/golden/mdqn_learning_stats.npz: the last-tenth mean return of seeds 1 .. 24 and nothing else (a few hundred bytes);
                                      the seeds run as parallel single-thread processes
  --time-only                         the uninstrumented script on one CPU core: env steps per second (the baseline tools/bench_mdqn.py is read against)
"""
import argparse, multiprocessing as mp, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "gym_shim")
HP = dict(total_timesteps=100_000, learning_starts=10_000, start_e=1.0, end_e=0.05, exploration_fraction=0.5, train_frequency=10, batch_size=128, gamma=0.99,
          learning_rate=2.5e-4, target_network_frequency=500, alpha=0.9, tau=0.03, clip_lo=-1.0)


def mdqn_torch(seed=1, out=print, **over):
    """The stand-in script."""
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import gym, torch
    from torch import nn, optim
    hp = dict(HP, **over)
    T, B, gamma = hp["total_timesteps"], hp["batch_size"], hp["gamma"]
    alpha, tau, clip_lo = hp["alpha"], hp["tau"], hp["clip_lo"]
    slope = (hp["end_e"] - hp["start_e"]) / (hp["exploration_fraction"] * T)

    def make_net():
        return nn.Sequential(nn.Linear(4, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU(), nn.Linear(84, 2))

    env = gym.wrappers.RecordEpisodeStatistics(gym.make("CartPole-v1"))
    env.seed(seed); np.random.seed(seed); torch.manual_seed(seed); env.action_space.seed(seed)
    q_network = make_net()
    optimizer = optim.Adam(q_network.parameters(), lr=hp["learning_rate"])
    target_network = make_net()
    target_network.load_state_dict(q_network.state_dict())
    observations = torch.zeros((T + 1, 4)); actions = torch.zeros(T + 1, dtype=torch.long)
    rewards = torch.zeros(T + 1); terminated = torch.zeros(T + 1, dtype=torch.bool)
    observation = torch.tensor(env.reset())
    observations[0] = observation
    rows = torch.arange(B)
    for global_step in range(T):
        epsilon = max(slope * global_step + hp["start_e"], hp["end_e"])
        if global_step < hp["learning_starts"] or np.random.random() < epsilon:
            action = torch.tensor(env.action_space.sample())
        else:
            with torch.no_grad():
                action = torch.argmax(q_network(observation), -1)
        actions[global_step] = action
        obs_np, reward, done, info = env.step(action.numpy())
        if done:
            obs_np = env.reset()
        observation = torch.tensor(obs_np)
        g = global_step + 1
        observations[g] = observation; rewards[g] = reward
        terminated[g] = done and not info.get("TimeLimit.truncated", False)
        if "episode" in info:
            out(f"global_step={g}, episodic_return={info['episode']['r']:.2f}")
        if g >= hp["learning_starts"]:
            if g % hp["train_frequency"] == 0:
                batch_inds = np.random.randint(g, size=B)
                with torch.no_grad():
                    q_next = target_network(observations[batch_inds + 1])
                    pi_next = torch.softmax(q_next / tau, -1)
                    soft_value = (pi_next * (q_next - tau * torch.log_softmax(q_next / tau, -1))).sum(-1)   # sum_a pi (q - tau ln pi)
                    log_pi = torch.log_softmax(target_network(observations[batch_inds]) / tau, -1)[rows, actions[batch_inds]]
                    bonus = torch.clamp(tau * log_pi, clip_lo, 0.0)                                          # not masked: it belongs to (s, a)
                    target = rewards[batch_inds + 1] + alpha * bonus + gamma * soft_value * torch.logical_not(terminated[batch_inds + 1]).float()
                current = q_network(observations[batch_inds])[rows, actions[batch_inds]]
                loss = ((target - current) ** 2).mean()
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            if g % hp["target_network_frequency"] == 0:
                target_network.load_state_dict(q_network.state_dict())
    env.close()


def run_lines(seed, **kw):
    lines = []; t0 = time.time()
    mdqn_torch(seed, out=lines.append, **kw)
    wall = time.time() - t0
    steps = np.array([int(ln.split(",")[0].split("=")[1]) for ln in lines], np.int64)
    rets = np.array([float(ln.split("episodic_return=")[1]) for ln in lines], np.float64)
    return steps, rets, wall


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def _run_seed(seed):
    import torch
    torch.set_num_threads(1)
    steps, rets, wall = run_lines(seed)
    return seed, last_tenth(rets), len(rets), wall


def capture_learning(out_path, seeds, jobs):
    lt = {}
    with mp.get_context("spawn").Pool(jobs, maxtasksperchild=1) as pool:
        for seed, mean, n_ep, wall in pool.imap_unordered(_run_seed, list(range(1, seeds + 1))):
            lt[seed] = mean
            print("seed %3d: %4d episodes, last-tenth mean %7.2f (%.0f s)" % (seed, n_ep, mean, wall), flush=True)
    order = sorted(lt)
    assert order == list(range(1, seeds + 1))
    arr = np.array([lt[s] for s in order], np.float64)    # entry s - 1: seed s
    np.savez_compressed(out_path, mdqn_last_tenth_mean=arr)
    print("last-tenth means: mean %.2f, seed-to-seed sd %.2f -> %s (%d bytes)" % (arr.mean(), arr.std(ddof=1), out_path, os.path.getsize(out_path)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.time_only:
        import torch
        torch.set_num_threads(1)
        steps, rets, wall = run_lines(1)
        T = HP["total_timesteps"]
        print('{"torch_mdqn_cpu_1core": {"env_steps": %d, "episodes": %d, "wall_s": %.2f, "env_steps_per_s": %.0f}}' % (T, len(steps), wall, T / wall))
    else:
        capture_learning(args.out or os.path.join(GOLD, "mdqn_learning_stats.npz"), args.seeds, args.jobs)


if __name__ == "__main__":
    main()
