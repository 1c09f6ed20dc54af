#!/usr/bin/env python3
"""The learning yardstick of Rainbow on CartPole-v1 (TEST INFRASTRUCTURE ONLY; never runs on a GPU machine).

The reference has NO Rainbow script.  Torch itself stands in for it: ``rainbow_torch`` below is tools/capture_noisy_ref.py's plain single-file torch program — noisy
value and advantage streams on torch's own generator, the double rule, prioritized replay, the n-step return as a masked loop over whole batches, autograd,
``optim.Adam``, one CPU thread, the env of oracle/gym_shim — with the algorithm of include/mi_rainbow.h in textbook form: the streams produce 51 atoms each on the
support [0, 100], combined by the dueling rule per atom and normalised by a softmax per action; the target is the categorical projection of the target network's
distribution of the online network's greedy action under R + gamma^m z (0 behind a terminal step); the loss is the importance-weighted cross-entropy with the 1e-8
inside the log; a row's unweighted cross-entropy is its new priority.  Nothing of the kernels' keyed draw is restated here, so the comparison with the library is
statistical, never draw for draw.

Output:
  (default) [--seeds 24] [--jobs 8]   tests/golden/rainbow_learning_stats.npz: the last-tenth mean return of seeds 1 .. 24 and nothing else (a few hundred bytes);
                                      the seeds run as parallel single-thread processes
  --time-only                         the uninstrumented script on one CPU core: env steps per second (the baseline tools/bench_rainbow.py is read against)
"""
import argparse, multiprocessing as mp, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "gym_shim")
HP = dict(total_timesteps=100_000, learning_starts=10_000, start_e=0.0, end_e=0.0, exploration_fraction=0.5, train_frequency=10, batch_size=128, gamma=0.99,
          learning_rate=2.5e-4, target_network_frequency=500, alpha=0.6, beta_0=0.4, n_step=3, sigma_0=0.5, n_atoms=51, v_min=0.0, v_max=100.0)


def rainbow_torch(seed=1, out=print, **over):
    """The stand-in script."""
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import gym, torch
    from torch import nn, optim
    hp = dict(HP, **over)
    T, B, gamma, alpha, n_step = hp["total_timesteps"], hp["batch_size"], hp["gamma"], hp["alpha"], hp["n_step"]
    slope = (hp["end_e"] - hp["start_e"]) / (hp["exploration_fraction"] * T)
    NA, v_min, v_max = hp["n_atoms"], hp["v_min"], hp["v_max"]
    dz = (v_max - v_min) / (NA - 1)
    atoms = v_min + dz * torch.arange(NA, dtype=torch.float32)

    class NoisyLinear(nn.Module):
        def __init__(self, n_in, n_out):
            super().__init__()
            bound = 1.0 / n_in ** 0.5
            self.weight_mu = nn.Parameter(torch.empty(n_out, n_in).uniform_(-bound, bound))
            self.weight_sigma = nn.Parameter(torch.full((n_out, n_in), hp["sigma_0"] / n_in ** 0.5))
            self.bias_mu = nn.Parameter(torch.empty(n_out).uniform_(-bound, bound))
            self.bias_sigma = nn.Parameter(torch.full((n_out,), hp["sigma_0"] / n_in ** 0.5))
            self.register_buffer("weight_eps", torch.zeros(n_out, n_in))
            self.register_buffer("bias_eps", torch.zeros(n_out))
            self.reset_noise()

        @staticmethod
        def f(x):
            return x.sign() * x.abs().sqrt()

        def reset_noise(self):
            e_in, e_out = self.f(torch.randn(self.weight_mu.shape[1])), self.f(torch.randn(self.weight_mu.shape[0]))
            self.weight_eps.copy_(torch.outer(e_out, e_in))
            self.bias_eps.copy_(e_out)

        def forward(self, x):
            return nn.functional.linear(x, self.weight_mu + self.weight_sigma * self.weight_eps, self.bias_mu + self.bias_sigma * self.bias_eps)

    class RainbowNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.features = nn.Sequential(nn.Linear(4, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU())
            self.value = NoisyLinear(84, NA)
            self.advantage = NoisyLinear(84, 2 * NA)

        def reset_noise(self):
            self.value.reset_noise(); self.advantage.reset_noise()

        def get_probs(self, x):
            h = self.features(x)
            adv = self.advantage(h).unflatten(-1, (2, NA))
            return torch.softmax(self.value(h).unsqueeze(-2) + (adv - adv.mean(dim=-2, keepdim=True)), dim=-1)   # the mean over the actions of each atom

        def forward(self, x):
            return (self.get_probs(x) * atoms).sum(-1)

    env = gym.wrappers.RecordEpisodeStatistics(gym.make("CartPole-v1"))
    env.seed(seed); np.random.seed(seed); torch.manual_seed(seed); env.action_space.seed(seed)
    q_network = RainbowNet()
    optimizer = optim.Adam(q_network.parameters(), lr=hp["learning_rate"])
    target_network = RainbowNet()
    target_network.load_state_dict(q_network.state_dict())
    observations = torch.zeros((T + 1, 4)); actions = torch.zeros(T + 1, dtype=torch.long)
    rewards = torch.zeros(T + 1); terminated = torch.zeros(T + 1, dtype=torch.bool)
    priorities = torch.zeros(T + 1)
    max_priority = 1e-2
    observation = torch.tensor(env.reset())
    observations[0] = observation
    rows = torch.arange(B)
    for global_step in range(T):
        epsilon = max(slope * global_step + hp["start_e"], hp["end_e"])
        if global_step < hp["learning_starts"] or np.random.random() < epsilon:
            action = torch.tensor(env.action_space.sample())
        else:
            with torch.no_grad():
                q_network.reset_noise()                                                  # a fresh network at every greedy step
                action = torch.argmax(q_network(observation), -1)
        actions[global_step] = action
        priorities[global_step] = max_priority                                       # a new row is drawn at least once soon
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
                beta = (1 - hp["beta_0"]) * g / T + hp["beta_0"]
                scaled = priorities[:g] ** alpha
                batch_inds = torch.multinomial(scaled, B, replacement=True)
                probability = scaled[batch_inds] / scaled.sum()
                weights = (g * probability) ** -beta
                weights = weights / weights.max()
                q_network.reset_noise(); target_network.reset_noise()                # one sample per network and update
                with torch.no_grad():
                    at = batch_inds + 1                                              # the first step is always taken
                    returns = rewards[at]
                    discount = torch.full((B,), gamma)
                    for _ in range(n_step - 1):
                        onward = torch.logical_not(terminated[at]) & (at < g)        # observations[g] is the newest: nothing lies behind it yet
                        at = torch.where(onward, at + 1, at)
                        returns = torch.where(onward, returns + discount * rewards[at], returns)
                        discount = torch.where(onward, discount * gamma, discount)
                    last = observations[at]
                    next_actions = torch.argmax(q_network(last), -1)                 # the ONLINE network chooses ...
                    next_probs = target_network.get_probs(last)[rows, next_actions]  # ... the TARGET network's distribution of it is projected
                    live = torch.logical_not(terminated[at]).float()
                    tz = (returns[:, None] + (discount * live)[:, None] * atoms[None, :]).clamp(v_min, v_max)
                    bj = (tz - v_min) / dz
                    lo, up = bj.floor(), bj.ceil()
                    target_probs = torch.zeros(B, NA)
                    target_probs.scatter_add_(1, lo.long(), (up + (lo == up).float() - bj) * next_probs)
                    target_probs.scatter_add_(1, up.long(), (bj - lo) * next_probs)
                probs = q_network.get_probs(observations[batch_inds])[rows, actions[batch_inds]]
                rowloss = -(target_probs * torch.log(probs + 1e-8)).sum(-1)
                priorities[batch_inds] = rowloss.detach().clamp(min=0.0)             # unweighted: the row's cross-entropy
                max_priority = max(max_priority, float(rowloss.detach().max()))      # the running maximum
                loss = (weights * rowloss).mean()
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            if g % hp["target_network_frequency"] == 0:
                target_network.load_state_dict(q_network.state_dict())
    env.close()


def run_lines(seed, **kw):
    lines = []; t0 = time.time()
    rainbow_torch(seed, out=lines.append, **kw)
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
    np.savez_compressed(out_path, rainbow_last_tenth_mean=arr)
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
        print('{"torch_rainbow_cpu_1core": {"env_steps": %d, "episodes": %d, "wall_s": %.2f, "env_steps_per_s": %.0f}}' % (T, len(steps), wall, T / wall))
    else:
        capture_learning(args.out or os.path.join(GOLD, "rainbow_learning_stats.npz"), args.seeds, args.jobs)


if __name__ == "__main__":
    main()
