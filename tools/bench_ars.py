#!/usr/bin/env python3
"""Times the launches of libmirl_ars.so on one MI355X and writes ONE JSON line to profiles/ars_bench.json (carrying the library's source id).

At N = 8 and N = 4,096 directions, with M frozen (step size 0) at the balancing controller — every episode runs its 500 steps — and at zero (random linear
policies), it times the episode launch, the update launch and the whole iteration: the median [min, max] of five windows bracketed by HIP events, env-steps/s and
the update's share of the iteration.  In the same run it times mi_ev_episodes (libmirl_eval.so) with the QR kind on its controller at 16 and 8,192 episodes — the
same episode counts, every episode 500 steps — as the yardstick for "per env step, no slower".

    python tools/bench_ars.py [--windows 5] [--reps 10] [--out profiles/ars_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

RULE_W = np.array([0.02, 0.1, 1.0, 0.5])   # (x, x_dot, theta, theta_dot): a = (w . obs > 0) balances the pole
CONTROLLER_K = 16.0


def windows(fn, n_windows, reps):
    """-> [median, min, max] microseconds per call over n_windows windows of `reps` calls"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return [float(np.median(out)), float(min(out)), float(max(out))]


def ars_case(dev, N, policy, n_windows, reps):
    import deep_rl_amd as D
    from deep_rl_amd import _native_ars as K

    # step size 0: the update runs and M keeps its bits; normalize off: the statistics are folded and norm stays 0 / 1, under which the controller is the rule
    eng = D.ARSEngine(n_directions=N, n_top=max(1, N // 2), step_size=0.0, noise=0.03, normalize=False, device=dev)
    if policy == "controller":
        w = (CONTROLLER_K * RULE_W).astype(np.float32)
        eng.policy.load_flat(np.concatenate([-w, w]))
    E = 2 * N
    returns = torch.empty(E, dtype=torch.float32, device=dev)
    lengths = torch.empty(E, dtype=torch.int32, device=dev)
    a = eng.args(returns, lengths, eng.truncated)
    s = K.stream_ptr(dev)
    L = K.lib()
    ep = windows(lambda: K.check(L.mi_ars_episodes(C.byref(a), s)), n_windows, reps)
    steps = int(lengths.sum().item())
    up = windows(lambda: K.check(L.mi_ars_update(C.byref(a), s)), n_windows, reps)
    it = windows(lambda: K.check(L.mi_ars_iterate(C.byref(a), 1, s)), n_windows, reps)
    return dict(n_directions=N, policy=policy, episodes=E, env_steps_per_launch=steps, episode_us=ep, update_us=up, iteration_us=it,
                env_steps_per_s=steps / (ep[0] * 1e-6), ns_per_env_step=ep[0] * 1e3 / steps, update_share=up[0] / it[0])


def eval_case(dev, E, n_windows, reps):
    import types

    import deep_rl_amd as D
    from deep_rl_amd import _native_ev as EV

    spec = types.SimpleNamespace(observation_space=types.SimpleNamespace(shape=(4,)), action_space=types.SimpleNamespace(n=2), device=dev)
    net = D.QRQNetwork(spec)
    p = np.zeros(21644, np.float32)   # two units carry +-w . obs into every quantile of actions 1 / 0: q_1 - q_0 = K (w . obs)
    W1, W2, W3 = p[0:480].reshape(120, 4), p[600:10680].reshape(84, 120), p[10764:21516].reshape(2, 64, 84)
    W1[0], W1[1] = RULE_W, -RULE_W
    W2[0, 0] = W2[1, 1] = 1
    W3[1, :, 0] = W3[0, :, 1] = CONTROLLER_K
    net.load_flat(p)
    res = D.evaluate(net, episodes=E)
    steps = int(res.lengths.sum().item())
    t = windows(lambda: D.evaluate(net, episodes=E), n_windows, reps)
    return dict(kind="QR", episodes=E, env_steps_per_launch=steps, episode_us=t, env_steps_per_s=steps / (t[0] * 1e-6), ns_per_env_step=t[0] * 1e3 / steps,
                eval_source_id=EV.source_id())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ars_bench.json"))
    args = ap.parse_args()
    from deep_rl_amd import _native_ars as K

    dev = torch.device("cuda", 0)
    out = dict(ars_source_id=K.source_id(), device=torch.cuda.get_device_name(dev), windows=args.windows, reps=args.reps, unit="us: median [min, max] of the windows",
               ars=[ars_case(dev, N, pol, args.windows, args.reps) for N in (8, 4096) for pol in ("controller", "zero")],
               eval_qr=[eval_case(dev, E, args.windows, args.reps) for E in (16, 8192)])
    line = json.dumps(out, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
