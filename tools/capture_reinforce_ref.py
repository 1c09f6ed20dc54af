#!/usr/bin/env python3
"""Golden vectors from the UNMODIFIED reference ``deep_rl/reinforce.py`` (TEST INFRASTRUCTURE ONLY; never runs on a GPU machine).

Same method as oracle/capture_dqn_trace.py — runpy + oracle/gym_shim (read-only, on sys.path) + instrumentation from OUTSIDE the reference source:
  * the shim's trace sink mirrors every reset (f64 state) and step (action, f32 observation, terminated)      (reinforce.py:56,64)
  * a wrapper on ``torch.nn.Dropout.forward`` records the mask each forward used (mask = out != 0; asserted: no pre-activation is exactly 0)   (:42,60)
  * ``torch.optim.Adam.__init__`` snapshots the initial parameters; ``torch.optim.Adam.step`` records, per update, b_returns, b_log_probs, policy_loss,
    the gradients, the parameters after the step and the episode length                                                                          (:47,71-77)
Output: tests/golden/reinforce_ref_trace.npz — arrays of dtype kind f / i / u only, masks bit-packed (unit u = bit u & 7 of byte u >> 3).

  --learning --seeds 50   tests/golden/reinforce_learning_stats.npz: episodic returns of seeds 1..50 (keys as learning_stats.npz, prefix ``reinforce_``), by the
                          seed shifting of oracle/capture_learning_stats.py (``env.seed`` and ``torch.manual_seed`` wrapped from outside); seed 1 must reproduce the trace
  --time-only             the uninstrumented script on one CPU core: env steps per second (the baseline tools/bench_reinforce.py is read against)

The reference checkout is named with --reference DIR (or the environment variable DEEP_RL_REFERENCE): the directory that holds ``deep_rl/reinforce.py``.
"""
import argparse, contextlib, io, multiprocessing as mp, os, runpy, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "gym_shim")


def ref_script(reference):
    path = os.path.join(reference, "deep_rl", "reinforce.py")
    if not os.path.exists(path):
        raise SystemExit("no reference script at %s (pass --reference DIR or set DEEP_RL_REFERENCE)" % path)
    return path


def flat(params, grad=False):
    import torch
    with torch.no_grad():
        return torch.cat([(p.grad if grad else p).detach().reshape(-1) for p in params]).numpy().copy()


def run_plain(script):
    """-> (episode_global_step, episode_return, wall seconds) of one uninstrumented run in this process"""
    buf = io.StringIO(); t0 = time.time()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(script, run_name="__ref_reinforce__")
    wall = time.time() - t0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("global_step=")]
    steps = np.array([int(ln.split(",")[0].split("=")[1]) for ln in lines], np.int64)
    rets = np.array([float(ln.split("episodic_return=")[1]) for ln in lines], np.float64)
    return steps, rets, wall


def capture_trace(script, out_path):
    sys.path.insert(0, SHIM)
    import gym, torch
    torch.set_num_threads(1)
    log = {"reset": [], "action": [], "obs": [], "terminated": []}

    def sink(event, p):
        if event == "reset":
            log["reset"].append(p["state"])
        else:
            log["action"].append(p["action"]); log["obs"].append(p["obs"]); log["terminated"].append(p["terminated"])

    gym.register_trace_sink(sink)
    masks, zero_z = [], [0]
    orig_fwd = torch.nn.Dropout.forward

    def d_fwd(self, x):
        y = orig_fwd(self, x)
        zero_z[0] += int((x == 0).sum())
        masks.append((y != 0).numpy().copy())
        return y

    torch.nn.Dropout.forward = d_fwd
    rec = {"init": None, "grads": [], "params": [], "loss": [], "len": [], "bret": [], "blp": []}
    st = {}
    orig_init, orig_step = torch.optim.Adam.__init__, torch.optim.Adam.step

    def p_init(self, params, *a, **kw):
        params = list(params); st["params"] = params; rec["init"] = flat(params)
        return orig_init(self, params, *a, **kw)

    def p_step(self, *a, **kw):
        f = sys._getframe(1)
        while f is not None and "policy_loss" not in f.f_globals:
            f = f.f_back
        g = f.f_globals
        rec["grads"].append(flat(st["params"], grad=True)); rec["loss"].append(float(g["policy_loss"].detach())); rec["len"].append(int(g["step"]))
        rec["bret"].append(g["b_returns"].detach().numpy().copy()); rec["blp"].append(g["b_log_probs"].detach().numpy().copy())
        out = orig_step(self, *a, **kw)
        rec["params"].append(flat(st["params"]))
        return out

    torch.optim.Adam.__init__, torch.optim.Adam.step = p_init, p_step
    try:
        steps, rets, wall = run_plain(script)
    finally:
        torch.optim.Adam.__init__, torch.optim.Adam.step = orig_init, orig_step
        torch.nn.Dropout.forward = orig_fwd
    assert zero_z[0] == 0, "a pre-activation was exactly 0: the mask cannot be read off the dropout output"
    lens = np.array(rec["len"], np.int32)
    assert len(masks) == len(log["action"]) == int(lens.sum()) and len(log["reset"]) == len(lens)
    out = {
        "hparams": np.array([0.99, 1e-2, 0.6, 1], np.float64),   # gamma, learning rate, dropout p, seed (reinforce.py:29,47,42,36)
        "init_params": rec["init"].astype(np.float32),
        "reset_states": np.array(log["reset"], np.float64),
        "actions": np.array(log["action"], np.int8), "obs": np.array(log["obs"], np.float32), "terminated": np.array(log["terminated"], np.uint8),
        "lengths": lens,
        "masks_packed": np.packbits(np.stack(masks).reshape(-1, 128), axis=1, bitorder="little"),
        "b_returns": np.concatenate(rec["bret"]).astype(np.float32), "b_log_probs": np.concatenate(rec["blp"]).astype(np.float32),
        "policy_loss": np.array(rec["loss"], np.float64),
        "grads": np.stack(rec["grads"]).astype(np.float32), "params_after": np.stack(rec["params"]).astype(np.float32),
        "episode_global_step": steps.astype(np.int32), "episode_return": rets.astype(np.float32),
        "ref_wall_seconds": np.array([wall]),
    }
    assert all(v.dtype.kind in "fiu" for v in out.values())
    np.savez_compressed(out_path, **out)
    print("reference reinforce.py: %d env steps, %d updates, lengths %d..%d, %.1f s (instrumented: %.0f env-steps/s) -> %s (%.0f KB)" % (
        lens.sum(), len(lens), lens.min(), lens.max(), wall, lens.sum() / wall, out_path, os.path.getsize(out_path) / 1024))


def run_seed(job):
    script, seed = job
    sys.path.insert(0, SHIM)
    import gym, gym.envs, torch
    torch.set_num_threads(1)
    off = seed - 1

    def shifted(fn):
        def w(*a, **kw):
            if a and a[-1] is not None and isinstance(a[-1], int):
                a = a[:-1] + (a[-1] + off,)
            elif kw.get("seed") is not None:
                kw["seed"] = kw["seed"] + off
            return fn(*a, **kw)
        return w

    torch.manual_seed = shifted(torch.manual_seed)
    gym.envs.CartPoleEnv.seed = shifted(gym.envs.CartPoleEnv.seed)
    steps, rets, wall = run_plain(script)
    return seed, steps, rets, wall


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def capture_learning(script, out_path, seeds, jobs):
    by_seed = {}
    with mp.get_context("spawn").Pool(jobs, maxtasksperchild=1) as pool:
        for seed, steps, rets, wall in pool.imap_unordered(run_seed, [(script, s) for s in range(1, seeds + 1)]):
            by_seed[seed] = (steps, rets)
            print("seed %2d: %3d episodes, last-tenth mean %7.2f, NaN-free %s (%.0f s)" % (seed, len(rets), last_tenth(rets), bool(np.isfinite(rets).all()), wall), flush=True)
    trace = os.path.join(GOLD, "reinforce_ref_trace.npz")
    if os.path.exists(trace):   # seed 1 must be the run the trace fixture holds
        g = np.load(trace)
        assert np.array_equal(g["episode_global_step"], by_seed[1][0]) and np.allclose(g["episode_return"], by_seed[1][1])
    order = sorted(by_seed)
    out = {
        "reinforce_seeds": np.array(order, np.int32),
        "reinforce_offsets": np.cumsum([0] + [len(by_seed[s][1]) for s in order]).astype(np.int64),
        "reinforce_episode_global_step": np.concatenate([by_seed[s][0] for s in order]).astype(np.int32),
        "reinforce_episode_return": np.concatenate([by_seed[s][1] for s in order]).astype(np.float32),
        "reinforce_last_tenth_mean": np.array([last_tenth(by_seed[s][1]) for s in order], np.float64),
    }
    np.savez_compressed(out_path, **out)
    lt = out["reinforce_last_tenth_mean"]
    print("last-tenth means: mean %.1f, seed-to-seed sd %.1f -> %s (%.0f KB)" % (lt.mean(), lt.std(ddof=1), out_path, os.path.getsize(out_path) / 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEEP_RL_REFERENCE"), help="directory that holds deep_rl/reinforce.py")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--seeds", type=int, default=50)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit("pass --reference DIR or set DEEP_RL_REFERENCE")
    script = ref_script(args.reference)
    if args.time_only:
        sys.path.insert(0, SHIM)
        import torch
        torch.set_num_threads(1)
        steps, rets, wall = run_plain(script)
        print('{"reference_reinforce_cpu_1core": {"env_steps": %d, "episodes": %d, "wall_s": %.2f, "env_steps_per_s": %.0f}}' % (steps[-1], len(steps), wall, steps[-1] / wall))
    elif args.learning:
        capture_learning(script, args.out or os.path.join(GOLD, "reinforce_learning_stats.npz"), args.seeds, args.jobs)
    else:
        capture_trace(script, args.out or os.path.join(GOLD, "reinforce_ref_trace.npz"))


if __name__ == "__main__":
    main()
