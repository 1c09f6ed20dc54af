#!/usr/bin/env python3
"""Golden vectors from the UNMODIFIED reference ``deep_rl/c51.py`` (TEST INFRASTRUCTURE ONLY; never runs on a GPU machine).

Same method as tools/capture_reinforce_ref.py — runpy + oracle/gym_shim (read-only, on sys.path) + instrumentation from OUTSIDE the reference source:
  * the shim's trace sink mirrors every reset (f64 state) and step (action, f32 observation, terminated)                                      (c51.py:86,106,108)
  * a wrapper on ``torch.argmax`` notes the steps at which the script acted greedily (the call with a 1-D argument, :100)
  * ``torch.optim.Adam.__init__`` snapshots the initial parameters; ``torch.optim.Adam.step`` reads c51.py's module globals from the calling frame: per update
    ``batch_inds`` and ``loss``, and at the CHECKPOINT updates the online and target parameters before the step, ``target_probs``, the greedy ``action`` of
    :144, ``probs`` of :156, the gradient and the parameters after the step                                                                   (:124-163)
Output, arrays of dtype kind f / i / u only:
  tests/golden/c51_ref_trace.npz      the run: initial parameters, all 20,000 steps, all 1,001 batch_inds and losses, the printed episode lines
  tests/golden/c51_ref_ckpt<k>.npz    one file per checkpoint update k (a parameter vector is 112 KB: every committed file stays below 1 MiB)
Checkpoints: the first update (which sits directly before the target sync at global_step 10,000), the one directly after it, the pair around the sync at
10,500, one in mid-run and the last; at least one of their batches must hold a terminated row (asserted).

  --learning --seeds 100   tests/golden/c51_learning_stats.npz: episodic returns of seeds 1..100 (keys as learning_stats.npz, prefix ``c51_``) through
                           ``run_one`` of oracle/capture_learning_stats.py (the seed shifting lives there); seed 1 must reproduce the trace
  --time-only              the uninstrumented script on one CPU core: env steps per second (the baseline tools/bench_c51.py is read against)

The reference checkout is named with --reference DIR (or the environment variable DEEP_RL_REFERENCE): the directory that holds ``deep_rl/c51.py``.
"""
import argparse, contextlib, importlib.util, io, multiprocessing as mp, os, runpy, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "gym_shim")
CHECKPOINTS = (0, 1, 50, 51, 500, 1000)   # update indices; update k runs at global_step 10,000 + 10 k, the target syncs at multiples of 500 BEHIND that step's update


def ref_script(reference):
    path = os.path.join(reference, "deep_rl", "c51.py")
    if not os.path.exists(path):
        raise SystemExit("no reference script at %s (pass --reference DIR or set DEEP_RL_REFERENCE)" % path)
    return path


def flat(params, grad=False):
    import torch
    with torch.no_grad():
        return torch.cat([(p.grad if grad else p).detach().reshape(-1) for p in params]).numpy().copy()


def run_plain(script):
    """-> (episode_global_step, episode_return, wall seconds) of one run in this process"""
    buf = io.StringIO(); t0 = time.time()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(script, run_name="__ref_c51__")
    wall = time.time() - t0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("global_step=")]
    steps = np.array([int(ln.split(",")[0].split("=")[1]) for ln in lines], np.int64)
    rets = np.array([float(ln.split("episodic_return=")[1]) for ln in lines], np.float64)
    return steps, rets, wall


def capture_trace(script, out_path):
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
    greedy = []
    orig_argmax = torch.argmax

    def argmax(x, *a, **kw):
        if x.dim() == 1:
            greedy.append(len(log["action"]))   # the step about to be taken
        return orig_argmax(x, *a, **kw)

    torch.argmax = argmax
    rec = {"init": None, "inds": [], "loss": [], "ckpt": {}}
    st = {}
    orig_init, orig_step = torch.optim.Adam.__init__, torch.optim.Adam.step

    def p_init(self, params, *a, **kw):
        params = list(params); st["params"] = params; rec["init"] = flat(params)
        return orig_init(self, params, *a, **kw)

    def p_step(self, *a, **kw):
        f = sys._getframe(1)
        while f is not None and "target_probs" not in f.f_globals:
            f = f.f_back
        g = f.f_globals
        k = len(rec["loss"])
        assert g["global_step"] == 10_000 + 10 * k
        rec["inds"].append(np.asarray(g["batch_inds"]).copy()); rec["loss"].append(float(g["loss"].detach()))
        c = None
        if k in CHECKPOINTS:
            c = rec["ckpt"][k] = {
                "update": np.array([k], np.int32), "global_step": np.array([g["global_step"]], np.int32),
                "batch_inds": np.asarray(g["batch_inds"]).astype(np.int32), "loss": np.array([float(g["loss"].detach())], np.float64),
                "params_before": flat(st["params"]), "target_params": flat(list(g["target_network"].parameters())),
                "target_probs": g["target_probs"].detach().numpy().copy(), "next_actions": g["action"].numpy().astype(np.int32),
                "probs": g["probs"].detach().numpy().copy(), "grads": flat(st["params"], grad=True),
                "batch_terminated": g["b_terminated"].numpy().astype(np.uint8),
            }
        out = orig_step(self, *a, **kw)
        if c is not None:
            c["params_after"] = flat(st["params"])
        return out

    torch.optim.Adam.__init__, torch.optim.Adam.step = p_init, p_step
    try:
        steps, rets, wall = run_plain(script)
    finally:
        torch.optim.Adam.__init__, torch.optim.Adam.step = orig_init, orig_step
        torch.argmax = orig_argmax
    T = len(log["action"])
    assert T == 20_000 and len(rec["loss"]) == 1001 and sorted(rec["ckpt"]) == sorted(CHECKPOINTS)
    assert any(c["batch_terminated"].any() for c in rec["ckpt"].values()), "no checkpoint batch holds a terminated row"
    is_greedy = np.zeros(T, np.uint8); is_greedy[np.array(greedy, np.int64)] = 1
    out = {
        "hparams": np.array([0.99, 2.5e-4, 0.01 / 128, 1, 0.05, 0.5, 20_000, 10_000, 10, 128, 500, 1], np.float64),   # gamma, lr, Adam eps, start_e, end_e,
        # exploration_fraction, total_timesteps, learning_starts, train_frequency, batch_size, target_network_frequency, seed (c51.py:42-54,67,75)
        "init_params": rec["init"].astype(np.float32),
        "reset_states": np.array(log["reset"], np.float64), "reset_at": np.array(log["reset_at"], np.int32),   # reset r happened after reset_at[r] steps
        "actions": np.array(log["action"], np.int8), "obs": np.array(log["obs"], np.float32), "terminated": np.array(log["terminated"], np.uint8),
        "greedy": is_greedy,
        "batch_inds": np.stack(rec["inds"]).astype(np.int32), "loss": np.array(rec["loss"], np.float64),
        "checkpoints": np.array(CHECKPOINTS, np.int32),
        "episode_global_step": steps.astype(np.int32), "episode_return": rets.astype(np.float32),
        "ref_wall_seconds": np.array([wall]),
    }
    assert all(v.dtype.kind in "fiu" for v in out.values())
    np.savez_compressed(out_path, **out)
    sizes = [os.path.getsize(out_path)]
    for k, c in rec["ckpt"].items():
        c = {n: (v.astype(np.float32) if v.dtype.kind == "f" and n != "loss" else v) for n, v in c.items()}
        assert all(v.dtype.kind in "fiu" for v in c.values())
        p = os.path.join(os.path.dirname(out_path), "c51_ref_ckpt%d.npz" % k)
        np.savez_compressed(p, **c)
        sizes.append(os.path.getsize(p))
    assert max(sizes) < (1 << 20), sizes
    print("reference c51.py: %d env steps, %d episodes, %d updates (%d greedy steps), final loss %.4f, %.1f s -> %s + %d checkpoint files (%s KB)" % (
        T, len(steps), len(rec["loss"]), int(is_greedy.sum()), rec["loss"][-1], wall, out_path, len(rec["ckpt"]), ", ".join("%.0f" % (s / 1024) for s in sizes)))


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def _run_one(job):
    spec = importlib.util.spec_from_file_location("capture_learning_stats", os.path.join(ROOT, "oracle", "capture_learning_stats.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod.run_one(job)


def capture_learning(out_path, seeds, jobs):
    by_seed = {}
    with mp.get_context("spawn").Pool(jobs, maxtasksperchild=1) as pool:
        for _script, seed, steps, rets, wall in pool.imap_unordered(_run_one, [("c51", s) for s in range(1, seeds + 1)]):
            by_seed[seed] = (steps, rets)
            print("seed %3d: %4d episodes, last-tenth mean %7.2f (%.0f s)" % (seed, len(rets), last_tenth(rets), wall), flush=True)
    trace = os.path.join(GOLD, "c51_ref_trace.npz")
    if os.path.exists(trace):   # seed 1 must be the run the trace fixture holds
        g = np.load(trace)
        assert np.array_equal(g["episode_global_step"], by_seed[1][0]) and np.allclose(g["episode_return"], by_seed[1][1])
    order = sorted(by_seed)
    out = {
        "c51_seeds": np.array(order, np.int32),
        "c51_offsets": np.cumsum([0] + [len(by_seed[s][1]) for s in order]).astype(np.int64),
        "c51_episode_global_step": np.concatenate([by_seed[s][0] for s in order]).astype(np.int32),
        "c51_episode_return": np.concatenate([by_seed[s][1] for s in order]).astype(np.float32),
        "c51_last_tenth_mean": np.array([last_tenth(by_seed[s][1]) for s in order], np.float64),
    }
    np.savez_compressed(out_path, **out)
    lt = out["c51_last_tenth_mean"]
    print("last-tenth means: mean %.2f, seed-to-seed sd %.2f -> %s (%.0f KB)" % (lt.mean(), lt.std(ddof=1), out_path, os.path.getsize(out_path) / 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEEP_RL_REFERENCE"), help="directory that holds deep_rl/c51.py")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.learning:   # (oracle/capture_learning_stats.py names the reference itself)
        return capture_learning(args.out or os.path.join(GOLD, "c51_learning_stats.npz"), args.seeds, args.jobs)
    if not args.reference:
        raise SystemExit("pass --reference DIR or set DEEP_RL_REFERENCE")
    script = ref_script(args.reference)
    if args.time_only:
        sys.path.insert(0, SHIM)
        import torch
        torch.set_num_threads(1)
        steps, rets, wall = run_plain(script)
        print('{"reference_c51_cpu_1core": {"env_steps": %d, "episodes": %d, "wall_s": %.2f, "env_steps_per_s": %.0f}}' % (20_000, len(steps), wall, 20_000 / wall))
    else:
        capture_trace(script, args.out or os.path.join(GOLD, "c51_ref_trace.npz"))


if __name__ == "__main__":
    main()
