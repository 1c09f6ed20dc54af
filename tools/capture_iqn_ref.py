#!/usr/bin/env python3
"""Golden vectors from the reference ``deep_rl/iqn.py``, re-targeted to CartPole-v1 (TEST INFRASTRUCTURE ONLY; CPU only, never runs on a GPU machine).

The reference script needs ALE, cv2 and ``utils.AtariWrapper`` and cannot run as a whole.  This tool reads its source at capture time and, with ``ast``, picks out
  * the definitions of ``initialize_weights_he``, ``CosineEmbeddingNetwork`` and ``QuantileNetwork``,
  * the statement suite of the greedy acting branch (the ``else`` of ``if global_step < learning_starts or np.random.rand() < epsilon``),
  * the statement suite of the update block (the body of ``if global_step % train_frequency == 0``),
compiles them in memory and runs them in a namespace the tool prepares: the re-targeted ``FeaturesExtractor`` (each Conv2d(c_in, c_out, k, s) becomes
Linear(c_in, c_out)), the re-targeted horizon, the CartPole of oracle/gym_shim, the CPU device.  No reference text is written anywhere; this file holds only its own
substitutions and its own loop around the two suites (the control flow of iqn.py:185-299 restated).

Both suites divide the observation by 255, so the tool's storage holds 255 * x (f32) and the fixtures record the network inputs the suites actually formed,
``(255 * x) / 255`` in f32.  ``torch.rand`` and ``torch.cos`` are wrapped from outside while a suite runs: the first logs the tau draws, the second the i_pi table
(argument / tau).

Output, arrays of dtype kind f / i / u only, each file < 1 MiB:
  tests/golden/iqn_ref_start.npz      parameters, target parameters and Adam's two moments at the window's start
  tests/golden/iqn_ref_trace.npz      21 chained updates late in one full run, a target sync behind the 11th: initial parameters, i_pi, the sampled transitions and their successors as a compact ring (the inputs the update block
                                      formed), per update batch_inds / taus / next_taus / tau_dashes / loss, the number of td errors inside the kappa margin and what
                                      they could move the loss by, and a few acting forwards.  The trace run uses a batch of TRACE_BATCH rows
  tests/golden/iqn_ref_ckpt<k>.npz    window updates k = the first that satisfies the conditions, 10, 11 (the pair around the sync) and the last that does:
                                      parameters before, target parameters, current / target quantiles, next actions, gradient, parameters after
The window is chosen and asserted: at every checkpoint no |td error| lies within KAPPA_MARGIN_REL x max(1, max |quantile|) of kappa, and at least one checkpoint
batch row is terminated.  The acting forwards use the online networks as the window's last update leaves them.

  --learning --seeds 50    tests/golden/iqn_learning_stats.npz: episodic returns of seeds 1..50 at the re-targeted horizon (keys as c51_learning_stats.npz, prefix iqn_)
  --time-only              one seed on one CPU core: env steps per second (the baseline tools/bench_iqn.py is read against)

The reference checkout is named with --reference DIR (or DEEP_RL_REFERENCE): the directory that holds ``deep_rl/iqn.py``.
"""
import argparse, ast, multiprocessing as mp, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
SHIM = os.path.join(ROOT, "oracle", "gym_shim")
KAPPA_MARGIN_REL = 4.8e-6   # a checkpoint is clear when no |td error| lies within this x max(1, max |quantile|) of kappa (NEAR_KAPPA_REL of tests/_iqn_ref.py, 8 x the
# measured quantile error)
TRACE_BATCH = 8             # batch size of the trace run: at the reference's 32 the 131,072 td errors of an update lie so densely around kappa (= CartPole's reward)
# that no update of two whole runs kept the margin; at 8 rows about one update in four does
LOG_FROM = 3_000            # the trace run looks for its window from this global step on and stops once it has one (about one update in eight keeps clear)
KEEP = 32                   # updates whose full record is kept while looking
# the re-target: horizon of the drop-in script; everything else is read from the reference's module-level assignments
RETARGET = dict(env_id="CartPole-v1", total_timesteps=50_000, learning_starts=1_000, epsilon_decay_steps=10_000, target_network_frequency=500, embedding_dim=64)
HPARAM_NAMES = ("final_epsilon", "train_frequency", "batch_size", "gamma", "learning_rate", "num_tau_samples", "num_tau_prime_samples", "num_quantile_samples", "num_cosines", "kappa")


def _mentions(node, name):
    return any(isinstance(n, ast.Name) and n.id == name for n in ast.walk(node))


def extract(reference):
    """-> (definitions code, acting-suite code, update-suite code, {hyper-parameter: value}) from the reference source"""
    path = os.path.join(reference, "deep_rl", "iqn.py")
    if not os.path.exists(path):
        raise SystemExit("no reference script at %s (pass --reference DIR or set DEEP_RL_REFERENCE)" % path)
    tree = ast.parse(open(path).read(), path)
    defs = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in ("initialize_weights_he", "CosineEmbeddingNetwork", "QuantileNetwork")]
    assert len(defs) == 3
    hp = {}
    for n in tree.body:
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) and n.targets[0].id in HPARAM_NAMES:
            hp[n.targets[0].id] = ast.literal_eval(n.value)
    assert sorted(hp) == sorted(HPARAM_NAMES), hp
    loop = [n for n in tree.body if isinstance(n, ast.While)]
    assert len(loop) == 1
    act = [n for n in loop[0].body if isinstance(n, ast.If) and _mentions(n.test, "epsilon") and _mentions(n.test, "learning_starts")]
    assert len(act) == 1 and act[0].orelse
    upd = [n for n in ast.walk(loop[0]) if isinstance(n, ast.If) and _mentions(n.test, "train_frequency")]
    assert len(upd) == 1
    mod = lambda body, tag: compile(ast.fix_missing_locations(ast.Module(body=list(body), type_ignores=[])), "<reference %s>" % tag, "exec")   # noqa: E731
    return mod(defs, "definitions"), mod(act[0].orelse, "acting"), mod(upd[0].body, "update"), hp


def flat(params, grad=False):
    import torch
    with torch.no_grad():
        return torch.cat([(p.grad if grad else p).detach().reshape(-1) for p in params]).numpy().copy()


class Run:
    """The tool's own loop (the control flow of iqn.py:139-299) around the two extracted suites."""

    def __init__(self, reference, seed, overrides=(), log=False, log_from=0):
        sys.path.insert(0, SHIM) if SHIM not in sys.path else None
        import gym, torch
        from torch import nn, optim
        torch.set_num_threads(1)
        self.torch = torch
        defs, self.act_code, self.upd_code, hp = extract(reference)
        g = self.g = {"torch": torch, "np": np, "nn": nn, "optim": optim, "gym": gym, "Tensor": torch.Tensor, "__name__": "__ref_iqn__"}
        g.update(hp); g.update(RETARGET); g.update(dict(overrides))
        exec(defs, g)

        class FeaturesExtractor(nn.Module):   # the re-target: Conv2d(c_in, c_out, k, s) -> Linear(c_in, c_out), spatial extent 1 x 1
            def __init__(self, env):
                super().__init__()
                self.net = nn.Sequential(nn.Linear(env.observation_space.shape[0], 32), nn.ReLU(), nn.Linear(32, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(),
                                         nn.Flatten()).apply(g["initialize_weights_he"])

            def forward(self, input):
                return self.net(input)

        g["FeaturesExtractor"] = FeaturesExtractor
        g["slope"] = -(1.0 - g["final_epsilon"]) / g["epsilon_decay_steps"]
        g["memory_size"] = g["total_timesteps"] + 1
        env = gym.wrappers.RecordEpisodeStatistics(gym.make(g["env_id"]))
        torch.manual_seed(seed); np.random.seed(seed); env.seed(seed); env.action_space.seed(seed); env.observation_space.seed(seed)
        g["env"], g["device"] = env, torch.device("cpu")
        for role in ("online", "target"):
            g[role + "_features_extractor"] = FeaturesExtractor(env)
            g[role + "_cosine_net"] = g["CosineEmbeddingNetwork"](num_cosines=g["num_cosines"], embedding_dim=g["embedding_dim"])
            g[role + "_quantile_net"] = g["QuantileNetwork"](num_actions=env.action_space.n, embedding_dim=g["embedding_dim"])
        self.sync()
        self.params = [*g["online_features_extractor"].parameters(), *g["online_cosine_net"].parameters(), *g["online_quantile_net"].parameters()]
        self.init_params = flat(self.params)
        g["optimizer"] = optim.Adam(self.params, lr=g["learning_rate"], eps=1e-2 / g["batch_size"])
        M = g["memory_size"]
        g["observations"] = torch.zeros((M, 4), dtype=torch.float32)   # holds 255 * x: both suites divide by 255
        g["actions"] = torch.zeros(M, dtype=torch.long)
        g["rewards"] = torch.zeros(M, dtype=torch.float32)
        g["terminated"] = torch.zeros(M, dtype=torch.bool)
        self.log, self.log_from = log, log_from
        self.rands = []
        self.updates, self.ckpt, self.episodes = [], {}, []
        self.on_update, self.stop = None, False

    def target_params(self):
        g = self.g
        return flat([*g["target_features_extractor"].parameters(), *g["target_cosine_net"].parameters(), *g["target_quantile_net"].parameters()])

    def sync(self):
        g = self.g
        for n in ("features_extractor", "cosine_net", "quantile_net"):
            g["target_" + n].load_state_dict(g["online_" + n].state_dict())

    def suite(self, code):
        """run one extracted suite with torch.rand wrapped from outside (the tau draws, in call order)"""
        torch = self.torch
        if not self.log:
            exec(code, self.g)
            return
        orig_rand = torch.rand
        self.rands = []

        def rand(*a, **kw):
            out = orig_rand(*a, **kw); self.rands.append(out.numpy().copy()); return out

        torch.rand = rand
        try:
            exec(code, self.g)
        finally:
            torch.rand = orig_rand

    def capture_ipi(self):
        """the i_pi table of the reference's CosineEmbeddingNetwork.forward: the argument torch.cos sees for tau = 1 (1 * x is exact)"""
        torch = self.torch
        seen = []
        orig_cos = torch.cos
        torch.cos = lambda x: (seen.append(x.detach().numpy().copy()), orig_cos(x))[1]
        try:
            with torch.no_grad():
                self.g["online_cosine_net"](torch.ones(1, 1))
        finally:
            torch.cos = orig_cos
        return seen[0].reshape(-1).astype(np.float32)

    def loop(self):
        g, torch = self.g, self.torch
        env, M = g["env"], g["memory_size"]
        g["observation"] = torch.tensor(env.reset()) * 255.0
        g["global_step"] = 0
        g["observations"][0] = g["observation"]
        while g["global_step"] < g["total_timesteps"] and not self.stop:
            gs = g["global_step"]
            g["epsilon"] = max(1.0 + g["slope"] * gs, g["final_epsilon"])
            if gs < g["learning_starts"] or np.random.rand() < g["epsilon"]:
                g["action"] = torch.tensor(env.action_space.sample())
            else:
                exec(self.act_code, g)
            g["actions"][gs % M] = g["action"]
            obs, reward, done, info = env.step(g["action"].cpu().numpy())
            if done:
                obs = env.reset()
            g["observation"] = torch.tensor(obs) * 255.0
            gs = g["global_step"] = gs + 1
            g["observations"][gs % M] = g["observation"]
            g["rewards"][gs % M] = reward
            g["terminated"][gs % M] = done and not info.get("TimeLimit.truncated", False)
            if "episode" in info:
                self.episodes.append((gs, float(info["episode"]["r"])))
            if gs >= g["learning_starts"]:
                if gs % g["train_frequency"] == 0:
                    self.update()
                if gs % g["target_network_frequency"] == 0:
                    self.sync()

    def update(self):
        g = self.g
        k = len(self.updates)
        want = self.log and g["global_step"] >= self.log_from
        if not want:
            exec(self.upd_code, g)
            self.updates.append(None)
            return
        before, tgt = flat(self.params), self.target_params()
        st = g["optimizer"].state
        m, v = (np.concatenate([st[p][n].numpy().reshape(-1) for p in self.params]) for n in ("exp_avg", "exp_avg_sq"))
        self.suite(self.upd_code)
        taus, next_taus, tau_dashes = self.rands
        self.updates.append(dict(batch_inds=np.asarray(g["batch_inds"]).astype(np.int32), taus=taus, next_taus=next_taus, tau_dashes=tau_dashes,
                                 loss=float(g["quantile_loss"].detach())))
        if want:
            d = lambda n: g[n].detach().numpy().copy()   # noqa: E731
            self.ckpt[k] = {
                "update": np.array([k], np.int32), "global_step": np.array([g["global_step"]], np.int32), "batch_inds": np.asarray(g["batch_inds"]).astype(np.int32),
                "loss": np.array([float(g["quantile_loss"].detach())], np.float64), "params_before": before, "target_params": tgt, "exp_avg": m, "exp_avg_sq": v,
                "b_observations": d("b_observations"), "b_next_observations": d("b_next_observations"), "b_actions": d("b_actions").astype(np.int32),
                "b_rewards": d("b_rewards"), "b_terminated": d("b_terminated").astype(np.uint8),
                "taus": taus, "next_taus": next_taus, "tau_dashes": tau_dashes,
                "current_action_quantiles": d("current_action_quantiles"), "target_action_quantiles": d("target_action_quantiles"),
                "next_actions": d("next_actions").astype(np.int32), "td_errors": d("td_errors"),
                "grads": flat(self.params, grad=True), "params_after": flat(self.params),
            }
            c = self.ckpt[k]
            scale = max(1.0, float(np.abs(c["current_action_quantiles"]).max()), float(np.abs(c["target_action_quantiles"]).max()))
            td = c.pop("td_errors")
            near = np.abs(np.abs(td) - g["kappa"]) <= KAPPA_MARGIN_REL * scale
            c["clear"] = not bool(near.any())
            # what the loss can move by if every td error inside the margin took the other Huber branch: the value jumps from d^2 to |d| - kappa / 2 there
            w = np.abs(taus[:, :, None] - (td < 0).astype(np.float32))
            c["flip_allowance"] = float((w * np.abs(td * td - (np.abs(td) - 0.5 * g["kappa"])))[near].sum() / (td.shape[0] * td.shape[2]))
            c["near_kappa"] = int(near.sum())
            self.ckpt.pop(k - KEEP, None)
            if self.on_update is not None and self.on_update(k):
                self.stop = True

    def acting_forwards(self, n=8):
        """the acting suite on n stored observations with the final online networks -> obs (as formed), taus, quantiles, q, action"""
        g, torch = self.g, self.torch
        out = {"obs": [], "taus": [], "quantiles": [], "q": [], "action": []}
        for i in np.linspace(g["global_step"] - 200, g["global_step"], n).astype(int):
            g["observation"] = g["observations"][i].clone()
            self.suite(self.act_code)
            out["obs"].append(g["observation_"].numpy().reshape(4).copy()); out["taus"].append(self.rands[0].reshape(-1))
            out["quantiles"].append(g["quantiles"].numpy().copy()); out["q"].append(g["q_values"].numpy().copy()); out["action"].append(int(g["action"]))
        return {k: np.array(v) for k, v in out.items()}


def last_tenth(rets):
    k = max(len(rets) // 10, 1)
    return float(np.mean(rets[-k:]))


def capture_trace(reference, out_path, seed=1):
    """One run at the re-targeted horizon; the fixture is a window of 21 chained updates late in it, around a target sync, and the run stops behind the window.
    (A fresh network's td errors cluster AT kappa — CartPole's reward is 1 — so that every early update has elements inside the margin; a trained one's are
    spread over hundreds of units, and about one update in five keeps clear.)"""
    r = Run(reference, seed, overrides=[("batch_size", TRACE_BATCH)], log=True, log_from=LOG_FROM)
    g = r.g
    tnf = g["target_network_frequency"]
    step_of = lambda k: int(r.ckpt[k]["global_step"][0])   # noqa: E731
    found = {}

    def on_update(k):
        ks = k - 10                                      # the update directly before a sync, ten updates on either side
        if ks - 10 not in r.ckpt or step_of(ks) % tnf != 0 or not (r.ckpt[ks]["clear"] and r.ckpt[ks + 1]["clear"]):
            return False
        window = list(range(ks - 10, ks + 11))
        wclear = [j for j in window if r.ckpt[j]["clear"]]
        cps = sorted({wclear[0], ks, ks + 1, wclear[-1]})
        if len(cps) != 4 or not any(r.ckpt[j]["b_terminated"].any() for j in cps):
            return False
        found.update(window=window, cps=cps, ks=ks)
        return True

    r.on_update = on_update
    r.loop()
    if not found:
        raise SystemExit("no target sync behind step %d has a clear pair of updates around it" % LOG_FROM)
    window, CHECKPOINTS = found["window"], found["cps"]
    for k in CHECKPOINTS:   # asserted, not just searched for
        assert r.ckpt[k]["clear"]
    assert any(r.ckpt[k]["b_terminated"].any() for k in CHECKPOINTS), "no checkpoint batch holds a terminated row"
    # the compact ring: rows 2 m / 2 m + 1 hold the m-th sampled transition of the window and its successor, so a fixture index is 2 m and its successor 2 m + 1
    M = g["memory_size"]
    inds = np.concatenate([r.ckpt[k]["batch_inds"] for k in window]).astype(np.int64)
    rows = np.stack([inds, (inds + 1) % M], 1).reshape(-1)
    obs = (g["observations"].float() / 255.0).numpy()   # the inputs the update block forms
    acting = r.acting_forwards()
    B = g["batch_size"]
    out = {
        "hparams": np.array([g["gamma"], g["learning_rate"], 1e-2 / g["batch_size"], g["final_epsilon"], g["kappa"], g["batch_size"], g["train_frequency"],
                             g["learning_starts"], tnf, g["total_timesteps"], seed], np.float64),
        "init_params": r.init_params.astype(np.float32), "i_pi": r.capture_ipi(),
        "start_adam_step": np.array([window[0]], np.int64),   # optimizer steps taken before the window
        "ring_observations": obs[rows].astype(np.float32), "ring_actions": g["actions"][rows].numpy().astype(np.int8),
        "ring_rewards": g["rewards"][rows].numpy().astype(np.float32), "ring_terminated": g["terminated"][rows].numpy().astype(np.uint8),
        "ring_source_index": rows.astype(np.int32),
        "update_global_step": np.array([step_of(k) for k in window], np.int32), "sync_after_update": np.array([10], np.int32),
        "batch_inds": (2 * np.arange(len(inds), dtype=np.int32)).reshape(len(window), B),
        "taus": np.stack([r.ckpt[k]["taus"] for k in window]), "next_taus": np.stack([r.ckpt[k]["next_taus"] for k in window]),
        "tau_dashes": np.stack([r.ckpt[k]["tau_dashes"] for k in window]),
        "loss": np.array([r.ckpt[k]["loss"][0] for k in window], np.float64),
        "near_kappa": np.array([r.ckpt[k]["near_kappa"] for k in window], np.int32), "flip_allowance": np.array([r.ckpt[k]["flip_allowance"] for k in window], np.float64),
        "checkpoints": np.array([k - window[0] for k in CHECKPOINTS], np.int32),
        "act_params": flat(r.params),   # the online networks behind the window's last update, which the acting forwards used
        "act_obs": acting["obs"].astype(np.float32), "act_taus": acting["taus"].astype(np.float32), "act_quantiles": acting["quantiles"].astype(np.float32),
        "act_q": acting["q"].astype(np.float32), "act_action": acting["action"].astype(np.int32),
        "episode_global_step": np.array([e[0] for e in r.episodes], np.int32), "episode_return": np.array([e[1] for e in r.episodes], np.float32),
    }
    assert all(v.dtype.kind in "fiu" for v in out.values())
    np.savez_compressed(out_path, **out)
    sizes = [os.path.getsize(out_path)]
    c0 = r.ckpt[window[0]]   # the state at the window's start, a file of its own (four parameter-sized vectors)
    p = os.path.join(os.path.dirname(out_path), "iqn_ref_start.npz")
    np.savez_compressed(p, params=c0["params_before"], target_params=c0["target_params"], exp_avg=c0["exp_avg"], exp_avg_sq=c0["exp_avg_sq"])
    sizes.append(os.path.getsize(p))
    for k in CHECKPOINTS:
        w = k - window[0]
        c = {n: v for n, v in r.ckpt[k].items() if n not in ("clear", "exp_avg", "exp_avg_sq", "flip_allowance", "near_kappa")}
        c["update"] = np.array([w], np.int32); c["batch_inds"] = out["batch_inds"][w]
        assert all(v.dtype.kind in "fiu" for v in c.values())
        p = os.path.join(os.path.dirname(out_path), "iqn_ref_ckpt%d.npz" % w)
        np.savez_compressed(p, **c)
        sizes.append(os.path.getsize(p))
    assert max(sizes) < (1 << 20), sizes
    print("reference iqn.py suites on CartPole-v1: seed %d, %d env steps, window = updates %d..%d, checkpoints %s, last-tenth return %.1f -> %s + %d checkpoint files (%s KB)" % (
        seed, g["global_step"], window[0], window[-1], [k - window[0] for k in CHECKPOINTS], last_tenth([e[1] for e in r.episodes]), out_path, len(CHECKPOINTS),
        ", ".join("%.0f" % (x / 1024) for x in sizes)))


def _run_one(job):
    reference, seed = job
    t0 = time.time()
    r = Run(reference, seed)
    r.loop()
    steps = np.array([e[0] for e in r.episodes], np.int64); rets = np.array([e[1] for e in r.episodes], np.float64)
    return seed, steps, rets, time.time() - t0


def capture_learning(reference, out_path, seeds, jobs):
    by_seed = {}
    with mp.get_context("spawn").Pool(jobs, maxtasksperchild=1) as pool:
        for seed, steps, rets, wall in pool.imap_unordered(_run_one, [(reference, s) for s in range(1, seeds + 1)]):
            by_seed[seed] = (steps, rets)
            print("seed %3d: %4d episodes, last-tenth mean %7.2f (%.0f s)" % (seed, len(rets), last_tenth(rets), wall), flush=True)
    order = sorted(by_seed)
    out = {
        "iqn_seeds": np.array(order, np.int32),
        "iqn_offsets": np.cumsum([0] + [len(by_seed[s][1]) for s in order]).astype(np.int64),
        "iqn_episode_global_step": np.concatenate([by_seed[s][0] for s in order]).astype(np.int32),
        "iqn_episode_return": np.concatenate([by_seed[s][1] for s in order]).astype(np.float32),
        "iqn_last_tenth_mean": np.array([last_tenth(by_seed[s][1]) for s in order], np.float64),
    }
    np.savez_compressed(out_path, **out)
    lt = out["iqn_last_tenth_mean"]
    print("last-tenth means: mean %.2f, seed-to-seed sd %.2f -> %s (%.0f KB)" % (lt.mean(), lt.std(ddof=1), out_path, os.path.getsize(out_path) / 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEEP_RL_REFERENCE"), help="directory that holds deep_rl/iqn.py")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--seeds", type=int, default=50)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=1, help="seed of the trace run")
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit("pass --reference DIR or set DEEP_RL_REFERENCE")
    if args.learning:
        return capture_learning(args.reference, args.out or os.path.join(GOLD, "iqn_learning_stats.npz"), args.seeds, args.jobs)
    if args.time_only:
        seed, steps, rets, wall = _run_one((args.reference, 1))
        print('{"reference_iqn_cartpole_cpu_1core": {"env_steps": %d, "episodes": %d, "wall_s": %.2f, "env_steps_per_s": %.0f, "last_tenth": %.2f}}' % (
            RETARGET["total_timesteps"], len(steps), wall, RETARGET["total_timesteps"] / wall, last_tenth(rets)))
    else:
        capture_trace(args.reference, args.out or os.path.join(GOLD, "iqn_ref_trace.npz"), args.seed)


if __name__ == "__main__":
    main()
