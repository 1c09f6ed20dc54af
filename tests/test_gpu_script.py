"""The drop-in script: `python -m deep_rl_amd.ppo` keeps the reference's surface (module globals, print format)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _ports import free_port, run_with_port  # noqa: E402


def _run(env_over):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_over)
    code = ("import runpy, json; g = runpy.run_module('deep_rl_amd.ppo', run_name='__main__');"
            "print('GLOBALS', json.dumps({k: (float(g[k]) if isinstance(g[k], float) else g[k]) for k in "
            "['env_id','total_timesteps','num_steps','num_updates','minibatch_size','update_epochs','gamma','gae_lambda',"
            "'learning_rate','clip_coef','ent_coef','vf_coef','max_grad_norm','seed','global_step','num_envs']}));"
            "print('SHAPES', [tuple(g[k].shape) for k in ['observations','values','actions','log_probs','rewards','dones','advantages','returns']]);"
            "print('OBS', tuple(g['observation'].shape), g['observation'].dtype, g['actions'].dtype);"
            "print('LOSS', g['pg_loss'], g['entropy_loss'], g['v_loss'], g['loss'], g['explained_var'])")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def test_reference_shape_run_n1():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _run({"NUM_ENVS": "1", "TOTAL_TIMESTEPS": "3840"})
    lines = [ln for ln in out.splitlines() if ln.startswith("global_step=")]
    assert len(lines) > 50
    assert all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.\d\d", ln) for ln in lines)  # ppo.py:130
    steps = [int(ln.split(",")[0].split("=")[1]) for ln in lines]
    assert steps == sorted(steps) and steps[-1] < 3840
    assert '"num_updates": 30' in out and '"minibatch_size": 32' in out and '"global_step": 3840' in out
    # the reference's own storage shapes (ppo.py:93-98; advantages / returns :144-151): no env axis at one env
    assert "SHAPES [(129, 4), (129,), (129,), (129,), (129,), (129,), (129,), (129,)]" in out
    assert "OBS (4,) torch.float32 torch.int64" in out


def test_vector_run_learns():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _run({"NUM_ENVS": "256", "TOTAL_TIMESTEPS": str(256 * 128 * 40)})
    rets = [float(ln.split("mean_episodic_return=")[1]) for ln in out.splitlines() if "mean_episodic_return=" in ln]
    assert len(rets) >= 30 and sum(rets[-5:]) / 5 > 2.0 * sum(rets[:3]) / 3, rets
    assert '"minibatch_size": 8192' in out


def _run_dqn(env_over):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_over)
    code = ("import runpy, json; g = runpy.run_module('deep_rl_amd.dqn', run_name='__main__');"
            "print('GLOBALS', json.dumps({k: g[k] for k in ['env_id','total_timesteps','learning_starts','train_frequency','batch_size',"
            "'gamma','learning_rate','target_network_frequency','seed','global_step','num_envs','memory_size']}));"
            "print('SHAPES', [tuple(g[k].shape) for k in ['observations','actions','rewards','terminated']], g['terminated'].dtype); print('LOSS', g['loss'])")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def test_dqn_script_reference_shape_n1():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _run_dqn({"NUM_ENVS": "1", "TOTAL_TIMESTEPS": "6000"})
    lines = [ln for ln in out.splitlines() if ln.startswith("global_step=")]
    assert len(lines) > 100 and all(re.fullmatch(r"global_step=\d+, episodic_return=\d+\.\d\d", ln) for ln in lines)  # dqn.py:111
    assert '"learning_starts": 600' in out and '"global_step": 6000' in out and '"memory_size": 6001' in out
    assert "SHAPES [(6001, 4), (6001,), (6001,), (6001,)] torch.bool" in out   # dqn.py:73-76


def test_dqn_script_vector_ring_runs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _run_dqn({"NUM_ENVS": "256", "TOTAL_TIMESTEPS": "4000", "MEMORY_SIZE": "512", "BATCH_SIZE": "1024"})
    assert '"memory_size": 512' in out and "SHAPES [(512, 256, 4)" in out
    loss = float(out.split("LOSS")[1].split()[0])
    assert np.isfinite(loss) and loss > 0


def _run_sac(env_over):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_over)
    code = ("import runpy, json; g = runpy.run_module('deep_rl_amd.sac', run_name='__main__');"
            "print('GLOBALS', json.dumps({k: g[k] for k in ['env_id','total_timesteps','learning_starts','policy_frequency','batch_size',"
            "'target_network_frequency','gamma','tau','policy_lr','q_lr','alpha_lr','seed','global_step','num_envs','memory_size','target_entropy','alpha']}));"
            "print('SHAPES', [tuple(g[k].shape) for k in ['observations','actions','rewards','terminated']]);"
            "print('STEPS', g['q_optimizer'].step_count, g['actor_optimizer'].step_count, g['engine'].alpha_steps)")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def test_sac_script_reference_shape_n1():
    """sac.py's surface at the reference's own shape (one env): globals, storage shapes, print format, update counts."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _run_sac({"NUM_ENVS": "1", "TOTAL_TIMESTEPS": "3000"})
    lines = [ln for ln in out.splitlines() if ln.startswith("global_step=")]
    assert len(lines) == 15 and all(re.fullmatch(r"global_step=\d+, episodic_return=-\d+\.\d\d", ln) for ln in lines)  # sac.py:161
    assert [int(ln.split(",")[0].split("=")[1]) for ln in lines] == list(range(200, 3001, 200))
    assert '"env_id": "Pendulum-v1"' in out and '"learning_starts": 500' in out and '"global_step": 3000' in out and '"memory_size": 3001' in out
    assert '"target_entropy": -1.0' in out and '"batch_size": 256' in out
    assert "SHAPES [(3001, 3), (3001, 1), (3001,), (3001,)]" in out   # sac.py:126-129 (actions keep the action axis)
    assert "STEPS 2501 2502 2502" in out    # one critic update per step from learning_starts on; 2 actor + 2 alpha updates every 2nd step
    alpha = float(out.split('"alpha": ')[1].split("}")[0])
    assert 0.0 < alpha < 1.0


def test_sac_script_vector_ring_runs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _run_sac({"NUM_ENVS": "2048", "TOTAL_TIMESTEPS": "600", "MEMORY_SIZE": "128", "BATCH_SIZE": "1024", "LEARNING_STARTS": "50"})
    assert '"memory_size": 128' in out and "SHAPES [(128, 2048, 3)" in out and "STEPS 551 552 552" in out


def test_bench_contract_line():
    """bench.py prints ONE JSON line with the driver's keys, the roofline of the dominant kernel (duration measured live with HIP events)
    and the CPU baseline (a bounded sample; shortened here through the same code path)."""
    import json
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full"], env=dict(os.environ, PYTHONPATH=ROOT, MIRL_CPU_BASELINE_SECONDS="1"),
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32"
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 3 * 128 * 4096 / (3 * d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0.3 < r["frac"] < 1.0 and r["launches"] == 16 and "every 10-th update" in r["sampling"]   # 3 timed updates: the launches of the first one are bracketed
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert "static" in r["traffic_source"]                        # roofline.traffic comes from committed PMC passes, and the line says so
    w = d["timed_windows"]                                        # the headline window + two repeats of it, so a sub-per-cent margin can be told from noise
    assert w["count"] == 3 and len(w["ms_per_step"]) == 3 and w["ms_per_step"][0] == d["ms_per_step"] and w["min"] <= w["median"] <= w["max"]
    sr = d["sharded_route"]                                       # the launches only a multi-GPU run takes, timed on this GPU (hook + real one-rank RCCL)
    assert "error" not in sr and "error" not in sr["rccl_world1"], sr
    assert sr["assume_sharded"]["ms_per_step"] > 0 and sr["rccl_world1"]["ms_per_step"] > 0 and "delta_us_per_optimizer_step" in sr["assume_sharded"]
    ps = sr["p2p_synthetic"]                                      # the P2P carrier's one-launch exchange with 2 / 4 / 8 synthetic ranks (round 5)
    for w in (2, 4, 8):
        assert "error" not in ps["world%d" % w], ps
        assert ps["world%d" % w]["ms_per_step"] > 0 and ps["world%d" % w]["back_to_back_us_per_allreduce"] > 0
    m = d["methodology"]                                          # rounds 1-3 and rounds 4+ measured differently: both figures live in one line
    assert m["prewarm_updates"] == 60 and m["protocol_changed_in"].startswith("r04") and m["ms_per_step_all_launches_bracketed"] > 0
    kd = d["kernel_device_ms_per_update"]                         # device durations + span + gaps of ONE profiled run: they add up (weak #8)
    assert "error" not in kd and abs(kd["sum_ms"] + kd["launch_gaps_ms"] - kd["span_ms_profiled"]) < 1e-3 and "static" in kd["source"]
    assert "kernel_ms_per_update" not in d and "note" in d["kernel_ms_per_update_bracketed"]
    vr = d["variant_bf16x3"]["roofline"]                          # the opt-in mode's own roofline against the BF16 matrix peak, executed and algorithmic
    assert vr["peak"] == 2516.8 and 0 < vr["frac_algorithmic"] < vr["frac"] < 1 and "error_bound" in d["variant_bf16x3"]
    n1 = d["cpu_baseline_n1"]                                     # the oracle at the reference's own shape (1 env, 1 thread)
    assert n1["cores"] == 1 and n1["value"] > 0 and n1["reference_python_env_steps_per_s"] == 886.0
    for key, kern in (("config3_dqn", "dqn_act4_kernel"), ("config4_sac", "sac_critic_kernel")):   # BASELINE configs[2] / [3] ride on the same line
        x = d[key]
        assert x["unit"] == "env-steps/s" and x["value"] > 0 and x["ms_per_step"] > 0 and x["dtype"] == "f32"
        assert x["roofline"]["kernel"] == kern and 0 < x["roofline"]["frac"] < 1 and x["roofline"]["avg_launch_us"] > 0
        assert x["cpu_baseline"]["kind"] == "port" and x["cpu_baseline"]["value"] > 0
        # the latency-bound configs are measured against their dependent-chain floor, and carry the sharded form's cost on 8 synthetic ranks
        assert 5 < x["chain_floor_us"] < 1e3 * x["ms_per_step"] and abs(x["frac_of_chain_floor"] - x["chain_floor_us"] / (1e3 * x["ms_per_step"])) < 1e-3
        # (a ratio of two ~10 ms timed loops: one of them catching a clock dip moves it by 10 % — a run on this pool measured 1.07 — so the bound only says "a plausible ratio")
        assert "error" not in x["sharded_synthetic"] and 0.3 < x["sharded_synthetic"]["efficiency_model"] < 1.5, x["sharded_synthetic"]
    for key in ("config3_dueling", "config3_per"):
        assert d[key]["ms_per_step"] > 0 and 0.2 < d[key]["frac_of_chain_floor"] < 1.0, d[key]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run (no --full) times the headline window only and prints the same contract keys; --dump-outputs writes the last timed update's outputs as
    float .npy files (<= 64 MB), and two runs with the same arguments write the same arrays."""
    import json
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    lines, dirs = [], []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", d], env=dict(os.environ, PYTHONPATH=ROOT),
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        assert len(out.stdout.splitlines()) == 1, out.stdout[-2000:]
        lines.append(json.loads(out.stdout))
        dirs.append(d)
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["params_finite"] is True
    assert abs(d["value"] - 3 * 128 * 4096 / (3 * d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    assert d["timed_windows"]["count"] == 1 and d["timed_windows"]["ms_per_step"][0] == d["ms_per_step"]
    for k in ("cpu_baseline", "cpu_baseline_n1", "config3_dqn", "config4_sac", "variant_bf16x3", "sharded_route", "kernel_ms_per_update_bracketed"):
        assert k not in d, k                                      # --full only
    names = sorted(f for f in os.listdir(dirs[0]) if f.endswith(".npy"))
    assert names == sorted(os.listdir(dirs[1])) and "params.npy" in names and "observations.npy" in names
    total = 0
    for f in names:
        a, b = np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f))
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape, f
        assert np.array_equal(a, b, equal_nan=True), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(dirs[0], "params.npy")).shape == (9155,) and np.load(os.path.join(dirs[0], "observations.npy")).shape == (129, 4096, 4)


@pytest.mark.parametrize("mirl_comm", [None, "rccl"])
def test_bench_two_ranks_code_path_on_one_gpu(mirl_comm):
    """`python bench.py --gpus 2` as the driver types it: the parent (no GPU call, no torch import) starts the two ranks through torch.distributed.run as a
    CHILD process, relays rank 0's one JSON line and returns the child's code.  Both ranks on cuda:0 over gloo here — RCCL on
    2..8 GPUs is the driver's run (tests/test_gpu_multigpu.py covers it when >= 2 GPUs are visible).
    MIRL_COMM unset: bench.py's N > 1 policy — the headline runs on RCCL when RCCL can carry the run, and says so when it cannot: here (gloo, both ranks on one device)
    both carriers are probed, RCCL is impossible, the HEADLINE runs the one-call route on the P2P carrier and config.collectives names the reason;
    MIRL_COMM=rccl forced by the caller: under gloo the host-sequenced route."""
    import json
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = dict(os.environ, PYTHONPATH=ROOT, MIRL_BENCH_BACKEND="gloo", MIRL_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("MIRL_COMM", None)
    if mirl_comm:
        env["MIRL_COMM"] = mirl_comm
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"], env=env, capture_output=True, text=True,
                         timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), out.stdout[-2000:]     # exactly one line on stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "cpu_baseline" not in d and d["params_finite"] is True
    assert abs(d["value"] - 2 * 2 * 128 * 4096 / (2 * d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]      # whole-job aggregate over both ranks
    assert "x2" in d["config"]["parallelism"] and d["roofline"]["launches"] == 16
    c = d["collectives"]
    assert c["per_update"] == 17 and c["world_size"] == 2 and c["grad_allreduce"]["bytes"] == 4 * 9159
    assert c["back_to_back"]["us_per_allreduce_grad"] > 0 and c["back_to_back"]["us_per_allreduce_stats"] > 0
    ch = c["carrier_choice"]
    if mirl_comm is None:
        assert ch["MIRL_COMM"] is None and ch["headline_carrier"] == "p2p" and ch["policy"].startswith("RCCL when"), ch
        assert ch["probes"]["p2p"]["ok"] is True and ch["probes"]["p2p"]["us_per_allreduce"] > 0 and ch["probes"]["rccl"]["ok"] is False, ch
        assert c["carrier"].startswith("P2P") and c["headline_exchange"]["replicas_identical"] is True
        assert d["config"]["collectives"].startswith("P2P") and "NOT the RCCL configuration" in d["config"]["collectives"] and "gloo" in d["config"]["collectives"]
        assert "value_p2p" not in d and "rccl_version" not in c or c["rccl_version"] == 0    # P2P carried the headline itself: nothing "beside" it, no RCCL communicator to report
    else:
        assert ch["MIRL_COMM"] == "rccl" and ch["headline_carrier"] is None and "set by the caller" in ch["policy"], ch
        assert "gloo" in c["carrier"] and "host-sequenced" in d["config"]["collectives"] and "NOT the RCCL configuration" in d["config"]["collectives"]
    # the per-carrier legs (round 5): RCCL cannot exist under gloo / two ranks on one device; the P2P carrier runs the ONE-CALL route with both ranks on cuda:0
    k = c["carriers"]
    assert "error" in k["rccl"] and "error" not in k["p2p"], k
    assert k["p2p"]["ms_per_step"] > 0 and k["p2p"]["replicas_identical"] is True and k["p2p"]["in_update"]["samples"] == [0, 2, 32]   # no all-reduce launch per step: the exchange rides in the 32 slab sums
    assert k["p2p"]["back_to_back_us_per_allreduce_grad"] > 0


def test_bench_native_rccl_diagnostics_at_world_size_1():
    """The `collectives` object of an RCCL run (libmirl's own communicator: version, rank count, in-update HIP-event times, back-to-back latencies) — the branch the
    first multi-GPU run of the driver takes — exercised on the one-GPU box: MIRL_FORCE_PG=1 makes the single process join a world_size-1 RCCL group."""
    import json
    import socket
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = run_with_port(lambda port: ([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--headline-only", "--no-cpu-baseline", "--full"],
                                      dict(os.environ, PYTHONPATH=ROOT, MIRL_FORCE_PG="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                                           HSA_ENABLE_IPC_MODE_LEGACY="0")), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    c = d["collectives"]
    assert "error" not in c, c
    assert "RCCL direct" in c["carrier"] and c["rccl_version"] > 0 and c["rccl_comm_count"] == 1 and c["world_size"] == 1
    assert c["back_to_back"]["us_per_allreduce_grad"] > 0 and c["back_to_back"]["us_per_allreduce_stats"] > 0 and "in_update" in c
    k = c["carriers"]                                             # both carriers at world_size 1 (a one-rank P2P communicator needs no peer)
    for which in ("rccl", "p2p"):
        assert "error" not in k[which] and k[which]["ms_per_step"] > 0 and k[which]["replicas_identical"] is True, k
    ch = c["carrier_choice"]
    assert ch["headline_carrier"] == "rccl" and ch["probes"]["rccl"]["ok"] is True and ch["probes"]["p2p"]["ok"] is True and ch["measured"] is None, ch
    # the headline policy: RCCL carries `value`, the P2P carrier stands beside it as first-class keys from its own three windows
    assert d["config"]["collectives"].startswith("RCCL direct") and "value_p2p" in d["config"]["collectives"]
    assert d["value_p2p"] > 0 and d["ms_per_step_p2p"] > 0 and d["timed_windows_p2p"]["count"] == 3 and d["replicas_identical_p2p"] is True
    assert d["best_carrier"] in ("rccl", "p2p") and d["value_best_carrier"] == (d["value_p2p"] if d["best_carrier"] == "p2p" else d["value"])


def test_bench_started_as_ranks_by_torch_distributed_run():
    """The way the DRIVER starts an N > 1 run: `python -m torch.distributed.run ... bench.py --gpus 2` — bench.py is a rank from its first line (WORLD_SIZE set, no
    self-launch), and nobody exported HSA_ENABLE_IPC_MODE_LEGACY for it: deep_rl_amd/dist.py sets it at import, before HIP exists in the process (VERDICT r05 weak #5;
    without it hipIpcGetMemHandle fails on this pool and no P2P communicator can be created).  Two ranks on cuda:0 over gloo; the line carries the policy's keys."""
    import json
    import socket
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = dict(os.environ, PYTHONPATH=ROOT, MIRL_BENCH_BACKEND="gloo", MIRL_BENCH_ONE_GPU="1", OMP_NUM_THREADS="1", MIRL_BENCH_CARRIER_LEGS="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MIRL_COMM", "HSA_ENABLE_IPC_MODE_LEGACY"):
        env.pop(k, None)
    out = run_with_port(lambda port: ([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                                       os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--headline-only", "--full"], env), capture_output=True, text=True,
                        timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    c = d["collectives"]
    ch = c["carrier_choice"]
    assert d["n_gpus"] == 2 and ch["headline_carrier"] == "p2p" and ch["probes"]["p2p"]["ok"] is True and ch["probes"]["rccl"]["ok"] is False, ch
    assert c["headline_exchange"]["replicas_identical"] is True and "NOT the RCCL configuration" in d["config"]["collectives"]


def test_bench_auto_carrier_tunes_on_real_updates_at_world_size_1():
    """MIRL_COMM=auto where BOTH carriers exist (a world_size-1 RCCL group; P2P needs no peer): the library's probe (known answer + stand-alone timing) passes both, then
    bench.py times the same window of real sharded updates of the throwaway prewarm engine on each and the faster one carries the headline's engine — the branch an
    8-GPU run of the driver takes (there with seven peers behind every exchange)."""
    import json
    import socket
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = run_with_port(lambda port: ([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--headline-only", "--no-cpu-baseline", "--full"],
                                      dict(os.environ, PYTHONPATH=ROOT, MIRL_FORCE_PG="1", MIRL_COMM="auto", MIRL_BENCH_CARRIER_LEGS="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                                           RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][0])
    ch = d["collectives"]["carrier_choice"]
    m = ch["measured"]
    assert ch["MIRL_COMM"] == "auto" and ch["headline_carrier"] == m["chosen"] and m["p2p"]["ok"] is True and m["rccl"]["ok"] is True and m["p2p"]["us_per_allreduce"] > 0 and m["rccl"]["us_per_allreduce"] > 0, ch
    t = m["chosen_by"]["ms_per_update"]
    assert t["p2p"] > 0 and t["rccl"] > 0 and m["chosen"] == min(t, key=t.get) and m["chosen_by_probe"] in ("p2p", "rccl"), ch
    assert ("P2P" if m["chosen"] == "p2p" else "RCCL direct") in d["collectives"]["carrier"]


def test_bench_self_launch_propagates_failure():
    """The self-launching parent exits with the child's return code (here: every rank fails in init_process_group on an unknown backend) and prints no JSON line."""
    env = dict(os.environ, PYTHONPATH=ROOT, MIRL_BENCH_BACKEND="no-such-backend")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode != 0 and out.stdout.strip() == "", (out.returncode, out.stdout[-500:])


def test_two_gpus_bench_headline_runs_on_rccl_with_p2p_beside_it():
    """The first contact with a multi-GPU node: `python bench.py --gpus 2` as the driver types it, one rank per GPU over RCCL.  `value` /
    `config.collectives` must be the RCCL configuration BASELINE.json names, the P2P carrier must stand beside it with its own windows and intact replicas, and the
    top-level RCCL facts must come from a communicator that saw both ranks.  Skips below 2 GPUs (the one-GPU box exercises the same keys through MIRL_FORCE_PG=1)."""
    import json
    import torch

    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MIRL_COMM", "MIRL_BENCH_BACKEND", "MIRL_BENCH_ONE_GPU"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--headline-only", "--full"], env=env, capture_output=True,
                         text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), out.stdout[-2000:]
    d = json.loads(lines[0])
    c = d["collectives"]
    ch = c["carrier_choice"]
    assert d["n_gpus"] == 2 and ch["headline_carrier"] == "rccl" and ch["probes"]["rccl"]["ok"] is True, ch
    assert d["config"]["collectives"].startswith("RCCL direct") and c["rccl_version"] > 0 and c["rccl_comm_count"] == 2
    assert c["headline_exchange"]["replicas_identical"] is True
    if ch["probes"]["p2p"]["ok"]:   # hipIpc across the two devices worked: the second carrier is measured beside the headline, never instead of it
        assert d["value_p2p"] > 0 and d["timed_windows_p2p"]["count"] == 3 and d["replicas_identical_p2p"] is True and d["best_carrier"] in ("rccl", "p2p")
    else:
        assert "value_p2p" not in d and ch["probes"]["p2p"].get("why")
