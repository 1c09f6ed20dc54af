"""Shared helpers of the IQN GPU tests — TEST INFRASTRUCTURE: engines from numpy state, and the record of the device's observed maxima."""
import json
import os

import numpy as np
import torch

import _iqn_ref as R


def make_engine(params, target_params, num_envs=1, slots=64, batch_size=32, seed=1, ringv=None, env_id_base=0, **kw):
    import deep_rl_amd as M
    dev = torch.device("cuda", 0)
    env = M.make("CartPole-v1", num_envs=num_envs, device=dev, env_id_base=env_id_base) if env_id_base else M.make("CartPole-v1", num_envs=num_envs, device=dev)
    env.seed(seed)
    p = torch.from_numpy(np.asarray(params, np.float32).copy()).to(dev)
    tp = torch.from_numpy(np.asarray(target_params, np.float32).copy()).to(dev)
    opt = M.Adam(p, lr=5e-5, eps=1e-2 / batch_size)
    eng = M.IQNEngine(env, p, tp, opt, slots=slots, batch_size=batch_size, **kw)
    if ringv is not None:
        load_ring(eng, ringv)
    return eng


def load_ring(eng, ringv):
    obs, actions, rewards, term = ringv
    eng.observations.copy_(torch.from_numpy(np.ascontiguousarray(obs)))
    eng.actions.copy_(torch.from_numpy(np.ascontiguousarray(actions)))
    eng.rewards.copy_(torch.from_numpy(np.ascontiguousarray(rewards)))
    eng.terminated.copy_(torch.from_numpy(np.ascontiguousarray(term)))


def run_grad(eng, inds, taus, next_taus, tau_dashes):
    eng.sample(inds)
    eng.force_taus(taus, next_taus, tau_dashes)
    eng.grad()
    torch.cuda.synchronize()
    return dict(current=eng.current_action_quantiles.cpu().numpy(), target=eng.target_action_quantiles.cpu().numpy(), next_actions=eng.next_actions.cpu().numpy(),
                grads=eng.grads.cpu().numpy(), loss=float(eng.loss.item()), taus=eng.taus.cpu().numpy())


_MAXIMA = {}


def record(name, value):
    """keep the largest figure seen under `name` and rewrite iqn_gpu_maxima.json in the results directory"""
    _MAXIMA[name] = max(float(value), _MAXIMA.get(name, 0.0))
    path = os.path.join(R.results_dir(), "iqn_gpu_maxima.json")
    old = {}
    if os.path.exists(path):
        try:
            old = json.load(open(path))
        except ValueError:
            old = {}
    old.update({k: max(v, old.get(k, 0.0)) for k, v in _MAXIMA.items()})
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)
    return float(value)
