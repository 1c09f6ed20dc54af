"""ActorCritic with the reference's constructor, initialisation and method surface (ppo.py:25-59), whose
parameters are views into ONE flat fp32 device buffer — the layout the HIP kernels consume."""
import numpy as np
import torch
from torch import nn
from torch.distributions import Categorical

from . import _native as N


def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
    """ppo.py:25-28."""
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class ActorCritic(nn.Module):
    """actor 4->64->64->n_actions, critic 4->64->64->1, tanh (ppo.py:31-47).

    Construction happens on the CPU in the reference's layer order so that ``torch.manual_seed(s)`` yields the
    reference's initial weights; the 12 parameter tensors are then re-pointed at slices of ``self.flat``
    (order of ``agent.parameters()`` == include/mi_rl.h "Parameter layout").
    """

    def __init__(self, env, device=None):
        super().__init__()
        obs_dim = int(np.array(env.observation_space.shape).prod())
        n_act = env.action_space.n
        if obs_dim != 4 or n_act != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2); got %d/%d" % (obs_dim, n_act))
        self.actor = nn.Sequential(
            layer_init(nn.Linear(obs_dim, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, n_act), std=0.01),
        )
        self.critic = nn.Sequential(
            layer_init(nn.Linear(obs_dim, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, 1), std=1.0),
        )
        dev = torch.device(device if device is not None else getattr(env, "device", "cuda"))
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in self.parameters()]).to(dev, torch.float32).contiguous()
        assert flat.numel() == N.NPARAMS
        self.flat = flat
        off = 0
        for p in self.parameters():
            n = p.numel()
            p.data = flat[off:off + n].view(p.shape)
            off += n
        self.device = dev

    # -- helpers -------------------------------------------------------------------------------
    def load_flat(self, vec):
        """Overwrite all parameters from a flat vector (numpy or tensor) in parameters() order."""
        self.flat.copy_(torch.as_tensor(vec, dtype=torch.float32).reshape(-1).to(self.device))

    def _forward(self, observation, want_logits, want_value):
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        n = obs.shape[0]
        logits = torch.empty((n, 2), dtype=torch.float32, device=self.device) if want_logits else None
        value = torch.empty(n, dtype=torch.float32, device=self.device) if want_value else None
        N.check(N.lib().mi_ppo_forward(N.ptr(self.flat), N.ptr(obs), n, N.ptr(logits), N.ptr(value), N.stream_ptr(self.device)),
                "mi_ppo_forward")
        return (logits.reshape(*lead, 2) if want_logits else None), (value.reshape(lead) if want_value else None)

    # -- reference surface (inference; training gradients come from mi_ppo_minibatch_grad) ----------------
    def get_value(self, observation):
        """ppo.py:49-50."""
        return self._forward(observation, False, True)[1]

    def get_action_distribution(self, observation):
        """ppo.py:52-54."""
        return Categorical(logits=self._forward(observation, True, False)[0])

    def get_action(self, observation):
        """ppo.py:56-59."""
        distribution = self.get_action_distribution(observation)
        action = distribution.sample()
        return action, distribution.log_prob(action)


class QNetwork(nn.Module):
    """QNetwork of the reference dqn.py:24-36 (4 -> 120 -> 84 -> n_actions, ReLU, torch default init) whose 6 parameter
    tensors are views into one flat fp32 device buffer (include/mi_rl.h "DQN")."""

    def __init__(self, env, device=None):
        super().__init__()
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or env.action_space.n != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        self.network = nn.Sequential(nn.Linear(obs_dim, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU(), nn.Linear(84, env.action_space.n))
        dev = torch.device(device if device is not None else getattr(env, "device", "cuda"))
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in self.parameters()]).to(dev, torch.float32).contiguous()
        assert flat.numel() == N.DQN_NPARAMS
        self.flat = flat
        off = 0
        for p in self.parameters():
            n = p.numel()
            p.data = flat[off:off + n].view(p.shape)
            off += n
        self.device = dev

    def load_flat(self, vec):
        self.flat.copy_(torch.as_tensor(vec, dtype=torch.float32).reshape(-1).to(self.device))

    def load_state_dict(self, state_dict, *a, **kw):
        """target_network.load_state_dict(q_network.state_dict()) (dqn.py:70,137): keeps the flat-buffer views intact."""
        own = dict(self.named_parameters())
        with torch.no_grad():
            for k, v in state_dict.items():
                own[k].copy_(v)

    def forward(self, observation):
        """dqn.py:35-36."""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        N.check(N.lib().mi_dqn_forward(N.ptr(self.flat), N.ptr(obs), obs.shape[0], N.ptr(q), N.stream_ptr(self.device)), "mi_dqn_forward")
        return q.reshape(*lead, 2)


def _bind_flat(module, flat):
    """Re-point every parameter of `module` at its slice of `flat` (parameters() order)."""
    off = 0
    for p in module.parameters():
        n = p.numel()
        p.data = flat[off:off + n].view(p.shape)
        off += n
    assert off == flat.numel()
    module.flat = flat


class _FlatModule(nn.Module):
    def _finish(self, env, device, nparams):
        dev = torch.device(device if device is not None else getattr(env, "device", "cuda"))
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in self.parameters()]).to(dev, torch.float32).contiguous()
        assert flat.numel() == nparams
        _bind_flat(self, flat)
        self.device = dev

    def load_flat(self, vec):
        self.flat.copy_(torch.as_tensor(vec, dtype=torch.float32).reshape(-1).to(self.device))

    def load_state_dict(self, state_dict, *a, **kw):
        """qf1_target.load_state_dict(qf1.state_dict()) (sac.py:115-116): keeps the flat-buffer views intact."""
        own = dict(self.named_parameters())
        with torch.no_grad():
            for k, v in state_dict.items():
                if k in own:
                    own[k].copy_(v)


def pack(*modules):
    """Lay the flat buffers of several modules back to back in ONE buffer (the twin critics share one Adam, sac.py:117) and
    re-point their parameters; returns the joint buffer."""
    joint = torch.cat([m.flat for m in modules]).contiguous()
    off = 0
    for m in modules:
        n = m.flat.numel()
        _bind_flat(m, joint[off:off + n])
        off += n
    return joint


class SoftQNetwork(_FlatModule):
    """SoftQNetwork of the reference sac.py:29-43 (cat(obs, action) -> 256 -> 256 -> 1, ReLU, torch default init)."""

    def __init__(self, env, device=None):
        super().__init__()
        obs_dim, act_dim = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))
        if obs_dim != 3 or act_dim != 1:
            raise N.MiError("the SAC kernels are specialised for Pendulum (obs 3, action 1); got %d/%d" % (obs_dim, act_dim))
        self.network = nn.Sequential(nn.Linear(obs_dim + act_dim, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 1))
        self._finish(env, device, N.SAC_Q_NPARAMS)

    def forward(self, observation, action):
        """sac.py:40-43."""
        obs = observation.to(self.device, torch.float32).reshape(-1, 3).contiguous()
        act = action.to(self.device, torch.float32).reshape(-1).contiguous()
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        N.check(N.lib().mi_sac_q_forward(N.ptr(self.flat), N.ptr(obs), N.ptr(act), obs.shape[0], N.ptr(out), N.stream_ptr(self.device)), "mi_sac_q_forward")
        return out


class Actor(_FlatModule):
    """Actor of the reference sac.py:46-78 (3 -> 256 -> 256 ReLU, mean head, tanh-bounded log-std head, tanh-squashed action)."""

    def __init__(self, env, device=None):
        super().__init__()
        obs_dim, act_dim = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))
        if obs_dim != 3 or act_dim != 1:
            raise N.MiError("the SAC kernels are specialised for Pendulum (obs 3, action 1); got %d/%d" % (obs_dim, act_dim))
        self.shared_net = nn.Sequential(nn.Linear(obs_dim, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU())
        self.mean_net = nn.Linear(256, act_dim)
        self.log_std_net = nn.Sequential(nn.Linear(256, act_dim), nn.Tanh())
        hi, lo = np.asarray(env.action_space.high, np.float32), np.asarray(env.action_space.low, np.float32)
        self.register_buffer("action_scale", torch.tensor((hi - lo) / 2.0, dtype=torch.float32))
        self.register_buffer("action_bias", torch.tensor((hi + lo) / 2.0, dtype=torch.float32))
        if float(self.action_scale) != 2.0 or float(self.action_bias) != 0.0:
            raise N.MiError("the SAC kernels are specialised for Pendulum's action range [-2, 2]")
        self._finish(env, device, N.SAC_ACTOR_NPARAMS)

    def get_action(self, observation, eps=None):
        """sac.py:65-78.  eps: the standard-normal draws of rsample() (default: torch.randn on the device)."""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 3).contiguous()
        n = obs.shape[0]
        e = torch.randn(n, device=self.device) if eps is None else eps.to(self.device, torch.float32).reshape(-1).contiguous()
        action = torch.empty(n, dtype=torch.float32, device=self.device)
        logp = torch.empty(n, dtype=torch.float32, device=self.device)
        N.check(N.lib().mi_sac_actor_sample(N.ptr(self.flat), N.ptr(obs), N.ptr(e), n, N.ptr(action), N.ptr(logp), N.stream_ptr(self.device)),
                "mi_sac_actor_sample")
        return action.reshape(*lead, 1), logp.reshape(lead)


class DuelingQNetwork(_FlatModule):
    """QNetwork of the reference dueling_dqn.py:24-40 (features 4 -> 120 -> 84 ReLU, value stream 84 -> 1, advantage stream 84 -> n,
    values + (advantages - mean advantages)); attribute names as in the reference (incl. its `feauture_layer` spelling).
    `flat` holds the dueling parameters; `eff` the equivalent plain-DQN vector the kernels consume (refresh with `repack()`)."""

    def __init__(self, env, device=None):
        super().__init__()
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or env.action_space.n != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        self.feauture_layer = nn.Sequential(nn.Linear(obs_dim, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU())
        self.value_stream = nn.Linear(84, 1)
        self.advantage_stream = nn.Linear(84, env.action_space.n)
        self._finish(env, device, N.DUELING_NPARAMS)
        self.eff = torch.empty(N.DQN_NPARAMS, dtype=torch.float32, device=self.device)
        self.repack()

    def repack(self):
        """refresh the plain-DQN image of the parameters (after an optimizer step / load_state_dict)"""
        N.check(N.lib().mi_dueling_pack(N.ptr(self.flat), N.ptr(self.eff), N.stream_ptr(self.device)), "mi_dueling_pack")

    def load_flat(self, vec):
        super().load_flat(vec)
        self.repack()

    def load_state_dict(self, state_dict, *a, **kw):
        super().load_state_dict(state_dict, *a, **kw)
        self.repack()

    def forward(self, observation):
        """dueling_dqn.py:36-40."""
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        N.check(N.lib().mi_dqn_forward(N.ptr(self.eff), N.ptr(obs), obs.shape[0], N.ptr(q), N.stream_ptr(self.device)), "mi_dqn_forward")
        return q.reshape(*lead, 2)


class DropoutPolicy(_FlatModule):
    """The policy of the reference reinforce.py:40-46 (4 -> 128, Dropout(p=0.6), ReLU, 128 -> 2, Softmax; torch default init) over one flat fp32 device
    buffer of 898 floats (include/mi_reinforce.h: W1 128x4, b1 128, W2 2x128, b2 2 — the order of ``agent.parameters()``).  The layer list is the
    reference's, so ``torch.manual_seed(s)`` before construction gives its initial weights.  Acting with live dropout, as the reference does (it never
    calls ``.eval()``), happens inside ReinforceEngine's episode kernel with a keyed mask stream; ``forward`` here evaluates given rows."""

    def __init__(self, env, device=None):
        super().__init__()
        from . import _native_pg as PG
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or env.action_space.n != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        self.network = nn.Sequential(nn.Linear(obs_dim, 128), nn.Dropout(p=0.6), nn.ReLU(), nn.Linear(128, env.action_space.n), nn.Softmax(-1))
        self._finish(env, device, PG.NPARAMS)

    def forward(self, observation, mask_bits=None):
        """-> action probabilities.  mask_bits (rows, 4) int32 / uint32: the 128 keep bits of each row (training mode); None: eval mode (no dropout)."""
        from . import _native_pg as PG
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        mb = None if mask_bits is None else mask_bits.to(self.device).reshape(-1, 4).contiguous()
        probs = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        PG.check(PG.lib().mi_pg_forward(N.ptr(self.flat), N.ptr(obs), obs.shape[0], N.ptr(mb), N.ptr(probs), N.stream_ptr(self.device)), "mi_pg_forward")
        return probs.reshape(*lead, 2)


class C51QNetwork(_FlatModule):
    """QNetwork of the reference c51.py:24-37 (4 -> 120 -> 84 -> n_actions * n_atoms, ReLU, Unflatten, torch default init) over one flat fp32 device buffer of
    27,934 floats (include/mi_c51.h).  The layer list is the reference's, so ``torch.manual_seed(s)`` before construction gives its initial weights.  The kernels
    are specialised for CartPole and the reference's 101 atoms on [-100, 100]."""

    def __init__(self, env, n_atoms=101, device=None):
        super().__init__()
        from . import _native_c51 as K
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or getattr(env.action_space, "n", None) != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        if int(n_atoms) != K.N_ATOMS:
            raise N.MiError("the C51 kernels are specialised for n_atoms = %d (v_min = -100, v_max = 100); got %r" % (K.N_ATOMS, n_atoms))
        self.network = nn.Sequential(nn.Linear(obs_dim, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU(), nn.Linear(84, env.action_space.n * n_atoms),
                                     nn.Unflatten(-1, (env.action_space.n, n_atoms)))
        self.n_atoms = int(n_atoms)
        self._finish(env, device, K.NPARAMS)

    def _run(self, observation, want_probs, want_q):
        from . import _native_c51 as K
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        n = obs.shape[0]
        probs = torch.empty((n, 2, K.N_ATOMS), dtype=torch.float32, device=self.device) if want_probs else None
        q = torch.empty((n, 2), dtype=torch.float32, device=self.device) if want_q else None
        K.check(K.lib().mi_c51_forward(N.ptr(self.flat), N.ptr(obs), n, N.ptr(probs), N.ptr(q), N.stream_ptr(self.device)), "mi_c51_forward")
        return (probs.reshape(*lead, 2, K.N_ATOMS) if want_probs else None), (q.reshape(*lead, 2) if want_q else None)

    def get_probs(self, observation):
        """c51.py:36-37."""
        return self._run(observation, True, False)[0]

    def get_q_values(self, observation):
        """torch.sum(get_probs(observation) * atoms, dim=-1) (c51.py:99) in the kernels' summation order."""
        return self._run(observation, False, True)[1]


class QRQNetwork(_FlatModule):
    """The QR-DQN network (4 -> 120 -> 84 -> n_actions * n_quantiles, ReLU, Unflatten, torch default init) over one flat fp32 device buffer of 21,644 floats
    (include/mi_qr.h).  The layer list is the plain ``nn.Sequential``'s, so ``torch.manual_seed(s)`` before construction gives its initial weights bit for bit.
    The kernels are specialised for CartPole and 64 quantiles."""

    def __init__(self, env, n_quantiles=64, device=None):
        super().__init__()
        from . import _native_qr as K
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or getattr(env.action_space, "n", None) != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        if int(n_quantiles) != K.N_QUANT:
            raise N.MiError("the QR-DQN kernels are specialised for n_quantiles = %d; got %r" % (K.N_QUANT, n_quantiles))
        self.network = nn.Sequential(nn.Linear(obs_dim, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU(), nn.Linear(84, env.action_space.n * n_quantiles),
                                     nn.Unflatten(-1, (env.action_space.n, n_quantiles)))
        self.n_quantiles = int(n_quantiles)
        self._finish(env, device, K.NPARAMS)

    def _run(self, observation, want_quantiles, want_q):
        from . import _native_qr as K
        obs = observation.to(self.device, torch.float32)
        lead = obs.shape[:-1]
        obs = obs.reshape(-1, 4).contiguous()
        n = obs.shape[0]
        quant = torch.empty((n, 2, K.N_QUANT), dtype=torch.float32, device=self.device) if want_quantiles else None
        q = torch.empty((n, 2), dtype=torch.float32, device=self.device) if want_q else None
        K.check(K.lib().mi_qr_forward(N.ptr(self.flat), N.ptr(obs), n, N.ptr(quant), N.ptr(q), N.stream_ptr(self.device)), "mi_qr_forward")
        return (quant.reshape(*lead, 2, K.N_QUANT) if want_quantiles else None), (q.reshape(*lead, 2) if want_q else None)

    def get_quantiles(self, observation):
        """The 64 quantiles of both actions: [..., 2, 64]."""
        return self._run(observation, True, False)[0]

    def get_q_values(self, observation):
        """The mean of the quantiles, through the collapsed head (include/mi_qr.h): [..., 2]."""
        return self._run(observation, False, True)[1]


def _cpu_only(module):
    """The single IQN modules have no kernel of their own: the library evaluates the three together (``iqn_forward``, IQNEngine).  Their ``forward`` is for
    inspecting a network on the CPU; on a device it is an error, never a quiet torch evaluation."""
    if module.device.type != "cpu":
        raise N.MiError("%s.forward runs on CPU parameters only; on the device use deep_rl_amd.iqn_forward(pack(...), observation, taus) or IQNEngine" % type(module).__name__)


class FeaturesExtractor(_FlatModule):
    """The IQN features extractor re-targeted to CartPole: the reference's three convolutions at spatial extent 1 x 1 are Linear(4, 32), Linear(32, 64),
    Linear(64, 64), each followed by a ReLU; 6,432 floats (include/mi_iqn.h).  Weights are kaiming-uniform and biases zero, drawn behind torch's default init as
    the reference's ``.apply`` does, so ``torch.manual_seed(s)`` before construction gives its initial values.  The three IQN modules are joined by ``pack`` into the
    one 44,898-float buffer the kernels read."""

    def __init__(self, env, device=None):
        super().__init__()
        from . import _native_iqn as K
        if int(np.prod(env.observation_space.shape)) != 4 or getattr(env.action_space, "n", None) != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        self.net = nn.Sequential(nn.Linear(4, 32), nn.ReLU(), nn.Linear(32, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Flatten())
        for layer in self.net:
            if isinstance(layer, nn.Linear):
                nn.init.kaiming_uniform_(layer.weight)
                nn.init.zeros_(layer.bias)
        self._finish(env, device, K.F_NPARAMS)

    def forward(self, input):
        _cpu_only(self)
        return self.net(input.to(torch.float32))


class CosineEmbeddingNetwork(_FlatModule):
    """relu(W cos(k pi tau) + b), k = 1 .. num_cosines, of taus [batch, n] -> [batch, n, embedding_dim] (torch default init); 4,160 floats."""

    def __init__(self, num_cosines, embedding_dim, device=None):
        super().__init__()
        from . import _native_iqn as K
        if int(num_cosines) != K.NCOS or int(embedding_dim) != K.EMB:
            raise N.MiError("the IQN kernels are specialised for num_cosines = %d and embedding_dim = %d; got %r / %r" % (K.NCOS, K.EMB, num_cosines, embedding_dim))
        self.net = nn.Sequential(nn.Linear(num_cosines, embedding_dim), nn.ReLU())
        self.num_cosines = int(num_cosines)
        self._finish(None, device, K.C_NPARAMS)

    def forward(self, taus):
        _cpu_only(self)
        k_pi = torch.arange(1, self.num_cosines + 1, dtype=torch.float32) * torch.tensor(np.pi, dtype=torch.float32)   # the f32 table of include/mi_iqn.h
        return self.net((taus.to(torch.float32)[..., None] * k_pi).cos())   # Linear acts on the last axis: [batch, n, cosines] -> [batch, n, embedding]


class QuantileNetwork(_FlatModule):
    """(embedding * tau embedding) -> 512 -> num_actions per tau, [batch, n, num_actions] (torch default init); 34,306 floats."""

    def __init__(self, num_actions, embedding_dim, device=None):
        super().__init__()
        from . import _native_iqn as K
        if int(num_actions) != 2 or int(embedding_dim) != K.EMB:
            raise N.MiError("the IQN kernels are specialised for 2 actions and embedding_dim = %d; got %r / %r" % (K.EMB, num_actions, embedding_dim))
        self.net = nn.Sequential(nn.Linear(embedding_dim, K.HID), nn.ReLU(), nn.Linear(K.HID, num_actions))
        self._finish(None, device, K.Q_NPARAMS)

    def forward(self, embeddings, tau_embeddings):
        _cpu_only(self)
        return self.net(embeddings[:, None, :] * tau_embeddings)


def iqn_forward(flat, observation, taus):
    """The three IQN networks in ONE launch (mi_iqn_forward): obs [..., 4], taus [..., K] -> (quantiles [..., K, 2], q [..., 2]) from a packed 44,898-float buffer."""
    from . import _native_iqn as K
    dev = flat.device
    obs = observation.to(dev, torch.float32)
    lead = obs.shape[:-1]
    obs = obs.reshape(-1, 4).contiguous()
    tau = taus.to(dev, torch.float32).reshape(obs.shape[0], -1).contiguous()
    n, k = tau.shape
    quant = torch.empty((n, k, 2), dtype=torch.float32, device=dev)
    q = torch.empty((n, 2), dtype=torch.float32, device=dev)
    K.check(K.lib().mi_iqn_forward(N.ptr(flat), N.ptr(obs), N.ptr(tau), n, k, N.ptr(quant), N.ptr(q), N.stream_ptr(dev)), "mi_iqn_forward")
    return quant.reshape(*lead, k, 2), q.reshape(*lead, 2)


class NoisyLinear(nn.Module):
    """A factorised-Gaussian noisy linear layer (Fortunato et al. 2018, as Rainbow uses it): weight = weight_mu + weight_sigma * eps_w, bias = bias_mu +
    bias_sigma * eps_b.  mu ~ U(+-1 / sqrt(in_features)), sigma = sigma_0 / sqrt(in_features).  The module holds the DISTRIBUTION only; the draws are the
    kernels' (include/mi_noisy.h), and ``forward`` is the mean layer."""

    def __init__(self, in_features, out_features, sigma_0=0.5):
        super().__init__()
        self.in_features, self.out_features, self.sigma_0 = int(in_features), int(out_features), float(sigma_0)
        bound = 1.0 / np.sqrt(self.in_features)
        self.weight_mu = nn.Parameter(torch.empty(self.out_features, self.in_features).uniform_(-bound, bound))
        self.bias_mu = nn.Parameter(torch.empty(self.out_features).uniform_(-bound, bound))
        self.weight_sigma = nn.Parameter(torch.full((self.out_features, self.in_features), self.sigma_0 / np.sqrt(self.in_features)))
        self.bias_sigma = nn.Parameter(torch.full((self.out_features,), self.sigma_0 / np.sqrt(self.in_features)))

    def forward(self, input):
        return nn.functional.linear(input, self.weight_mu, self.bias_mu)


class NoisyDuelingQNetwork(_FlatModule):
    """DuelingQNetwork whose value and advantage streams are ``NoisyLinear``s: 11,274 floats (include/mi_noisy.h).  ``flat`` is DuelingQNetwork's 11,019-float
    vector with the streams' means in the place of their weights, then the 255 sigmas in the same order — all mu, then all sigma — which is NOT the modules'
    registration order, so ``parameters()`` is overridden to give the flat order (what ``_finish``, ``_bind_flat`` and an optimizer walk).  The torso is plain.
    ``forward`` is the mean network on CPU parameters; on the device the values come from NoisyDQNEngine.forward."""

    def __init__(self, env, device=None, sigma_0=0.5):
        super().__init__()
        from . import _native_nz as K
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or env.action_space.n != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        self.feauture_layer = nn.Sequential(nn.Linear(obs_dim, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU())
        self.value_stream = NoisyLinear(84, 1, sigma_0)
        self.advantage_stream = NoisyLinear(84, env.action_space.n, sigma_0)
        self._finish(env, device, K.NPARAMS)

    def parameters(self, recurse=True):
        v, a = self.value_stream, self.advantage_stream
        yield from self.feauture_layer.parameters()
        yield from (v.weight_mu, v.bias_mu, a.weight_mu, a.bias_mu, v.weight_sigma, v.bias_sigma, a.weight_sigma, a.bias_sigma)

    def forward(self, observation):
        _cpu_only(self)
        h = self.feauture_layer(observation.to(torch.float32))
        values, advantages = self.value_stream(h), self.advantage_stream(h)
        return values + (advantages - advantages.mean(dim=-1, keepdim=True))


class RainbowQNetwork(_FlatModule):
    """Rainbow's network: the 4 -> 120 -> 84 torso and two ``NoisyLinear`` streams that produce 51 atoms each — value [51], advantage [2 * 51] — combined by the
    dueling rule per atom and normalised by a softmax per action: 36,774 floats (include/mi_rainbow.h).  ``flat`` is all mu, then all sigma (``parameters()`` is
    overridden to give that order, as NoisyDuelingQNetwork does).  ``forward`` is the MEAN network's action values on CPU parameters under the support
    ``(v_min, v_max)``; on the device the distributions and values come from RainbowEngine.forward."""

    def __init__(self, env, device=None, sigma_0=0.5, n_atoms=51, v_min=0.0, v_max=100.0):
        super().__init__()
        from . import _native_rb as K
        obs_dim = int(np.prod(env.observation_space.shape))
        if obs_dim != 4 or env.action_space.n != 2:
            raise N.MiError("the HIP kernels are specialised for CartPole (obs 4, actions 2)")
        if int(n_atoms) != K.N_ATOMS:
            raise N.MiError("the Rainbow kernels are specialised for n_atoms = %d; got %r" % (K.N_ATOMS, n_atoms))
        self.n_atoms, self.v_min, self.v_max = int(n_atoms), float(v_min), float(v_max)
        self.feauture_layer = nn.Sequential(nn.Linear(obs_dim, 120), nn.ReLU(), nn.Linear(120, 84), nn.ReLU())
        self.value_stream = NoisyLinear(84, self.n_atoms, sigma_0)
        self.advantage_stream = NoisyLinear(84, env.action_space.n * self.n_atoms, sigma_0)
        self._finish(env, device, K.NPARAMS)

    def parameters(self, recurse=True):
        v, a = self.value_stream, self.advantage_stream
        yield from self.feauture_layer.parameters()
        yield from (v.weight_mu, v.bias_mu, a.weight_mu, a.bias_mu, v.weight_sigma, v.bias_sigma, a.weight_sigma, a.bias_sigma)

    def get_probs(self, observation):
        _cpu_only(self)
        h = self.feauture_layer(observation.to(torch.float32))
        values = self.value_stream(h)[..., None, :]
        advantages = self.advantage_stream(h).unflatten(-1, (2, self.n_atoms))
        return torch.softmax(values + (advantages - advantages.mean(dim=-2, keepdim=True)), dim=-1)

    def forward(self, observation):
        atoms = torch.linspace(self.v_min, self.v_max, self.n_atoms)
        return (self.get_probs(observation) * atoms).sum(-1)


class LinearPolicy(_FlatModule):
    """The policy of Augmented Random Search (include/mi_ars.h): M, f32 [n_actions][4] without a bias, over one flat fp32 device buffer of 8 floats; it starts at
    zero, as the paper's does.  The action of an observation is argmax_a (M x)_a with x the normalised observation — ARSEngine holds the normaliser."""

    def __init__(self, env, device=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(env.action_space.n, int(np.prod(env.observation_space.shape))), requires_grad=False)
        self._finish(env, device, 8)
