"""Agent-side drop-in surface: the ``RLAgent`` family of
smartstart/reinforcementLearningCore/agents_abstract_classes.py and GPU-backed counterparts of
``DDPG_Baselines_agent`` (action path) and ``NND_MB_agent`` (the SmartStart navigator).

Constructor keyword names follow the reference classes so existing call sites keep working; the
TensorFlow session argument ``sess`` is accepted and ignored.  Both learners run on the GPU: the DDPG step
(``ssc_ddpg_train``) and the dynamics-model training of the navigator
(``ssc_mlp_train_steps``, rank 3; ``NND_MB_agent.train_dynamics_model``).  Weights stay plain torch tensors
(TensorFlow layout) that a caller may also overwrite through ``set_weights``.
"""
from __future__ import annotations

import abc
import ctypes
import os

import numpy as np
import torch

from . import _ffi, navigator
from .numerical import (distances_left, elliptical_euclidean_distance_function_generator,
                        get_start_waypoints_final_states_steps, path_deltas_stds_and_means_per_dim,
                        path_shortcutter, radii_calc)
from .obs_rms import ObsRms
from .population import DeviceItems, IndexDraw
from .replay_buffer import ReplayBuffer
from .vec_env import ActorPolicy


# --------------------------------------------------------------------------------- ABCs --
class RLAgent(metaclass=abc.ABCMeta):
    """agents_abstract_classes.py:6-53"""

    @abc.abstractmethod
    def get_action(self, state):
        """state -> action appropriate for the environment"""

    @abc.abstractmethod
    def observe(self, state, action, reward, new_state, done):
        """called after every env.step"""

    @abc.abstractmethod
    def render(self, env, **kwargs):
        """render the environment the agent is in"""

    def start_new_episode(self, state):
        pass

    def end_episode(self):
        pass

    def get_param_dict(self):
        raise NotImplementedError("Agent hasn't overridden get_param_dict, if you don't wish to implement it "
                                  "just return None")


class NavigationRLAgent(RLAgent):
    """agents_abstract_classes.py:55-65"""

    def start_new_episode_plan(self, state, path_to_follow):
        raise NotImplementedError


class ValueFuncRLAgent(RLAgent):
    """agents_abstract_classes.py:68-80"""

    @abc.abstractmethod
    def get_state_value(self, state):
        """value of ``state`` (max over actions)"""


class ReplayBufferRLAgent(RLAgent):
    """agents_abstract_classes.py:82-91"""

    def __init__(self):
        self.replay_buffer = None

    def set_replay_buffer_main_agent(self, new_main_agent):
        self.replay_buffer.set_main_agent(new_main_agent)


# --------------------------------------------------------------------------------- DDPG --
class DecayingOrnsteinUhlenbeckActionNoise:
    """DDPG_Baselines_agent.py:52-78 over baselines' OrnsteinUhlenbeckActionNoise [third-party]:
    x <- x + theta (mu - x) dt + sigma sqrt(dt) N(0,1); output x * max(epsilon, 0)."""

    def __init__(self, epsilon, min_epsilon, epsilon_decay_factor, mu, sigma, theta=.15, dt=1e-2, x0=None):
        self.mu, self.sigma, self.theta, self.dt, self.x0 = np.asarray(mu, np.float64), sigma, theta, dt, x0
        self.epsilon, self.min_epsilon, self.epsilon_decay_factor = epsilon, min_epsilon, epsilon_decay_factor
        self.reset()

    def __call__(self):
        x = self.x_prev + self.theta * (self.mu - self.x_prev) * self.dt + \
            self.sigma * np.sqrt(self.dt) * np.random.normal(size=self.mu.shape)
        self.x_prev = x
        return x * max(self.epsilon, 0)

    def reset(self):
        self.x_prev = self.x0 if self.x0 is not None else np.zeros_like(self.mu)

    def reduce_epsilon(self):
        self.epsilon = max(self.epsilon * self.epsilon_decay_factor, self.min_epsilon)


def init_critic_weights(obs_dim, h1, h2, nb_actions, generator=None):
    """Critic_Editted (models_editted.py:78-100): glorot-uniform kernels, zero biases, W2 is
    [h1 + nb_actions, h2] (the action joins after the first ReLU), last layer U(-3e-3, 3e-3)."""
    g = generator

    def glorot(i, o):
        lim = float(np.sqrt(6.0 / (i + o)))
        return (torch.rand((i, o), generator=g) * 2 - 1) * lim
    return dict(W1=glorot(obs_dim, h1), b1=torch.zeros(h1), W2=glorot(h1 + nb_actions, h2), b2=torch.zeros(h2),
                W3=(torch.rand((h2, 1), generator=g) * 2 - 1) * 3e-3, b3=torch.zeros(1))


def init_actor_weights(obs_dim, h1, h2, nb_actions, generator=None):
    """tf.layers.dense defaults in Actor_Editted (models_editted.py:44-59): glorot-uniform kernels,
    zero biases; last layer U(-3e-3, 3e-3)."""
    g = generator

    def glorot(i, o):
        lim = float(np.sqrt(6.0 / (i + o)))
        return (torch.rand((i, o), generator=g) * 2 - 1) * lim
    return dict(W1=glorot(obs_dim, h1), b1=torch.zeros(h1), W2=glorot(h1, h2), b2=torch.zeros(h2),
                W3=(torch.rand((h2, nb_actions), generator=g) * 2 - 1) * 3e-3, b3=torch.zeros(nb_actions))


PARAM_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
# layer_norm=True (models_editted.py:45-46, 50-51, 85-86, 91-92): tc.layers.layer_norm creates beta, then gamma
LN_PARAM_KEYS = ("W1", "b1", "ln1_b", "ln1_g", "W2", "b2", "ln2_b", "ln2_g", "W3", "b3")


def param_keys(weights):
    return LN_PARAM_KEYS if "ln1_g" in weights else PARAM_KEYS


def with_layer_norm(weights):
    """The same network with tc.layers.layer_norm's initial parameters (gamma = 1, beta = 0) behind both hidden layers."""
    h1, h2 = weights["W1"].shape[1], weights["W2"].shape[1]
    return dict(weights, ln1_b=torch.zeros(h1), ln1_g=torch.ones(h1), ln2_b=torch.zeros(h2), ln2_g=torch.ones(h2))


def views_like(flat, like):
    """dict of views into ``flat`` with the shapes of the weight dict ``like``, in ``param_keys`` order -- the ONE walk over
    the flat layout [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3]."""
    views, o = {}, 0
    for k in param_keys(like):
        shape = tuple(torch.as_tensor(like[k]).shape)
        n = int(np.prod(shape))
        views[k] = flat[o:o + n].view(shape)
        o += n
    return views


def flatten_params(weights, device, extra=0):
    """One flat fp32 tensor in TensorFlow trainable_vars order [W1|b1|W2|b2|W3|b3] (with LayerNorm:
    [W1|b1|beta1|gamma1|W2|b2|beta2|gamma2|W3|b3]) plus a dict of VIEWS into it, so that kernels reading the dict see what
    the learner kernel wrote into the flat array.
    ``extra`` zero-initialised floats follow the parameters in the same allocation (flat[-extra:])."""
    keys = param_keys(weights)
    parts = [torch.as_tensor(weights[k], dtype=torch.float32).reshape(-1) for k in keys]
    if extra:
        parts.append(torch.zeros(int(extra), dtype=torch.float32))
    flat = torch.cat(parts).to(device).contiguous()
    return flat, views_like(flat, weights)


class AdaptiveParamNoiseSpec:
    """baselines 0.1.5 ddpg/noise.py AdaptiveParamNoiseSpec [third-party, restated in DESIGN section 5]: the stddev of
    the parameter-space noise, adapted so that the perturbed actor's actions lie ``desired_action_stddev`` from the plain
    actor's.  On an agent the value lives in ONE fp32 device scalar (``d_stddev``) that ``ssc_param_noise_perturb`` reads
    and ``ssc_param_noise_adapt`` updates; ``current_stddev`` reads it (a device -> host copy).  ``adapt`` is the same
    rule in the same fp32 arithmetic on the host."""

    def __init__(self, initial_stddev=0.1, desired_action_stddev=0.1, adoption_coefficient=1.01, d_stddev=None):
        if not float(adoption_coefficient) > 1.0:
            raise ValueError("adoption_coefficient must be > 1")
        if not float(initial_stddev) >= 0.0:
            raise ValueError("initial_stddev must be >= 0")
        self.initial_stddev = float(initial_stddev)
        self.desired_action_stddev = float(desired_action_stddev)
        self.adoption_coefficient = float(adoption_coefficient)
        self.d_stddev = d_stddev
        self.current_stddev = self.initial_stddev

    @property
    def current_stddev(self):
        if self.d_stddev is not None:
            return float(self.d_stddev.item())
        return float(self._stddev)

    @current_stddev.setter
    def current_stddev(self, value):
        self._stddev = np.float32(value)
        if self.d_stddev is not None:
            self.d_stddev.fill_(float(self._stddev))

    def adapt(self, distance):
        sd, c = np.float32(self.current_stddev), np.float32(self.adoption_coefficient)
        if np.float32(distance) > np.float32(self.desired_action_stddev):
            self.current_stddev = sd / c          # decrease stddev
        else:
            self.current_stddev = sd * c          # increase stddev (a tie lands here)

    def get_stats(self):
        return {"param_noise_stddev": self.current_stddev}

    def __repr__(self):
        return "AdaptiveParamNoiseSpec(initial_stddev={}, desired_action_stddev={}, adoption_coefficient={})".format(
            self.initial_stddev, self.desired_action_stddev, self.adoption_coefficient)


class DDPG_Baselines_agent(ValueFuncRLAgent, ReplayBufferRLAgent):
    """Action path of smartstart/RLAgents/DDPG_Baselines_agent.py (:86-273): actor forward on the GPU
    (``ssc_actor_forward``), decaying OU noise, clip, double ``scale``; transitions go to the shared
    ReplayBuffer.  ``as_policy()`` hands the same actor to the fused rollout kernel."""

    def __init__(self, env, sess=None, replay_buffer=None, buffer_size=10000, batch_size=64, num_train_iterations=50,
                 num_steps_before_train=40, ou_epsilon=1.0, ou_min_epsilon=0.01, ou_epsilon_decay_factor=.99,
                 ou_mu=0.4, ou_sigma=0.2, ou_theta=.15, actor_lr=1e-4, actor_h1=64, actor_h2=64, critic_lr=1e-3,
                 critic_h1=64, critic_h2=64, gamma=0.99, tau=0.001, layer_norm=False, normalize_observations=False,
                 normalize_returns=False, critic_l2_reg=0, enable_popart=False, clip_norm=None, reward_scale=1.,
                 lastLayerTanh=False, finalizeGraph=True, device="cuda", precision="f32", seed=None, training=True,
                 param_noise_stddev=None, param_noise_desired_action_stddev=None, param_noise_adoption_coefficient=1.01):
        args = dict(locals())
        self.param_dict = {k: (v if isinstance(v, (int, float, bool, str, type(None))) else "Not serializable")
                           for k, v in args.items() if k not in ("self", "__class__")}   # :135-137
        # ddpg_editted.py:140-149, 201-217, 291-301: Pop-Art is the conjunction (the only ret_rms.update call site is under
        # both).  One switch without the other -- in the reference the plain step, with a ret_rms that never moves for
        # normalize_returns alone -- stays refused.
        if bool(normalize_returns) != bool(enable_popart):
            raise NotImplementedError("return normalisation / popart: only the conjunction normalize_returns=True, "
                                      "enable_popart=True (Pop-Art) is on the accelerated path; one switch alone is the "
                                      "plain step in the reference, use False for both")
        self.normalize_returns, self.enable_popart = bool(normalize_returns), bool(enable_popart)
        self.layer_norm = bool(layer_norm)      # models_editted.py:45-46, 50-51, 85-86, 91-92 (fp32 kernels)
        if self.layer_norm:
            precision = "f32"
        self.env = env
        self.device = torch.device(device)
        self.lib = _ffi.lib()
        self.batch_size = batch_size
        self.num_train_iterations = num_train_iterations
        self.num_steps_before_train = num_steps_before_train
        self.remaining_steps_before_train = num_steps_before_train
        self.reward_scale = reward_scale
        self.gamma, self.tau, self.actor_lr, self.critic_lr = gamma, tau, actor_lr, critic_lr
        # ddpg_editted.py:183-191 / :175, 197 (unused by the shipped runs; the multi-workgroup learner carries both)
        if critic_l2_reg < 0 or (clip_norm is not None and not clip_norm > 0):
            raise ValueError("critic_l2_reg must be >= 0 and clip_norm None or > 0")
        self.critic_l2_reg, self.clip_norm = float(critic_l2_reg), clip_norm
        self.lastLayerTanh = bool(lastLayerTanh)
        # DDPG_editted clips what it feeds its networks to observation_range (ddpg_editted.py:66,106-109); the reference
        # agent never overrides the default (-5, 5), and it applies with normalize_observations=False too
        self.observation_range = (-5.0, 5.0)
        self.precision = precision
        self.replay_buffer = replay_buffer if replay_buffer is not None else ReplayBuffer(self, buffer_size)
        self.training_enabled = training
        nb_actions = env.action_space.shape[-1]
        obs_dim = env.observation_space.shape[-1]
        gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
        aw, cw = init_actor_weights(obs_dim, actor_h1, actor_h2, nb_actions, gen), init_critic_weights(obs_dim, critic_h1, critic_h2, nb_actions, gen)
        if self.layer_norm:
            aw, cw = with_layer_norm(aw), with_layer_norm(cw)
        # normalize_observations (ddpg_editted.py:100-109): the running obs statistics every network input goes through
        self.obs_rms = ObsRms(obs_dim, self.device) if normalize_observations else None
        # Pop-Art: the one-column return statistics; the critic outputs normalised values, every read-out of Q denormalises
        # (q * std + mean, :129-131) and the learner updates them with every iteration
        self.popart = self.normalize_returns and self.enable_popart
        self.ret_rms = ObsRms(1, self.device) if self.popart else None
        # adaptive parameter-space noise (ddpg_editted.py:151-166; main_editted.py:48: desired = initial stddev)
        self.param_noise = None
        if param_noise_stddev is not None:
            desired = param_noise_stddev if param_noise_desired_action_stddev is None else param_noise_desired_action_stddev
            # [stddev | distance]: what the perturb kernel reads and the adapt kernel writes
            self._pn_scalars = torch.zeros(2, dtype=torch.float32, device=self.device)
            self.d_param_noise_stddev, self.d_param_noise_distance = self._pn_scalars[0:1], self._pn_scalars[1:2]
            self.param_noise = AdaptiveParamNoiseSpec(param_noise_stddev, desired, param_noise_adoption_coefficient,
                                                      d_stddev=self.d_param_noise_stddev)
            self.param_noise_seed = int(seed) if seed is not None else int(np.random.randint(0, 2 ** 31 - 1))
            self.param_noise_generation = 0      # the generation the NEXT perturbation draws (acting or adaptive copy)
        self.set_weights(aw)
        self.set_critic_weights(cw)
        self.decaying_ou_action_noise = DecayingOrnsteinUhlenbeckActionNoise(
            ou_epsilon, ou_min_epsilon, ou_epsilon_decay_factor, mu=ou_mu * np.ones(nb_actions),
            sigma=float(ou_sigma) * np.ones(nb_actions), theta=ou_theta)   # :152-157
        self.ou = dict(mu=ou_mu, sigma=ou_sigma, theta=ou_theta)
        self.d_epsilon.fill_(float(max(ou_epsilon, 0.0)))

    # ---- weights ---------------------------------------------------------------------------
    def set_weights(self, weights):
        """weights: dict W1[obs,h1] b1 W2[h1,h2] b2 W3[h2,act] b3 (TensorFlow layout)."""
        # [parameters | epsilon]: what an actor needs from the learner is ONE contiguous array (one broadcast in the
        # sharded loop); the trailing float is the device copy of the OU epsilon (as_policy(device_epsilon=True))
        self.actor_sync, self.weights = flatten_params(weights, self.device, extra=1)
        self.actor_flat, self.d_epsilon = self.actor_sync[:-1], self.actor_sync[-1:]
        if hasattr(self, "decaying_ou_action_noise"):
            self.d_epsilon.fill_(float(max(self.decaying_ou_action_noise.epsilon, 0.0)))
        self.target_actor_flat = self.actor_flat.clone()        # target_init_updates (ddpg_editted.py:331-336)
        self._adam_actor = (torch.zeros_like(self.actor_flat), torch.zeros_like(self.actor_flat))
        if hasattr(self, "_adam_t"):
            self._adam_t[0] = 0                                  # fresh moments start their bias correction over
        w = self.weights
        self.obs_dim, self.h1 = w["W1"].shape
        self.h2, self.act_dim = w["W3"].shape
        d = _ffi.ActorDesc()
        d.obs_dim, d.h1, d.h2, d.act_dim = self.obs_dim, self.h1, self.h2, self.act_dim
        _ffi.set_net_ptrs(d, w)
        d.last_layer_tanh = int(self.lastLayerTanh)
        d.precision = _ffi.SSC_PREC_F32 if self.precision == "f32" else _ffi.SSC_PREC_BF16_MFMA
        d.obs_clip = float(self.observation_range[1])
        self._desc = d
        if self.param_noise is not None:
            self._setup_param_noise()

    # ---- parameter-space noise ---------------------------------------------------------------
    def _views_desc(self, flat):
        """views into ``flat`` laid out like ``actor_flat`` + the actor descriptor over them"""
        views = views_like(flat, self.weights)
        d = _ffi.ActorDesc.from_buffer_copy(self._desc)
        _ffi.set_net_ptrs(d, views)
        return views, d

    def _setup_param_noise(self):
        """setup_param_noise (ddpg_editted.py:151-166): the acting copy and the copy the stddev is adapted on, both flat
        arrays in the layout of ``actor_flat``; the acting copy is perturbed right away (the reset() before the first
        episode, training_editted.py:70)."""
        self.perturbed_actor_flat = self.actor_flat.clone()
        self.adaptive_actor_flat = self.actor_flat.clone()
        self.perturbed_weights, self._perturbed_desc = self._views_desc(self.perturbed_actor_flat)
        _, self._adaptive_desc = self._views_desc(self.adaptive_actor_flat)
        # LayerNorm beta / gamma are not perturbable_vars (models_editted.py:18-19): [beta | gamma] of each layer is one range
        self._pn_skip, o = [], 0
        for k, v in self.weights.items():
            if k in ("ln1_b", "ln2_b"):
                self._pn_skip += [o, o + 2 * v.numel()]
            o += v.numel()
        self._pn_skip = tuple(self._pn_skip) if self._pn_skip else (0, 0, 0, 0)
        self.perturbed_generation = None
        if self.device.type == "cuda":
            self.perturb_policy()

    def _perturb(self, dst):
        """dst = actor_flat + stddev * N(0, 1) with a generation of its own; returns that generation"""
        g = self.param_noise_generation
        self.param_noise_generation = g + 1
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_param_noise_perturb(self.actor_flat.numel(), _ffi.ptr(self.actor_flat), _ffi.ptr(dst),
                                                        _ffi.ptr(self.d_param_noise_stddev), *self._pn_skip,
                                                        self.param_noise_seed, g, _ffi.stream()))
        return g

    def perturb_policy(self):
        """The perturbation of DDPG_editted.reset (ddpg_editted.py:382-385): ``perturbed_actor_flat`` = actor + noise of the
        current (device) stddev.  Stream-ordered; ``perturbed_generation`` is the generation it drew."""
        if self.param_noise is None:
            raise RuntimeError("the agent was built without param_noise_stddev")
        self.perturbed_generation = self._perturb(self.perturbed_actor_flat)

    def adapt_param_noise(self, obs_batch, obs_rms=None):
        """DDPG_editted.adapt_param_noise (ddpg_editted.py:360-376) on a batch of obs0 [m, obs_dim]: perturb the adaptive
        copy, distance = sqrt(mean((actor(obs) - adaptive_actor(obs))^2)), adapt the device stddev.  Returns the
        1-element DEVICE tensor holding the distance (no host read; 0. without parameter noise, like the reference)."""
        if self.param_noise is None:
            return 0.
        o = torch.as_tensor(obs_batch, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim).contiguous()
        self._perturb(self.adaptive_actor_flat)
        a = self._forward(self._desc, o, obs_rms)
        b = self._forward(self._adaptive_desc, o, obs_rms)
        pn = self.param_noise
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_param_noise_adapt(a.numel(), _ffi.ptr(a), _ffi.ptr(b), pn.desired_action_stddev,
                                                      pn.adoption_coefficient, _ffi.ptr(self.d_param_noise_stddev),
                                                      _ffi.ptr(self.d_param_noise_distance), _ffi.stream()))
        return self.d_param_noise_distance

    def param_noise_cycle(self, obs_batch, dst=None, obs_rms=None):
        """:meth:`adapt_param_noise` on ``obs_batch`` [m <= 4096, obs_dim] followed by :meth:`perturb_policy`, in ONE launch
        (``ssc_param_noise_cycle``): the adaptive copy is drawn, used and dropped inside the kernel (``adaptive_actor_flat``
        is not touched), the device stddev is adapted and ``dst`` (default ``perturbed_actor_flat``) becomes actor + noise
        of the NEW stddev.  Consumes two generations, adaptive then acting, exactly like the pair of calls, and leaves
        ``perturbed_generation`` at the acting one.  Both forwards run in fp32.  Returns the 1-element DEVICE tensor
        holding the distance."""
        if self.param_noise is None:
            raise RuntimeError("the agent was built without param_noise_stddev")
        o = torch.as_tensor(obs_batch, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim).contiguous()
        dst = self.perturbed_actor_flat if dst is None else dst
        if dst.dtype != torch.float32 or dst.numel() != self.actor_flat.numel() or not dst.is_contiguous():
            raise ValueError("dst must be a contiguous fp32 array of the size of actor_flat")
        g = self.param_noise_generation
        pn, rms = self.param_noise, self._rms_block(obs_rms)
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_param_noise_cycle(
                ctypes.byref(self._desc), o.shape[0], _ffi.ptr(o), _ffi.ptr(rms), self.actor_flat.numel(),
                _ffi.ptr(self.actor_flat), *self._pn_skip, self.param_noise_seed, g, g + 1, pn.desired_action_stddev,
                pn.adoption_coefficient, _ffi.ptr(self.d_param_noise_stddev), _ffi.ptr(self.d_param_noise_distance),
                _ffi.ptr(dst), _ffi.stream()))
        self.param_noise_generation = g + 2
        self.perturbed_generation = g + 1
        return self.d_param_noise_distance

    def set_critic_weights(self, weights):
        """weights: dict W1[obs,h1] b1 W2[h1+act,h2] b2 W3[h2,1] b3 (Critic_Editted, models_editted.py:78-100)."""
        self.critic_flat, self.critic_weights = flatten_params(weights, self.device)
        self.target_critic_flat = self.critic_flat.clone()
        self._adam_critic = (torch.zeros_like(self.critic_flat), torch.zeros_like(self.critic_flat))
        self._adam_t = torch.zeros(2, dtype=torch.int32, device=self.device)
        w = self.critic_weights
        c = _ffi.CriticDesc()
        c.obs_dim, c.h1 = w["W1"].shape
        c.h2 = w["W2"].shape[1]
        c.act_dim = w["W2"].shape[0] - c.h1
        _ffi.set_net_ptrs(c, w)
        c.last_layer_tanh = int(self.lastLayerTanh)
        c.obs_clip = float(self.observation_range[1])
        self._critic_desc = c

    def _rms_block(self, obs_rms=None):
        """The statistics block the networks read: ``obs_rms`` (an ObsRms or its f64 tensor), else the agent's own."""
        r = self.obs_rms if obs_rms is None else obs_rms
        return r.block if isinstance(r, ObsRms) else r

    def _denormalize(self, q):
        """critic_tf = denormalize(normalized_critic_tf, ret_rms) (ddpg_editted.py:129-131): q * std + mean in fp32, a
        multiply and an add on the current stream with the statistics read on the device"""
        mean, std = self.ret_rms.mean_std_device()
        return q * std + mean

    def critic(self, obs, act, obs_rms=None, raw=False):
        """Critic_Editted forward: Q(obs [m, obs_dim], act [m, act_dim]) -> [m].  With observation statistics (the
        agent's, or ``obs_rms``) the network sees clip((obs - mean) / std).  With return statistics
        (Pop-Art: ``normalize_returns`` with ``enable_popart``) the network's output is the normalised value and the result is denormalised;
        ``raw=True`` returns the network's output itself."""
        o = torch.as_tensor(obs, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim).contiguous()
        a = torch.as_tensor(act, dtype=torch.float32, device=self.device).reshape(o.shape[0], -1).contiguous()
        q = torch.empty(o.shape[0], dtype=torch.float32, device=self.device)
        rms = self._rms_block(obs_rms)
        with torch.cuda.device(self.device):
            if rms is None:
                _ffi.check(self.lib.ssc_critic_forward(ctypes.byref(self._critic_desc), o.shape[0], _ffi.ptr(o),
                                                       _ffi.ptr(a), _ffi.ptr(q), _ffi.stream()))
            else:
                _ffi.check(self.lib.ssc_critic_forward_rms(ctypes.byref(self._critic_desc), o.shape[0], _ffi.ptr(o),
                                                           _ffi.ptr(a), _ffi.ptr(q), _ffi.stream(), _ffi.ptr(rms)))
        return q if raw or self.ret_rms is None else self._denormalize(q)

    def actor(self, obs, obs_rms=None):
        """Actor_Editted forward (models_editted.py:38-61) on a batch: obs [m, obs_dim] -> [m, act_dim] (normalised
        observations as in :meth:`critic`)."""
        return self._forward(self._desc, obs, obs_rms)

    def _forward(self, desc, obs, obs_rms=None):
        """:meth:`actor` through ``desc``: the actor itself or one of its perturbed copies"""
        o = torch.as_tensor(obs, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim).contiguous()
        out = torch.empty((o.shape[0], self.act_dim), dtype=torch.float32, device=self.device)
        rms = self._rms_block(obs_rms)
        with torch.cuda.device(self.device):
            if rms is None:
                _ffi.check(self.lib.ssc_actor_forward(ctypes.byref(desc), o.shape[0], _ffi.ptr(o), _ffi.ptr(out),
                                                      _ffi.stream()))
            else:
                _ffi.check(self.lib.ssc_actor_forward_rms(ctypes.byref(desc), o.shape[0], _ffi.ptr(o), _ffi.ptr(out),
                                                          _ffi.stream(), _ffi.ptr(rms)))
        return out

    # ---- RLAgent ---------------------------------------------------------------------------
    def scale(self, actions):
        """:236-240"""
        actions = np.clip(actions, -1, 1)
        low, high = self.env.action_space.low, self.env.action_space.high
        return (((actions + 1) / 2) * (high - low)) + low

    def get_action(self, state):
        """:206-234 -> DDPG_editted.pi (ddpg_editted.py:255-272)"""
        # pi (ddpg_editted.py:256-259): the perturbed actor acts while training when parameter noise is on
        desc = self._perturbed_desc if self.param_noise is not None and self.training_enabled else self._desc
        action = self._forward(desc, np.asarray(state, np.float32)[None, :])[0].cpu().numpy()   # fp32, like sess.run
        noise = self.decaying_ou_action_noise()
        action = action + noise.astype(np.float32)             # in-place add keeps fp32 (:266-270)
        action = np.clip(action, -1.0, 1.0)                    # :271
        return self.scale(self.scale(action))

    def as_policy(self, precision=None, device_epsilon=False, obs_rms=None, perturbed=False):
        """The same action path as a fused-rollout policy (current epsilon).  ``device_epsilon``: the kernel reads
        epsilon from ``self.d_epsilon`` (kept current by a :class:`rl_train.DecaySchedule`) instead of the host value.
        With observation statistics (the agent's, or ``obs_rms``) the rollout reads them once per launch.
        ``perturbed=True``: the policy over ``perturbed_weights`` (views into ``perturbed_actor_flat``, so every
        :meth:`perturb_policy` shows in the next launch; LayerNorm parameters are copied unperturbed)."""
        n = self.decaying_ou_action_noise
        if "ln1_g" in self.weights:
            precision = "f32"                    # LayerNorm networks run on the fp32 kernels
        if perturbed and self.param_noise is None:
            raise ValueError("as_policy(perturbed=True) needs an agent built with param_noise_stddev")
        weights = self.perturbed_weights if perturbed else self.weights
        return ActorPolicy(weights, last_layer_tanh=self.lastLayerTanh, precision=precision or "bf16_mfma",
                           ou_mu=float(self.ou["mu"]), ou_sigma=float(self.ou["sigma"]), ou_theta=float(self.ou["theta"]),
                           ou_dt=n.dt, ou_epsilon=float(max(n.epsilon, 0)), obs_clip=float(self.observation_range[1]),
                           d_ou_epsilon=self.d_epsilon if device_epsilon else None, d_obs_rms=self._rms_block(obs_rms))

    def get_state_value(self, state, raw=False):
        """:197-204 -> DDPG_editted.get_q_value (ddpg_editted.py:274-279): Q(s, pi(s)) without noise.
        Returns [n, 1] for a batch, a length-1 array for a single state (like ``sess.run(...)[0]``).  Denormalised with
        return statistics, like :meth:`critic` (``raw=True``: the network's output)."""
        single = np.ndim(state) == 1 if not torch.is_tensor(state) else state.dim() == 1
        q = self.state_value_device(state, raw=raw).reshape(-1, 1).double().cpu().numpy()
        return q[0] if single else q

    def state_value_device(self, state, raw=False):
        """Q(s, pi(s)) for a batch of states as a DEVICE tensor [m] (no host round trip: the SmartStart selection of the
        vectorised loop feeds candidate states gathered from the device replay ring).  Denormalised with return
        statistics, like :meth:`critic` (``raw=True``: the network's output)."""
        o = torch.as_tensor(state, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim)
        return self.critic(o, self.actor(o), raw=raw).reshape(-1)     # (both with the agent's observation statistics, if any)

    def observe(self, state, action, reward, new_state, done):
        """:242-247 (store_transition, ddpg_editted.py:281-285)"""
        self.replay_buffer.add(self, state, action, reward * self.reward_scale, done, new_state)
        if self.obs_rms is not None:                            # store_transition: obs_rms.update(np.array([obs0]))
            self.obs_rms.update_rows(np.asarray(state, np.float32).reshape(1, -1))
        self.remaining_steps_before_train -= 1
        if self.training_enabled and self.remaining_steps_before_train <= 0:
            self.train()

    def start_new_episode(self, state):
        """:249-250 -- ``pass`` in the reference: a bare DDPG agent never marks episode starts in its buffer (only the
        SmartStart wrapper, the buffer's main agent then, does: smartexplorationcontinuous.py:369).  With parameter noise
        the acting copy is perturbed anew, as DDPG_editted.reset does between episodes (ddpg_editted.py:382-385)."""
        if self.param_noise is not None:
            self.perturb_policy()

    def render(self, env, **kwargs):
        return env.render()

    def end_episode(self):
        """:255-258"""
        self.decaying_ou_action_noise.reset()
        self.decaying_ou_action_noise.reduce_epsilon()
        if self.training_enabled:
            self.train()

    # ---- training diagnostics (ddpg_editted.py:219-253 setup_stats, 341-358 get_stats) ---------------------------------
    # the reference's stats_names with normalize_observations and parameter noise on: the eleven slots of the device block.
    # With Pop-Art (normalize_returns + enable_popart) the four Q slots hold the DENORMALISED values (get_stats_device), and ret_rms_mean /
    # ret_rms_std -- first in the reference's list, :223-225 -- are added in front by get_stats() from agent.ret_rms (the
    # vectorised loop logs them beside the block: summary.ret_rms)
    STATS_NAMES = ("obs_rms_mean", "obs_rms_std", "reference_Q_mean", "reference_Q_std", "reference_actor_Q_mean",
                   "reference_actor_Q_std", "reference_action_mean", "reference_action_std",
                   "reference_perturbed_action_mean", "reference_perturbed_action_std", "param_noise_stddev")
    _STATS_KEY = 0x5354415453          # the stats sample's own Philox key / host generator seed ("STATS")

    def set_stats_sample(self, obs, act):
        """Fix the sample the diagnostics are evaluated on (ddpg_editted.py:345-349 draws it once): obs [m, obs_dim] and
        act [m, act_dim], host arrays or device tensors, 1 <= m <= 4096.  Kept as device tensors (copies)."""
        o = torch.as_tensor(obs, dtype=torch.float32).to(self.device).reshape(-1, self.obs_dim).contiguous().clone()
        a = torch.as_tensor(act, dtype=torch.float32).to(self.device).reshape(o.shape[0], -1).contiguous().clone()
        if a.shape[1] != self.act_dim or not 1 <= o.shape[0] <= 4096:
            raise ValueError(f"stats sample: need 1..4096 rows of ({self.obs_dim}, {self.act_dim}) columns, got "
                             f"{tuple(o.shape)} / {tuple(a.shape)}")
        self.stats_sample = (o, a)

    def _draw_stats_sample(self, replay):
        """``batch_size`` records of ``replay`` (a host ReplayBuffer or a DeviceReplayBuffer), drawn from a stream of their
        own: neither the ring's batch counter nor the host ``random`` state moves, so the learner's next batch is the one
        it would have been."""
        B = self.batch_size
        if len(replay) < B:
            raise ValueError(f"get_stats: the replay buffer holds {len(replay)} records, the sample needs {B}")
        if hasattr(replay, "sample_indices"):                    # DeviceReplayBuffer: ssc_replay_sample under another key
            idx = torch.empty((1, B), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                _ffi.check(self.lib.ssc_replay_sample((replay.seed ^ self._STATS_KEY) & (2 ** 64 - 1), 0, len(replay), 1, B,
                                                      _ffi.ptr(idx), _ffi.stream()))
            rows = idx[0].long()
            self.set_stats_sample(replay.s.index_select(0, rows), replay.a.index_select(0, rows))
        else:                                                    # replay_buffer.py:79-91 with a generator of its own
            import random
            rows = np.asarray(random.Random(self._STATS_KEY).sample(range(len(replay)), B), dtype=np.int64)
            s, a = replay._gather(rows)[:2]
            self.set_stats_sample(np.asarray(s, np.float32).reshape(B, -1), np.asarray(a, np.float32).reshape(B, -1))

    def get_stats_device(self, replay=None, out=None, perturbed=None):
        """The stats_ops of DDPG_editted in one enqueue (``ssc_ddpg_stats``): a float64 DEVICE tensor [SSC_DDPG_N_STATS] in
        ``STATS_NAMES`` order, NaN where a slot does not apply (no observation statistics / no parameter noise).  No host
        read; stream-ordered.  The first call without a fixed sample draws ``batch_size`` records from ``replay`` (default:
        the agent's own buffer) and keeps them.  ``out``: a contiguous float64 device tensor of that size to write into.
        ``perturbed``: the flat perturbed copy to measure (default ``perturbed_actor_flat``)."""
        if getattr(self, "stats_sample", None) is None:
            self._draw_stats_sample(self.replay_buffer if replay is None else replay)
        o, a = self.stats_sample
        n = _ffi.SSC_DDPG_N_STATS
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.numel() != n or not out.is_contiguous() or out.device != o.device:
            raise ValueError(f"out must be a contiguous float64 tensor of {n} elements on {o.device}")
        pdesc = sd = None
        if self.param_noise is not None:
            sd = self.d_param_noise_stddev
            pdesc = self._perturbed_desc
            if perturbed is not None and perturbed.data_ptr() != self.perturbed_actor_flat.data_ptr():
                if perturbed.dtype != torch.float32 or perturbed.numel() != self.actor_flat.numel() or not perturbed.is_contiguous():
                    raise ValueError("perturbed must be a contiguous fp32 array of the size of actor_flat")
                cache = self.__dict__.setdefault("_stats_pdesc", {})      # (the overlapped loop alternates two copies)
                if perturbed.data_ptr() not in cache:
                    cache[perturbed.data_ptr()] = (perturbed, self._views_desc(perturbed)[1])
                pdesc = cache[perturbed.data_ptr()][1]
        with torch.cuda.device(self.device):
            need = int(self.lib.ssc_ddpg_stats_workspace_bytes(o.shape[0]))
            ws = getattr(self, "_stats_ws", None)
            if ws is None or ws.numel() < need:
                ws = self._stats_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            _ffi.check(self.lib.ssc_ddpg_stats(ctypes.byref(self._desc), ctypes.byref(self._critic_desc),
                                               None if pdesc is None else ctypes.byref(pdesc), o.shape[0], _ffi.ptr(o),
                                               _ffi.ptr(a), _ffi.ptr(self._rms_block()), _ffi.ptr(sd), _ffi.ptr(out),
                                               _ffi.ptr(ws), ws.numel(), _ffi.stream()))
        if self.ret_rms is not None:
            # the four Q slots are statistics of the network's (normalised) output: mean * std + mean_ret, std * std_ret
            # in f64 on the current stream (the mean and the std of an affine map of the sample)
            mean, std = (x.to(torch.float64) for x in self.ret_rms.mean_std_device())
            out[2:6:2].mul_(std).add_(mean)
            out[3:6:2].mul_(std)
        return out

    @classmethod
    def stats_dict(cls, values):
        """name -> Python float in ``STATS_NAMES`` order, without the slots that do not apply (NaN)."""
        vals = [float(v) for v in values]
        return {k: v for k, v in zip(cls.STATS_NAMES, vals) if not np.isnan(v)}

    def get_stats(self, replay=None):
        """DDPG_editted.get_stats (ddpg_editted.py:341-358): dict name -> float in the reference's order; with parameter
        noise merged with ``param_noise.get_stats()`` (:355-356).  Reads the device block (a device -> host copy)."""
        stats = self.stats_dict(self.get_stats_device(replay).cpu().tolist())
        ret_rms = getattr(self, "ret_rms", None)
        if ret_rms is not None:                                 # setup_stats lists ret_rms first (:223-225)
            mean, std = ret_rms.mean_std()
            stats = {"ret_rms_mean": float(mean[0]), "ret_rms_std": float(std[0]), **stats}
        if self.param_noise is not None:
            stats = {**stats, **self.param_noise.get_stats()}
        return stats

    # ---- evaluation rollouts (training_editted.py:122-138; reported :160-164) -----------------------------------------
    EVAL_NAMES = ("eval/episodes", "eval/return", "eval/return_std", "eval/Q", "eval/Q_std", "eval/steps", "eval/goals",
                  "eval/episode_length")
    _EVAL_COUNTS = ("eval/episodes", "eval/steps", "eval/goals")

    def evaluate_device(self, eval_env, nb_eval_steps, out=None, log=None, q=None, carry_returns=False):
        """``nb_eval_steps`` steps of the reference's evaluation loop on every env of ``eval_env`` (a VecEnv of its own, never
        the training env) in one fused launch (``ssc_ddpg_eval_rollout``): the PLAIN actor without noise of any kind -- also
        on a parameter-noise agent, ``pi(apply_noise=False)`` uses ``actor_tf`` -- Q of its raw output from the critic at
        every step, the live observation statistics when the agent normalises.  Returns the float64 DEVICE tensor
        [SSC_DDPG_N_EVAL] in ``EVAL_NAMES`` order (NaN return / length when no episode ended).  No host read; enqueued on
        the current stream.  ``eval_env`` keeps its own state, seed, ``env_id0`` and step counter ``t`` (advanced by
        ``nb_eval_steps``; reset first if it never was), so consecutive calls continue the same episodes.
        ``carry_returns=False`` is the reference: every env's running return starts at 0 in each call while its episode goes
        on (training_editted.py:125); True carries ``eval_env.ep_ret`` over.  ``out``: a contiguous float64 device tensor
        of that size to write into; ``log``: a TransitionChunk [nb_eval_steps, n] that receives the transitions (the
        executed action); ``q``: a contiguous fp32 [nb_eval_steps, n] tensor that receives Q (the reference's eval_qs)."""
        K, n = int(nb_eval_steps), eval_env.n
        if K < 1 or K != nb_eval_steps:
            raise ValueError("nb_eval_steps must be a positive integer")
        if eval_env.obs_dim != self.obs_dim:
            raise ValueError(f"eval_env observes {eval_env.obs_dim} values, the agent's networks take {self.obs_dim}")
        dev = eval_env.s0.device                         # (a tensor's device carries its index: cuda:0, not cuda)
        if dev != self.actor_flat.device:
            raise ValueError(f"eval_env lives on {dev}, the agent on {self.actor_flat.device}")
        ne = _ffi.SSC_DDPG_N_EVAL
        if out is None:
            out = torch.empty(ne, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.numel() != ne or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous float64 tensor of {ne} elements on {dev}")
        if log is not None and (log.K, log.N, log.obs_dim) != (K, n, eval_env.obs_dim):
            raise ValueError("log chunk has the wrong shape")
        if q is not None and (q.dtype != torch.float32 or tuple(q.shape) != (K, n) or not q.is_contiguous()
                              or q.device != dev):
            raise ValueError(f"q must be a contiguous fp32 [{K}, {n}] tensor on {dev}")
        if eval_env._needs_reset:
            eval_env.reset()
        if log is not None:
            log.step0, log.env_id0 = eval_env.t, eval_env.env_id0
        st = eval_env.rollout_state(ou=False)
        log_s = log.as_struct() if log is not None else None
        with torch.cuda.device(self.device):
            need = int(self.lib.ssc_ddpg_eval_workspace_bytes(n))
            ws = getattr(self, "_eval_ws", None)
            if ws is None or ws.numel() < need:
                ws = self._eval_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            _ffi.check(self.lib.ssc_ddpg_eval_rollout(
                ctypes.byref(eval_env.params), ctypes.byref(self._desc), ctypes.byref(self._critic_desc),
                float(eval_env.action_space.low[0]), float(eval_env.action_space.high[0]), n, K, ctypes.byref(st),
                _ffi.ptr(self._rms_block()), ctypes.byref(log_s) if log_s is not None else None, _ffi.ptr(q),
                0 if carry_returns else 1, _ffi.ptr(out), _ffi.ptr(ws), ws.numel(), eval_env._seed, eval_env.env_id0,
                eval_env.t, _ffi.stream()))
            if self.ret_rms is not None:                         # eval/Q, eval/Q_std and eval_qs are denormalised Q too
                mean, std = self.ret_rms.mean_std_device()
                out[3:4].mul_(std.to(torch.float64)).add_(mean.to(torch.float64))
                out[4:5].mul_(std.to(torch.float64))
                if q is not None:
                    q.mul_(std).add_(mean)
        eval_env.t += K
        return out

    @classmethod
    def eval_dict(cls, values):
        """name -> value in ``EVAL_NAMES`` order; the three counts as ints"""
        return {k: (int(v) if k in cls._EVAL_COUNTS else float(v)) for k, v in zip(cls.EVAL_NAMES, values)}

    def evaluate(self, eval_env, nb_eval_steps, **kw):
        """:meth:`evaluate_device` as a dict by ``EVAL_NAMES`` (eval/episodes, eval/steps and eval/goals as ints).  Reads
        the device block (a device -> host copy)."""
        return self.eval_dict(self.evaluate_device(eval_env, nb_eval_steps, **kw).cpu().tolist())

    def get_param_dict(self):
        return self.param_dict

    # ---- learner -------------------------------------------------------------
    def ddpg_desc(self):
        d = _ffi.DdpgDesc()
        d.obs_dim, d.act_dim = self.obs_dim, self.act_dim
        d.actor_h1, d.actor_h2 = self.h1, self.h2
        d.critic_h1, d.critic_h2 = self._critic_desc.h1, self._critic_desc.h2
        d.last_layer_tanh, d.batch_size = int(self.lastLayerTanh), self.batch_size
        d.actor, d.critic = self.actor_flat.data_ptr(), self.critic_flat.data_ptr()
        d.target_actor, d.target_critic = self.target_actor_flat.data_ptr(), self.target_critic_flat.data_ptr()
        d.adam_m_actor, d.adam_v_actor = (t.data_ptr() for t in self._adam_actor)
        d.adam_m_critic, d.adam_v_critic = (t.data_ptr() for t in self._adam_critic)
        d.adam_t = self._adam_t.data_ptr()
        d.gamma, d.tau, d.actor_lr, d.critic_lr = self.gamma, self.tau, self.actor_lr, self.critic_lr
        d.beta1, d.beta2, d.epsilon = 0.9, 0.999, 1e-8          # ddpg_editted.py:176,198
        d.obs_clip = float(self.observation_range[1])
        d.layer_norm = int("ln1_g" in self.weights)
        d.critic_l2_reg, d.clip_norm = self.critic_l2_reg, 0.0 if self.clip_norm is None else float(self.clip_norm)
        return d

    def train_on(self, s, a, r, t, s2, batch_idx, n_iters, obs_rms=None):
        """``n_iters`` x (DDPG_editted.train + update_target_net) on device replay arrays; ``batch_idx``
        int32 [n_iters, batch_size].  Returns the (critic_loss, actor_loss) tensor [n_iters, 2].  With observation
        statistics (the agent's, or ``obs_rms``) the raw s / s2 enter the networks normalised."""
        rv = _ffi.ReplayView(s.data_ptr(), a.data_ptr(), r.data_ptr(), t.data_ptr(), s2.data_ptr(), s.shape[0])
        losses = torch.empty((n_iters, 2), dtype=torch.float32, device=self.device)
        d = self.ddpg_desc()
        if tuple(batch_idx.shape) != (n_iters, self.batch_size):
            raise ValueError(f"batch_idx must be [{n_iters}, {self.batch_size}], got {tuple(batch_idx.shape)}")
        with torch.cuda.device(self.device):
            # gradient partials of the multi-workgroup path (layers wider than 64 / batch != 64); kept with the agent
            need = (self.lib.ssc_ddpg_train_popart_workspace_bytes if self.popart
                    else self.lib.ssc_ddpg_train_workspace_bytes)(ctypes.byref(d))
            ws = getattr(self, "_train_ws", None)
            if ws is None or ws.numel() < need:
                ws = self._train_ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
            rms = self._rms_block(obs_rms)
            if self.popart:
                # Pop-Art (ddpg_editted.py:201-217, 291-301): the return statistics move with every iteration and both
                # critics' output layers with them; four launches per iteration on the multi-workgroup kernels
                _ffi.check(self.lib.ssc_ddpg_train_ws_popart(ctypes.byref(d), ctypes.byref(rv), _ffi.ptr(batch_idx), n_iters,
                                                             _ffi.ptr(losses), _ffi.ptr(ws), ws.numel(), _ffi.stream(),
                                                             _ffi.ptr(rms), _ffi.ptr(self.ret_rms.block)))
            elif rms is None:
                _ffi.check(self.lib.ssc_ddpg_train_ws(ctypes.byref(d), ctypes.byref(rv), _ffi.ptr(batch_idx), n_iters,
                                                      _ffi.ptr(losses), _ffi.ptr(ws), ws.numel(), _ffi.stream()))
            else:
                _ffi.check(self.lib.ssc_ddpg_train_ws_rms(ctypes.byref(d), ctypes.byref(rv), _ffi.ptr(batch_idx), n_iters,
                                                          _ffi.ptr(losses), _ffi.ptr(ws), ws.numel(), _ffi.stream(), _ffi.ptr(rms)))
        return losses

    def popart_workspace(self):
        """What the last Pop-Art iteration left in the learner's workspace, as views (include/ssc.h: [the plain step's
        workspace | y | partials | scalars], each part rounded up to 256 bytes): ``y`` fp32 [batch_size], ``partials`` f64
        [ceil(batch_size / 16), 2] = per-workgroup (sum y, sum y^2), ``scalars`` fp32 [4] = (mu_old, sigma_old, mu_new,
        sigma_new)."""
        if not self.popart or getattr(self, "_train_ws", None) is None:
            raise RuntimeError("popart_workspace: no Pop-Art iteration has run on this agent")
        up = lambda x: (int(x) + 255) // 256 * 256
        B, nb = self.batch_size, (self.batch_size + 15) // 16
        o_y = up(self.lib.ssc_ddpg_train_workspace_bytes(ctypes.byref(self.ddpg_desc())))
        o_part = o_y + up(4 * B)
        o_scal = o_part + up(16 * nb)
        ws = self._train_ws
        return dict(y=ws[o_y:o_y + 4 * B].view(torch.float32), partials=ws[o_part:o_part + 16 * nb].view(torch.float64).view(nb, 2),
                    scalars=ws[o_scal:o_scal + 16].view(torch.float32))

    def train_from(self, device_replay, n_iters=None):
        """``train()`` on a :class:`DeviceReplayBuffer`: batch indices drawn on the device, the records read
        where the rollout left them -- nothing crosses PCIe.  Returns the loss tensor [n_iters, 2] or None."""
        if len(device_replay) < self.batch_size:
            return None                                          # DDPG_Baselines_agent.py:265-266
        n = self.num_train_iterations if n_iters is None else int(n_iters)
        idx = device_replay.sample_indices(n, self.batch_size)
        r = device_replay
        return self.train_on(r.s, r.a, r.r, r.t, r.s2, idx, n)

    def train(self):
        """DDPG_Baselines_agent.train (:264-273): ``num_train_iterations`` x (train + update_target_net),
        each on a fresh uniform batch -- all iterations in one kernel launch."""
        if len(self.replay_buffer) < self.batch_size:
            return None
        self.remaining_steps_before_train = self.num_steps_before_train
        n = self.num_train_iterations
        B = self.batch_size
        if self.param_noise is not None:                         # the commented call of :270, once per train()
            self.adapt_param_noise(np.asarray(self.replay_buffer.sample_batch(B)[0], np.float32))
        cols = [[] for _ in range(5)]
        for _ in range(n):                                       # sample_batch per iteration (:287-289)
            for c, x in zip(cols, self.replay_buffer.sample_batch(B)):
                c.append(x)
        s, a, r, t, s2 = (np.concatenate(c) for c in cols)
        dev = self.device
        f = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(dev)
        idx = torch.arange(n * B, dtype=torch.int32, device=dev).view(n, B)
        losses = self.train_on(f(s, torch.float32), f(a, torch.float32), f(r, torch.float32), f(t, torch.uint8),
                               f(s2, torch.float32), idx, n)
        return losses


# DDPGPopulation.param_noise_cycle: one launch for all noisy agents (True), or its own fallback -- the per-agent
# adapt_and_perturb(cycle=True) calls (False: the yardstick of tools/exp_ddpg_population_param_noise.py).
POPULATION_FUSED_PARAM_NOISE = True

# DDPGPopulation.train_from / train_on on a population its single launch does not serve: sub-populations in grouped
# launches (True), or the per-agent calls one after the other (False: the yardstick of tools/exp_ddpg_population_wide.py).
# Fewer than POPULATION_WIDE_MIN_GROUP agents on the multi-workgroup kernels train alone, and so do fewer than
# POPULATION_POPART_MIN_GROUP Pop-Art agents (the smallest group size at which the grouped launches were measured to win:
# tools/exp_ddpg_population_popart.py, profiles/ddpg_population/popart.json).
POPULATION_GROUPED_WIDE = True
POPULATION_WIDE_MIN_GROUP = 2
POPULATION_POPART_MIN_GROUP = 2


def ddpg_population_route(facts):
    """The learner way of every agent of a :class:`DDPGPopulation` from per-agent facts only: ``facts[p]`` = (agent p's
    ``ssc_ddpg_desc``, popart, has statistics, the addresses of its nine parameter / optimiser arrays).  -> (``ways``, the
    groups as [(way, [agent, ...]), ...] in launch order: one ``"one_workgroup"`` group per (obs_dim, lastLayerTanh,
    statistics) key, then the ``"wide"`` group, then the ``"wide_popart"`` one).  Which learner a shape takes is the
    library's ``ssc_ddpg_learner_path``, the ``SSC_DDPG_INTERPRETER`` / ``SSC_DDPG_WIDE`` switches included."""
    P = len(facts)
    ptrs = [x for f in facts for x in f[3]]
    if len(set(ptrs)) < len(ptrs):                           # two workgroups on one array would race
        return ("alone",) * P, []
    lib, path_way = _ffi.lib(), {_ffi.SSC_DDPG_PATH_FIXED: "one_workgroup", _ffi.SSC_DDPG_PATH_WIDE: "wide"}
    ways = ["wide_popart" if popart else path_way.get(lib.ssc_ddpg_learner_path(ctypes.byref(d), 1, int(rms)), "alone")
            for d, popart, rms, _ in facts]
    keys = {}
    for p, (d, _, rms, _) in enumerate(facts):
        if ways[p] == "one_workgroup":
            keys.setdefault((d.obs_dim, bool(d.last_layer_tanh), bool(rms)), []).append(p)
    if len(keys) != 1 or ways.count("one_workgroup") != P:   # (a uniform one-workgroup population is one launch regardless)
        if not POPULATION_GROUPED_WIDE:
            return ("alone",) * P, []
        for way, least in (("wide", POPULATION_WIDE_MIN_GROUP), ("wide_popart", POPULATION_POPART_MIN_GROUP)):
            if ways.count(way) < least:
                ways = ["alone" if w == way else w for w in ways]
    groups = [("one_workgroup", ps) for ps in keys.values()]
    groups += [(way, [p for p in range(P) if ways[p] == way]) for way in ("wide", "wide_popart") if way in ways]
    return tuple(ways), groups


def _loss_rows(block, n, copy):
    """agent after agent, its rows [n_p, 2] of a loss block (None where n_p is 0) -- views of a fresh copy with ``copy``"""
    block, out, off = block.clone() if copy else block, [], 0
    for k in n:
        out.append(block[off:off + k] if k > 0 else None)
        off += k
    return out


class _LearnerGroup:
    """The agents ``ps`` of a population on one grouped learner launch: items, index and loss tensors, built when the call's
    signature changes and kept until it changes again.  Our own draw is one :class:`IndexDraw` for all rings where at
    least ``shared_draw`` agents train and all have one batch size <= 64 (the sampler's one-wave kernel; agent p reads its
    first n[p] batches of its row), else one ``ssc_replay_sample`` per ring."""
    shared_draw = 2

    def __init__(self, pop, way, ps, descs, views, n, batch_idx, rms):
        ag, dev = pop.agents, pop.device
        self.lib, self.device, self.way, self.ps, self.n = pop.lib, dev, way, ps, [n[p] for p in ps]
        active = [p for p in ps if n[p] > 0]
        sizes = {ag[p].batch_size for p in active}
        self.draw = None
        if batch_idx is None and len(active) >= self.shared_draw and len(sizes) == 1 and max(sizes) <= 64:
            self.draw = IndexDraw(len(active), max(n[p] for p in active), max(sizes), dev)
        self.idx = [None if n[p] == 0 else batch_idx[p] if batch_idx is not None else self.draw.idx[active.index(p)] if self.draw
                    else torch.empty((n[p], ag[p].batch_size), dtype=torch.int32, device=dev) for p in ps]
        self.losses = torch.empty((sum(self.n), 2), dtype=torch.float32, device=dev)
        self.rows = _loss_rows(self.losses, self.n, False)

    def _fill(self, items, descs, views, rms):
        for it, p, k, row, idx in zip(items, self.ps, self.n, self.rows, self.idx):
            v = views[p]
            it.ddpg, it.n_iters, it.d_rms = descs[p], k, rms[p]
            it.replay = _ffi.ReplayView(*(x.data_ptr() for x in v), v[0].shape[0])
            if k > 0:
                it.d_losses, it.d_batch_idx = row.data_ptr(), idx.data_ptr()

    def train(self, replays, out, copy):
        """one call: the index draw (``replays``: train_from; None: train_on), the launch, the agents' slots of ``out``"""
        if not any(self.n):
            return
        with torch.cuda.device(self.device):
            if replays is not None and self.draw is not None:
                self.draw.draw([replays[p].take_sample_key(k, self.draw.B) for p, k in zip(self.ps, self.n) if k > 0])
            elif replays is not None:                    # every ring draws under its own key, as its sample_indices would
                for p, k, idx in zip(self.ps, self.n, self.idx):
                    if k > 0:
                        seed, counter0, size = replays[p].take_sample_key(k, idx.shape[1])
                        _ffi.check(self.lib.ssc_replay_sample(seed, counter0, size, k, idx.shape[1], _ffi.ptr(idx),
                                                              _ffi.stream(self.device)))
            self._launch()
            rows = _loss_rows(self.losses, self.n, True) if copy else self.rows
        for p, r in zip(self.ps, rows):
            out[p] = r


class _OneWorkgroupGroup(_LearnerGroup):
    """agents of one (obs_dim, lastLayerTanh, statistics) key on ``ssc_ddpg_train_many``, one workgroup each"""
    shared_draw = 1

    def __init__(self, pop, way, ps, descs, views, n, batch_idx, rms):
        super().__init__(pop, way, ps, descs, views, n, batch_idx, rms)
        self.items = DeviceItems(_ffi.DdpgManyItem, len(ps), self.device)
        self._fill(self.items.items, descs, views, rms)
        self.items.upload()

    def _launch(self):
        _ffi.check(self.lib.ssc_ddpg_train_many(self.items.h_ptr, self.items.d_ptr, len(self.ps), _ffi.stream(self.device)))


class _PlanGroup(_LearnerGroup):
    """the ``"wide"`` agents on ``ssc_ddpg_train_many_wide`` or the ``"wide_popart"`` ones on ``ssc_ddpg_train_many_popart``:
    host items, each agent on its own workspace (the one its ``train_on`` keeps), and the plan the library builds from them
    (``plan``: its pinned-host and device copies)"""

    def __init__(self, pop, way, ps, descs, views, n, batch_idx, rms):
        super().__init__(pop, way, ps, descs, views, n, batch_idx, rms)
        lib, popart = self.lib, way == "wide_popart"
        item_t, ws_bytes, plan_bytes, plan, self._train = (
            (_ffi.DdpgManyPopartItem, lib.ssc_ddpg_train_popart_workspace_bytes, lib.ssc_ddpg_train_many_popart_plan_bytes,
             lib.ssc_ddpg_train_many_popart_plan, lib.ssc_ddpg_train_many_popart) if popart else
            (_ffi.DdpgManyWideItem, lib.ssc_ddpg_train_workspace_bytes, lib.ssc_ddpg_train_many_wide_plan_bytes,
             lib.ssc_ddpg_train_many_wide_plan, lib.ssc_ddpg_train_many_wide))
        self.items = (item_t * len(ps))()
        self._fill(self.items, descs, views, rms)
        self.ws = []                                     # (alive as long as the plan names them)
        for it, p in zip(self.items, ps):
            a = pop.agents[p]
            if popart:
                it.d_ret_rms = a.ret_rms.block.data_ptr()
            need = int(ws_bytes(ctypes.byref(descs[p])))
            ws = getattr(a, "_train_ws", None)
            if ws is None or ws.numel() < need:
                ws = a._train_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            it.d_workspace, it.workspace_bytes = ws.data_ptr(), ws.numel()
            self.ws.append(ws)
        nbytes = int(plan_bytes(len(ps)))
        self.plan = DeviceItems(ctypes.c_uint8, nbytes, self.device)
        _ffi.check(plan(ctypes.addressof(self.items), len(ps), self.plan.h_ptr, nbytes))
        self.plan.upload()

    def _launch(self):
        _ffi.check(self._train(ctypes.addressof(self.items), self.plan.h_ptr, self.plan.d_ptr, len(self.ps), _ffi.stream(self.device)))


class DDPGPopulation:
    """P independent :class:`DDPG_Baselines_agent` objects -- seeds x hyper-parameter grids, what the reference fans out
    over processes (experimenter.py) -- trained by ONE learner launch, one workgroup per agent (``ssc_ddpg_train_many``),
    on batch indices drawn by one launch (``ssc_replay_sample_many``).  The agents are wrapped, not copied: every result is
    bit for bit what ``agent.train_from`` / ``agent.train_on`` gives agent by agent.

    The launch serves the agents ``ssc_ddpg_learner_path`` -- the library's own rule, the ``SSC_DDPG_INTERPRETER`` /
    ``SSC_DDPG_WIDE`` switches included -- sends to the one-workgroup kernel (the shipped 64-32 shape at batch 64), one
    launch per (obs_dim, lastLayerTanh, statistics) key, and no array may be shared by two agents.  ``fused`` tells whether
    the last call went in one such launch as a whole.

    :func:`ddpg_population_route` gives every agent its way (``ways``: one of ``"one_workgroup"``, ``"wide"``,
    ``"wide_popart"``, ``"alone"`` per agent, for the last call) and the groups.  The agents the library sends to the
    multi-workgroup kernels (wider layers, other batch sizes, LayerNorm, critic_l2_reg, clip_norm, statistics on a shape
    without a normalising one-workgroup build) train together in the grouped launches of ``ssc_ddpg_train_many_wide``: 2
    launches per iteration for all of them (3 with critic_l2_reg / clip_norm) on a plan this object owns.  The Pop-Art
    agents (``normalize_returns`` with ``enable_popart``), of any shape, train together in the grouped launches of
    ``ssc_ddpg_train_many_popart``: 4 launches per iteration for all of them (5 with critic_l2_reg / clip_norm), each agent
    on its own ``ret_rms`` block and workspace.  Everything else -- the step interpreter's shapes, the tiled 64-32 path,
    fewer wide agents than ``POPULATION_WIDE_MIN_GROUP`` or Pop-Art ones than ``POPULATION_POPART_MIN_GROUP``, agents that
    share an array -- runs ``agent.train_from`` / ``agent.train_on`` as before, and so does every agent of a population
    that is not one launch as a whole when ``POPULATION_GROUPED_WIDE`` is False.  A call runs the lone agents first, then
    the one-workgroup groups, the wide group and the Pop-Art group.

    Index and loss tensors and the pinned-host and device copies of the launch descriptors stay with the population and
    are rebuilt only when a pointer, an iteration count or a ring changes: in steady state a call uploads the P sampling
    keys and nothing else.  The loss tensors a call returns are therefore views of one buffer the NEXT call overwrites
    (``copy=True`` returns views of a fresh copy instead).

    What the agents of a sweep are compared by comes in one launch per phase too: :meth:`evaluate_device` (eval/return,
    eval/Q) and :meth:`get_stats_device` (the ``get_stats`` diagnostics), for any mix of network shapes -- and so does the
    adaption interval of the agents with parameter-space noise: :meth:`param_noise_cycle`."""

    def __init__(self, agents):
        self.agents = list(agents)
        if not self.agents:
            raise ValueError("a population needs at least one agent")
        self.device = self.agents[0].device
        if any(a.device != self.device for a in self.agents):
            raise ValueError("the agents of a population live on one device")
        self.lib = _ffi.lib()
        self.fused = None
        self.ways = None
        self._sig = None
        self._groups = None

    def __len__(self):
        return len(self.agents)

    @staticmethod
    def _arrays(a):
        return (a.actor_flat, a.critic_flat, a.target_actor_flat, a.target_critic_flat, *a._adam_actor, *a._adam_critic, a._adam_t)

    # ---- the two public calls --------------------------------------------------------------------
    def _iters(self, n_iters):
        if n_iters is None:
            return [int(a.num_train_iterations) for a in self.agents]
        if isinstance(n_iters, (int, np.integer)):
            return [int(n_iters)] * len(self.agents)
        n = [int(x) for x in n_iters]
        if len(n) != len(self.agents) or min(n) < 0:
            raise ValueError("n_iters: None, one count, or one count >= 0 per agent")
        return n

    def train_from(self, replays, n_iters=None, copy=False):
        """``agent.train_from(replay, n_iters)`` for every (agent, :class:`DeviceReplayBuffer`) pair -> list of the loss
        tensors [n_iters_p, 2]; None for an agent whose ring holds fewer than ``batch_size`` records (it is left exactly as
        it is).  ``n_iters``: None (each agent's ``num_train_iterations``), one count, or one per agent.  Every ring's index
        stream (``seed``, batches drawn so far) moves exactly as its own ``sample_indices`` would move it."""
        replays = list(replays)
        if len(replays) != len(self.agents):
            raise ValueError("one replay ring per agent")
        n = [k if len(r) >= a.batch_size else 0 for k, r, a in zip(self._iters(n_iters), replays, self.agents)]
        return self._train([(r.s, r.a, r.r, r.t, r.s2) for r in replays], n, None, replays, copy)

    def train_on(self, views, batch_idx, n_iters, copy=False):
        """The index-explicit form: ``views[p]`` = agent p's (s, a, r, t, s2) device arrays, ``batch_idx[p]`` int32
        [n_iters[p], agent p's batch_size] (ignored where ``n_iters[p]`` is 0) -> list of loss tensors, None where ``n_iters[p]`` is 0."""
        n = self._iters(n_iters)
        views, batch_idx = [tuple(v) for v in views], list(batch_idx)
        if len(views) != len(self.agents) or len(batch_idx) != len(self.agents):
            raise ValueError("one set of replay arrays and one index tensor per agent")
        for a, k, idx in zip(self.agents, n, batch_idx):
            if k > 0 and (tuple(idx.shape) != (k, a.batch_size) or idx.dtype != torch.int32 or not idx.is_contiguous()):
                raise ValueError(f"batch_idx must be contiguous int32 [{k}, {a.batch_size}]")
        return self._train(views, n, batch_idx, None, copy)

    def _train(self, views, n, batch_idx, replays, copy):
        """the call: the agents that train alone, one after the other, then every group's launch in ``_groups`` order;
        ``replays`` (train_from) or ``batch_idx`` (train_on) is None"""
        self._prepare(views, n, batch_idx)
        ag, out = self.agents, [None] * len(self.agents)
        for p, way in enumerate(self.ways):
            if way == "alone" and n[p] > 0:
                out[p] = ag[p].train_from(replays[p], n[p]) if batch_idx is None else ag[p].train_on(*views[p], batch_idx[p], n[p])
        for g in self._groups:
            g.train(replays, out, copy)
        return out

    def _prepare(self, views, n, batch_idx):
        """Route the agents (-> ``ways``, ``fused``) and build the groups (-> ``_groups``) unless nothing they depend on
        changed since the last call."""
        ag = self.agents
        ptrs = [tuple(t.data_ptr() for t in self._arrays(a)) for a in ag]
        rms = [None if a.obs_rms is None else a._rms_block().data_ptr() for a in ag]
        switches = tuple(os.environ.get(k) for k in ("SSC_DDPG_INTERPRETER", "SSC_DDPG_WIDE")) + (POPULATION_GROUPED_WIDE, POPULATION_WIDE_MIN_GROUP, POPULATION_POPART_MIN_GROUP)
        sig = (switches, tuple(ptrs), tuple(rms), tuple(None if a.ret_rms is None else a.ret_rms.block.data_ptr() for a in ag), tuple(n),
               tuple((v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(), v[4].data_ptr(), v[0].shape[0]) for v in views),
               None if batch_idx is None else tuple(idx.data_ptr() if k > 0 else 0 for idx, k in zip(batch_idx, n)),
               tuple((a.gamma, a.tau, a.actor_lr, a.critic_lr, a.obs_dim, a.lastLayerTanh, a.batch_size, a.critic_l2_reg, a.clip_norm,
                      a.popart) for a in ag),
               torch.cuda.current_stream(self.device).cuda_stream)
        if sig == self._sig:
            return
        descs = [a.ddpg_desc() for a in ag]
        self.ways, groups = ddpg_population_route([(d, a.popart, r is not None, x) for d, a, r, x in zip(descs, ag, rms, ptrs)])
        self.fused = groups == [("one_workgroup", list(range(len(ag))))]
        with torch.cuda.device(self.device):
            self._groups = [(_OneWorkgroupGroup if way == "one_workgroup" else _PlanGroup)(self, way, ps, descs, views, n, batch_idx, rms)
                            for way, ps in groups]
        self._sig = sig

    # ---- evaluation and diagnostics: what a sweep's agents are compared by, one launch per phase ---------------------
    # Both calls wrap the per-agent methods' kernels (``ssc_ddpg_eval_rollout_many`` / ``ssc_ddpg_stats_many``: grid row p
    # runs agent p exactly as its own launch would) and do, object by object, the per-agent methods' host bookkeeping.
    # Unlike the learner launch they take any mix of network shapes, LayerNorm and normalize_observations.  A population
    # the launch does not serve -- an agent with normalize_returns (the Pop-Art denormalisation lives in the per-agent
    # path), mixed env kinds, shared arrays -- runs the per-agent calls; ``eval_fused`` / ``stats_fused`` tell which way
    # the last call went.  Descriptors are rebuilt only when a pointer, a shape or the stream changes.
    eval_fused = stats_fused = None

    def _out_block(self, out, cols):
        P = len(self.agents)
        if out is None:
            return torch.empty((P, cols), dtype=torch.float64, device=self.device)
        if out.dtype != torch.float64 or tuple(out.shape) != (P, cols) or not out.is_contiguous() or out.device != self.agents[0].actor_flat.device:
            raise ValueError(f"out must be a contiguous float64 [{P}, {cols}] tensor on {self.device}")
        return out

    def _workspaces(self, name, sizes):
        """one buffer, a 256-byte aligned slice per pair -> the slices"""
        offs = [0]
        for s in sizes:
            offs.append(offs[-1] + (int(s) + 255) // 256 * 256)
        ws = getattr(self, name, None)
        if ws is None or ws.numel() < offs[-1]:
            ws = torch.empty(max(offs[-1], 256), dtype=torch.uint8, device=self.device)
            setattr(self, name, ws)
        return [ws[o:o + int(s)] for o, s in zip(offs, sizes)]

    def evaluate_device(self, eval_envs, nb_eval_steps, out=None, carry_returns=False):
        """``agent.evaluate_device(eval_env, nb_eval_steps, out=out[p], carry_returns=...)`` for every (agent, eval VecEnv)
        pair -> the float64 DEVICE tensor [P, SSC_DDPG_N_EVAL], row p in ``EVAL_NAMES`` order, bit for bit what the
        per-agent call writes; every eval env's state and step counter ``t`` move as there (reset first if it never was).
        One fused launch plus one merge launch for the whole population; no transition log and no Q buffer (the per-agent
        call stays for traces).  No host read; enqueued on the current stream."""
        from .population import DeviceItems, PairCursors, served
        ag, envs = self.agents, list(eval_envs)
        K, P = int(nb_eval_steps), len(ag)
        if K < 1 or K != nb_eval_steps:
            raise ValueError("nb_eval_steps must be a positive integer")
        if len(envs) != P:
            raise ValueError("one eval env per agent")
        for a, e in zip(ag, envs):
            if e.obs_dim != a.obs_dim:
                raise ValueError(f"eval_env observes {e.obs_dim} values, the agent's networks take {a.obs_dim}")
            if e.s0.device != a.actor_flat.device:
                raise ValueError(f"eval_env lives on {e.s0.device}, the agent on {a.actor_flat.device}")
        out = self._out_block(out, _ffi.SSC_DDPG_N_EVAL)
        for e in envs:
            if e._needs_reset:
                e.reset()
        sig = (torch.cuda.current_stream(self.device).cuda_stream, out.data_ptr(),
               tuple((bytes(e.params), bytes(a._desc), bytes(a._critic_desc), float(e.action_space.low[0]), float(e.action_space.high[0]),
                      e.n, e.s0.data_ptr(), e.s1.data_ptr(), e.steps.data_ptr(), e.ep_ret.data_ptr(),
                      None if a.obs_rms is None else a._rms_block().data_ptr(), e._seed, e.env_id0, a.ret_rms is not None)
                     for a, e in zip(ag, envs)))
        if sig != getattr(self, "_eval_sig", None):
            self._eval_sig, self._eval_items, self.eval_fused = sig, None, False
            if all(a.ret_rms is None for a in ag):
                with torch.cuda.device(self.device):
                    sizes = [int(self.lib.ssc_ddpg_eval_workspace_bytes(e.n)) for e in envs]
                    ws = self._workspaces("_eval_ws", sizes)
                    items = DeviceItems(_ffi.DdpgEvalManyItem, P, self.device)
                    for p, (it, a, e) in enumerate(zip(items.items, ag, envs)):
                        it.params, it.actor, it.critic = e.params, a._desc, a._critic_desc
                        it.act_low, it.act_high = float(e.action_space.low[0]), float(e.action_space.high[0])
                        it.n, it.state = e.n, e.rollout_state(ou=False)
                        it.d_rms = None if a.obs_rms is None else a._rms_block().data_ptr()
                        it.d_out, it.d_workspace, it.workspace_bytes = out[p].data_ptr(), ws[p].data_ptr(), sizes[p]
                        it.seed, it.env_id0 = e._seed, e.env_id0
                    items.upload()
                # the library's own rules decide: a validation-only call (K = 0 launches nothing; the cursors may be any array)
                probe = (_ffi.PairCursor * P)()
                self.eval_fused = served(self.lib.ssc_ddpg_eval_rollout_many(items.h_ptr, items.d_ptr, ctypes.addressof(probe),
                                                                             items.d_ptr, P, 0, 1, None))
                if self.eval_fused:
                    self._eval_items, self._eval_keep = items, ws
                    if getattr(self, "_eval_cursors", None) is None:
                        self._eval_cursors = PairCursors(P, self.device)
        if not self.eval_fused:
            for p, (a, e) in enumerate(zip(ag, envs)):
                a.evaluate_device(e, K, out=out[p], carry_returns=carry_returns)
            return out
        cursors = self._eval_cursors.stage(step0=[e.t for e in envs])
        cursors.upload()
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_ddpg_eval_rollout_many(self._eval_items.h_ptr, self._eval_items.d_ptr, cursors.h_ptr, cursors.d_ptr,
                                                           P, K, 0 if carry_returns else 1, _ffi.stream()))
        for e in envs:
            e.t += K
        return out

    def evaluate(self, eval_envs, nb_eval_steps, **kw):
        """:meth:`evaluate_device` as a list of dicts by ``EVAL_NAMES``, one per agent.  Reads the device block (one device ->
        host copy for the population)."""
        rows = self.evaluate_device(eval_envs, nb_eval_steps, **kw).cpu().tolist()
        return [a.eval_dict(r) for a, r in zip(self.agents, rows)]

    def get_stats_device(self, replays=None, out=None):
        """``agent.get_stats_device(replay, out=out[p])`` for every agent -> the float64 DEVICE tensor
        [P, SSC_DDPG_N_STATS], row p in ``STATS_NAMES`` order, bit for bit what the per-agent call writes.  An agent without
        a fixed sample draws and keeps ``batch_size`` records of its replay (``replays[p]``, default its own buffer) exactly
        as its own call would; one whose replay holds fewer has no sample yet: it is skipped and row p of ``out`` is left as
        it is (NaN in a block this call allocates).  Two launches for the whole population; no host read."""
        from .population import DeviceItems
        ag, P = self.agents, len(self.agents)
        replays = [None] * P if replays is None else list(replays)
        if len(replays) != P:
            raise ValueError("one replay (or None) per agent")
        out = torch.full((P, _ffi.SSC_DDPG_N_STATS), float("nan"), dtype=torch.float64, device=self.device) if out is None \
            else self._out_block(out, _ffi.SSC_DDPG_N_STATS)
        have = []
        for a, r in zip(ag, replays):
            if getattr(a, "stats_sample", None) is None:
                r = a.replay_buffer if r is None else r
                if len(r) >= a.batch_size:
                    a._draw_stats_sample(r)
            have.append(getattr(a, "stats_sample", None) is not None)
        noisy = [a.param_noise is not None for a in ag]
        sig = (torch.cuda.current_stream(self.device).cuda_stream, out.data_ptr(),
               tuple((bytes(a._desc), bytes(a._critic_desc), bytes(a._perturbed_desc) if pn else None,
                      a.d_param_noise_stddev.data_ptr() if pn else None,
                      (a.stats_sample[0].data_ptr(), a.stats_sample[1].data_ptr(), a.stats_sample[0].shape[0]) if h else None,
                      None if a.obs_rms is None else a._rms_block().data_ptr(), a.ret_rms is not None)
                     for a, pn, h in zip(ag, noisy, have)))
        if sig != getattr(self, "_stats_sig", None):
            self._stats_sig, self._stats_items = sig, None
            self.stats_fused = all(a.ret_rms is None for a in ag) and all(a.device == self.device for a in ag)
            if self.stats_fused:
                with torch.cuda.device(self.device):
                    m = [a.stats_sample[0].shape[0] if h else 0 for a, h in zip(ag, have)]
                    sizes = [int(self.lib.ssc_ddpg_stats_workspace_bytes(k)) for k in m]
                    ws = self._workspaces("_stats_ws", sizes)
                    items = DeviceItems(_ffi.DdpgStatsManyItem, P, self.device)
                    for p, (it, a) in enumerate(zip(items.items, ag)):
                        it.actor, it.critic, it.m = a._desc, a._critic_desc, m[p]
                        if noisy[p]:
                            it.perturbed, it.has_perturbed = a._perturbed_desc, 1
                            it.d_param_noise_stddev = a.d_param_noise_stddev.data_ptr()
                        if have[p]:
                            it.d_obs, it.d_act = a.stats_sample[0].data_ptr(), a.stats_sample[1].data_ptr()
                        it.d_rms = None if a.obs_rms is None else a._rms_block().data_ptr()
                        it.d_out, it.d_workspace, it.workspace_bytes = out[p].data_ptr(), ws[p].data_ptr(), sizes[p]
                    items.upload()
                self._stats_items, self._stats_keep = items, ws
        if not self.stats_fused:
            for p, (a, r) in enumerate(zip(ag, replays)):
                if have[p]:
                    a.get_stats_device(r, out=out[p])
            return out
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_ddpg_stats_many(self._stats_items.h_ptr, self._stats_items.d_ptr, P, _ffi.stream()))
        return out

    # ---- parameter-space noise: the adaption interval of every noisy agent in one launch ---------------------------
    # ``ssc_param_noise_cycle_many``: workgroup j runs noisy agent j exactly as ``agent.param_noise_cycle`` (or, while its ring
    # holds no batch, ``agent.perturb_policy``) would; the batch is gathered out of the ring inside the kernel, from indices
    # that ONE ``ssc_replay_sample_many`` draws for all rings.  Any mix of shapes, LayerNorm and normalize_observations.
    pn_fused = None
    _pn_sig = None

    def param_noise_plan(self, replays):
        """The host half of :meth:`param_noise_cycle`, moving nothing: per agent with parameter noise its index ``p``, the
        interval (``m`` = batch_size when its ring holds a batch, else 0: perturb only), the generations the interval draws
        and the key (seed, counter0, size) of the ONE index batch ``replay.sample_indices(1, batch_size)`` would draw."""
        plan = []
        for p, (a, r) in enumerate(zip(self.agents, replays)):
            if a.param_noise is None:
                continue
            g = int(a.param_noise_generation)
            if len(r) >= a.batch_size:
                plan.append(dict(p=p, m=int(a.batch_size), generation_adaptive=g, generation_acting=g + 1,
                                 key=(int(r.seed), int(r._batches_drawn), len(r))))
            else:
                plan.append(dict(p=p, m=0, generation_adaptive=g, generation_acting=g, key=None))
        return plan

    def param_noise_commit(self, plan, replays):
        """What the planned intervals consume, once they are enqueued: two generations and one batch of the ring's index
        stream where the stddev is adapted, one generation where not; ``perturbed_generation`` is the acting one."""
        for e in plan:
            a = self.agents[e["p"]]
            a.perturbed_generation = e["generation_acting"]
            a.param_noise_generation = e["generation_acting"] + 1
            if e["key"] is not None:
                replays[e["p"]]._batches_drawn += 1

    def param_noise_cycle(self, replays, dsts=None):
        """``rl_train.adapt_and_perturb(agent, replay, dst, cycle=True)`` for every agent that has ``param_noise`` (the others
        are not in the launch): the stddev adapted on the obs0 of ONE fresh batch of the agent's ring, then ``dsts[p]``
        (default ``agent.perturbed_actor_flat``) = actor + noise of the adapted stddev; only the perturbation while the ring
        holds fewer than ``batch_size`` records.  Generations, ``perturbed_generation`` and every ring's index stream move
        exactly as there, and every array holds the same bits.  One sampling launch and one cycle launch for the whole
        population; in steady state a call uploads the sampling keys and the cursors (24 bytes per agent) and nothing
        else.  A population the launch does not serve -- a ``batch_size`` above 64 or not the same for all noisy agents (the
        one-wave sampler), agents on different devices, an agent without ``param_noise_cycle``, a refusal by the library's
        own validation -- runs the per-agent calls; ``pn_fused`` tells which way the last call went.  Stream-ordered, no
        host read."""
        from .population import served
        from .rl_train import adapt_and_perturb
        ag, P = self.agents, len(self.agents)
        replays = list(replays)
        dsts = [None] * P if dsts is None else list(dsts)
        if len(replays) != P or len(dsts) != P:
            raise ValueError("one replay ring (and one dst or None) per agent")
        plan = self.param_noise_plan(replays)
        if not plan:
            return
        noisy = [e["p"] for e in plan]
        out = [ag[p].perturbed_actor_flat if dsts[p] is None else dsts[p] for p in noisy]
        for p, d in zip(noisy, out):
            if d.dtype != torch.float32 or d.numel() != ag[p].actor_flat.numel() or not d.is_contiguous():
                raise ValueError("dst must be a contiguous fp32 array of the size of actor_flat")
        active = tuple(j for j, e in enumerate(plan) if e["m"] > 0)
        rms = [ag[p]._rms_block() for p in noisy]
        sig = (POPULATION_FUSED_PARAM_NOISE, torch.cuda.current_stream(self.device).cuda_stream, active,
               tuple((bytes(a._desc), a.actor_flat.data_ptr(), a.actor_flat.numel(), d.data_ptr(), r.s.data_ptr(), r.s.shape[0],
                      None if b is None else b.data_ptr(), tuple(a._pn_skip), a.param_noise_seed,
                      a.param_noise.desired_action_stddev, a.param_noise.adoption_coefficient, a.d_param_noise_stddev.data_ptr(),
                      a.d_param_noise_distance.data_ptr(), a.batch_size, str(a.actor_flat.device), str(r.s.device))
                     for a, d, r, b in zip((ag[p] for p in noisy), out, (replays[p] for p in noisy), rms)))
        if sig != self._pn_sig:
            self._pn_sig, self._pn = sig, None
            B = ag[noisy[0]].batch_size
            self.pn_fused = (POPULATION_FUSED_PARAM_NOISE and B <= 64 and all(ag[p].batch_size == B for p in noisy)
                             and all(hasattr(ag[p], "param_noise_cycle") for p in noisy)
                             and all(ag[p].actor_flat.device == ag[noisy[0]].actor_flat.device == replays[p].s.device for p in noisy))
            if self.pn_fused:
                n = len(noisy)
                with torch.cuda.device(self.device):
                    st = dict(items=DeviceItems(_ffi.ParamNoiseManyItem, n, self.device),
                              cursors=DeviceItems(_ffi.ParamNoiseCursor, n, self.device),
                              draw=IndexDraw(max(len(active), 1), 1, B, self.device))
                    for j, (it, p, d) in enumerate(zip(st["items"].items, noisy, out)):
                        a, r = ag[p], replays[p]
                        it.actor, it.d_obs = a._desc, r.s.data_ptr()
                        it.d_idx = st["draw"].idx[active.index(j)].data_ptr() if j in active else None
                        it.d_rms = None if rms[j] is None else rms[j].data_ptr()
                        it.n, it.d_src = a.actor_flat.numel(), a.actor_flat.data_ptr()
                        it.skip0_begin, it.skip0_end, it.skip1_begin, it.skip1_end = a._pn_skip
                        it.seed, it.desired, it.coefficient = a.param_noise_seed, a.param_noise.desired_action_stddev, a.param_noise.adoption_coefficient
                        it.d_stddev, it.d_distance = a.d_param_noise_stddev.data_ptr(), a.d_param_noise_distance.data_ptr()
                        it.d_dst = d.data_ptr()
                    st["items"].upload()
                self._pn = st
        if self.pn_fused:
            st = self._pn
            st["cursors"].wait()
            for c, e in zip(st["cursors"].items, plan):
                c.generation_adaptive, c.generation_acting, c.m = e["generation_adaptive"], e["generation_acting"], e["m"]
            st["cursors"].upload()
            with torch.cuda.device(self.device):
                if active:
                    st["draw"].draw([plan[j]["key"] for j in active])
                # the library's own rules decide: validation precedes every HIP call, so a refusal has launched nothing
                self.pn_fused = served(self.lib.ssc_param_noise_cycle_many(st["items"].h_ptr, st["items"].d_ptr, st["cursors"].h_ptr,
                                                                           st["cursors"].d_ptr, len(noisy), _ffi.stream(self.device)))
            if self.pn_fused:
                self.param_noise_commit(plan, replays)
                return
        for p in noisy:
            adapt_and_perturb(ag[p], replays[p], dst=dsts[p], cycle=True)

    def get_stats(self, replays=None):
        """:meth:`get_stats_device` as a list of dicts, one per agent, each what ``agent.get_stats`` returns (an agent
        without a sample yet: only what does not come from the block).  Reads the device block (one device -> host copy)."""
        rows = self.get_stats_device(replays).cpu().tolist()
        res = []
        for a, r in zip(self.agents, rows):
            stats = a.stats_dict(r)
            if a.ret_rms is not None:                            # setup_stats lists ret_rms first (ddpg_editted.py:223-225)
                mean, std = a.ret_rms.mean_std()
                stats = {"ret_rms_mean": float(mean[0]), "ret_rms_std": float(std[0]), **stats}
            if a.param_noise is not None:
                stats = {**stats, **a.param_noise.get_stats()}
            res.append(stats)
        return res


# ---------------------------------------------------------------------------- navigator --
def add_noise(data_inp, noiseToSignal, rng=None):
    """NN_Dynamics_Model/helper_funcs.py:10-17: per column, Gaussian noise of std ``mean(column) * noiseToSignal``
    -- applied only where that product is > 0, so columns with a negative or zero mean get none (the
    reference's behaviour, kept)."""
    rng = rng if rng is not None else np.random
    data = np.array(data_inp, dtype=np.float64, copy=True)
    if data.size == 0:
        return data
    std_of_noise = np.mean(data, axis=0) * noiseToSignal
    for j in range(std_of_noise.shape[0]):
        if std_of_noise[j] > 0:
            data[:, j] = data[:, j] + rng.normal(0, np.absolute(std_of_noise[j]), (data.shape[0],))
    return data


def init_dynamics_weights(in_dim, out_dim, num_fc_layers, depth_fc_layers, generator=None):
    """xavier-NORMAL weights and biases (feedforward_network.py:8, 14-23)."""
    dims = [in_dim] + [depth_fc_layers] * num_fc_layers + [out_dim]
    Ws, bs = [], []
    for i in range(len(dims) - 1):
        Ws.append(torch.randn((dims[i], dims[i + 1]), generator=generator) * float(np.sqrt(2.0 / (dims[i] + dims[i + 1]))))
        bs.append(torch.randn(dims[i + 1], generator=generator) * float(np.sqrt(2.0 / (1 + dims[i + 1]))))
    return Ws, bs


class NND_MB_agent(NavigationRLAgent):
    """The SmartStart navigator (smartstart/RLAgents/NND_MB_agent.py): MPC over a learned dynamics
    model -- sample ``num_control_samples`` action sequences of length ``horizon``, forward-simulate
    them (``ssc_dyn_forward_sim``), score waypoint progress (``ssc_mpc_score``), execute the first action
    of the best sequence plus small Gaussian noise (``ssc_mpc_select_action``)."""

    noiseToSignal = 0.01
    actions_ag = 'nc'

    def __init__(self, env, sess=None, replay_buffer=None, BUFFER_SIZE=10000,
                 final_steps=10, steps_per_waypoint=1, mean_per_stepsize=1, std_per_stepsize=1,
                 stepsizes_in_waypoint_radii=1,
                 gamma=.75, horizontal_penalty_factor=.5, horizon=20, num_control_samples=5000, path_shortcutting=True,
                 steps_before_giving_up_on_waypoint=5,
                 num_fc_layers=1, depth_fc_layers=500,
                 training_data=None, weights=None, biases=None, norm=None,
                 make_aggregated_dataset_noisy=True, nEpochs=30, fraction_use_new=0.9,
                 num_episodes_for_aggregation=3,
                 save_dir_name="save_untitled", load_dir_name="untitled_load", model_root=None,
                 save_training_data=False, load_existing_training_data=False,
                 save_resulting_dynamics_model=False, load_existing_dynamics_model=False,
                 make_training_dataset_noisy=True, num_rollouts_train=25, num_rollouts_val=20,
                 steps_per_rollout_train=333, steps_per_rollout_val=333,
                 device="cuda", precision="bf16_mfma", seed=1234, per_row_projection=False, noise_stream=0, **unused):
        self.env = env
        self.noise_stream = int(noise_stream)   # which pair of Philox streams add_noise draws the data set's noise from
        self.device = torch.device(device)
        self.replay_buffer = replay_buffer if replay_buffer is not None else ReplayBuffer(self, BUFFER_SIZE)
        self.final_steps, self.steps_per_waypoint = final_steps, steps_per_waypoint
        self.mean_per_stepsize, self.std_per_stepsize = mean_per_stepsize, std_per_stepsize
        self.stepsizes_in_waypoint_radii = stepsizes_in_waypoint_radii
        self.gamma, self.horizontal_penalty_factor = gamma, horizontal_penalty_factor
        self.horizon, self.N = horizon, num_control_samples
        self.path_shortcutting = path_shortcutting
        self.steps_before_giving_up_on_waypoint = steps_before_giving_up_on_waypoint
        self.make_aggregated_dataset_noisy = make_aggregated_dataset_noisy   # NND_MB_agent.py:66
        self.nEpochs, self.fraction_use_new = nEpochs, fraction_use_new      # :64, :68
        self.num_episodes_for_aggregation = num_episodes_for_aggregation     # :65
        self.num_episodes_finished = 0
        self.theta = 1                      # NND_MB_agent.py:143
        self.noise_amount = 0.005           # :188-191
        self.per_row_projection = per_row_projection
        self.seed, self._t = int(seed), 0
        state_dim = env.observation_space.shape[0]
        act_dim = env.action_space.shape[0]
        self._train_inputs = self._train_outputs = None
        self.states_val = self.controls_val = None
        # the reference keeps its data under <models>/NND_MB_agent/<dir_name>/training_data (:35-44, :181-185)
        root = model_root if model_root is not None else os.path.join(os.getcwd(), "models", "NND_MB_agent")
        self.load_dir, self.save_dir = os.path.join(root, load_dir_name), os.path.join(root, save_dir_name)
        if load_existing_training_data and training_data is None:
            # :203-213 -- e.g. the reference's own models/NND_MB_agent/default/training_data/*.npy
            d = os.path.join(self.load_dir, "training_data")
            training_data = {k: np.load(os.path.join(d, k + ".npy")) for k in ("dataX", "dataY", "dataZ")}
            self.states_val = np.load(os.path.join(d, "states_val.npy"), allow_pickle=True)
            self.controls_val = np.load(os.path.join(d, "controls_val.npy"), allow_pickle=True)
        if norm is None and training_data is None:
            norm = self._collect_training_data(num_rollouts_train, steps_per_rollout_train, num_rollouts_val,
                                               steps_per_rollout_val, make_training_dataset_noisy)
        elif norm is None:
            norm = self.normalisation_from_data(training_data["dataX"], training_data["dataY"], training_data["dataZ"])
        if training_data is not None:
            # z-scored (x, y) -> z training set (NND_MB_agent.py:302-319)
            with np.errstate(divide="ignore", invalid="ignore"):
                nz = lambda v, m, s: np.nan_to_num((np.asarray(v, np.float64) - m) / s)
                self._train_inputs = np.concatenate([nz(training_data["dataX"], norm["mean_x"], norm["std_x"]),
                                                     nz(training_data["dataY"], norm["mean_y"], norm["std_y"])], axis=1)
                self._train_outputs = nz(training_data["dataZ"], norm["mean_z"], norm["std_z"])
        if save_training_data:                                                  # :289-296
            d = os.path.join(self.save_dir, "training_data")
            os.makedirs(d, exist_ok=True)
            src = training_data if training_data is not None else \
                {k: getattr(self, k).double().cpu().numpy() for k in ("dataX", "dataY", "dataZ")}
            for k in ("dataX", "dataY", "dataZ"):
                np.save(os.path.join(d, k + ".npy"), np.asarray(src[k], np.float64))
            if self.states_val is not None:
                def stacked(rollouts):       # equal-length rollouts stack; ragged ones (a rollout hit a terminal state)
                    same = len({len(r) for r in rollouts}) <= 1          # become an object array, as numpy 1.15 made them
                    if same:
                        return np.asarray(rollouts)
                    out = np.empty(len(rollouts), dtype=object)
                    for i, r in enumerate(rollouts):
                        out[i] = np.asarray(r)
                    return out
                np.save(os.path.join(d, "states_val.npy"), stacked(self.states_val), allow_pickle=True)
                np.save(os.path.join(d, "controls_val.npy"), stacked(self.controls_val), allow_pickle=True)
        if weights is None:
            gen = torch.Generator().manual_seed(self.seed)
            weights, biases = init_dynamics_weights(state_dim + act_dim, state_dim, num_fc_layers, depth_fc_layers, gen)
        self.dyn_model = navigator.DynamicsModel(weights, biases, norm, state_dim, act_dim, device=device,
                                                 precision=precision)
        self.state_dim, self.act_dim = state_dim, act_dim
        self.save_resulting_dynamics_model = save_resulting_dynamics_model   # :179
        self.use_existing_dynamics_model = load_existing_dynamics_model      # :158
        self.desired_states = None
        self.radii = None                   # NND_MB_agent.py:168
        self.param_dict = None

    def _collect_training_data(self, num_rollouts_train, steps_per_rollout_train, num_rollouts_val,
                               steps_per_rollout_val, make_training_dataset_noisy):
        """The constructor's data-collection branch (NND_MB_agent.py:215-319) with everything resident in HBM:
        random-policy rollouts (one fused launch), (s, a, s' - s) formatting, optional ``add_noise`` on states and
        deltas (:263-266), column statistics and z-scoring.  Leaves ``dataX / dataY / dataZ`` (raw, device),
        the z-scored training matrices, ``states_val / controls_val`` (host lists like the reference keeps) and
        returns the ``norm`` dict."""
        from . import collect_samples as cs
        collector = cs.CollectSamples(self.env, cs.Policy_Random(self.env), seed=self.seed)
        train = collector.collect_dataset(num_rollouts_train, steps_per_rollout_train)
        if len(train) == 0:
            raise ValueError("the random rollouts produced no training rows")
        self.states_val, self.controls_val, _, _ = collector.collect_samples(num_rollouts_val, steps_per_rollout_val)
        if make_training_dataset_noisy:
            cs.add_noise_device(train.dataX, self.noiseToSignal, self.seed, stream_id=2 * self.noise_stream)
            cs.add_noise_device(train.dataZ, self.noiseToSignal, self.seed, stream_id=2 * self.noise_stream + 1)
        self.dataX, self.dataY, self.dataZ = train.dataX, train.dataY, train.dataZ
        (mx, sx), (my, sy), (mz, sz) = (cs.column_stats(v) for v in (train.dataX, train.dataY, train.dataZ))
        host = lambda t: t.cpu().numpy()
        norm = dict(mean_x=host(mx), std_x=host(sx), mean_y=host(my), std_y=host(sy), mean_z=host(mz), std_z=host(sz))
        self._train_inputs, self._train_outputs = train.normalised(norm)  # :302-319, np.concatenate((dataX, dataY), axis=1)
        return norm

    @staticmethod
    def normalisation_from_data(dataX, dataY, dataZ):
        """NND_MB_agent.py:302-315 (mean / std per column)."""
        X, Y, Z = (np.asarray(v, np.float64) for v in (dataX, dataY, dataZ))
        return dict(mean_x=X.mean(0), std_x=(X - X.mean(0)).std(0), mean_y=Y.mean(0), std_y=(Y - Y.mean(0)).std(0),
                    mean_z=Z.mean(0), std_z=(Z - Z.mean(0)).std(0))

    # ---- planning (host, once per episode) -----------------------------------------------------
    def start_new_episode_plan(self, starting_state, path_to_follow):
        """NND_MB_agent.py:375-423, including the retraining of the dynamics model on the aggregated replay-buffer
        transitions every ``num_episodes_for_aggregation`` planned episodes (:420-423; the very first plan trains
        too).  An agent built from ``norm`` statistics alone has no initial data set and skips the training."""
        self.current_desired_state_index = 0
        self.actions_done_for_current_waypoint = 0
        stds, means = path_deltas_stds_and_means_per_dim(path_to_follow)
        self.stds = stds
        self.radii = radii_calc(means, stds, self.mean_per_stepsize, self.std_per_stepsize,
                                self.stepsizes_in_waypoint_radii)
        self.distance_function = elliptical_euclidean_distance_function_generator(self.radii)
        if self.path_shortcutting:
            self.path_to_follow = path_shortcutter(path_to_follow, self.distance_function, self.theta)
        else:
            self.path_to_follow = np.asarray(path_to_follow, np.float64)
        self.desired_states = np.asarray(get_start_waypoints_final_states_steps(self.path_to_follow,
                                                                                self.steps_per_waypoint))
        self.distances_left = distances_left(self.desired_states, self.distance_function)
        self._problems = None
        can_train = self._train_inputs is not None or self.use_existing_dynamics_model
        if can_train and self.num_episodes_finished % self.num_episodes_for_aggregation == 0:
            self.train_dynamics_model()                                       # :421-422
        self.num_episodes_finished += 1

    @property
    def current_desired_state(self):
        return self.desired_states[self.current_desired_state_index]

    @property
    def next_desired_state(self):
        return self.desired_states[min(self.current_desired_state_index + 1, len(self.desired_states) - 1)]

    def move_to_next(self, pt, desired_state_index, distance_to_curr, distance_to_next):
        """:491-496"""
        return np.logical_and(np.logical_or(distance_to_curr <= self.theta, distance_to_next <= distance_to_curr),
                              desired_state_index != len(self.desired_states) - 1)

    def close_enough_to_goal(self, current_state):
        """:425-432"""
        if self.distance_function(current_state, self.desired_states[-1]) <= self.theta:
            return True
        return self.current_desired_state_index == len(self.desired_states) - 1 and \
            self.final_steps <= self.actions_done_for_current_waypoint

    # ---- acting (GPU, every step) --------------------------------------------------------------
    def get_action(self, state):
        return self.get_action_with_predicted_states(state)[0]

    def get_best_sim_actions(self, curr_nn_state):
        """:498-520 -> (best_action, best_sim_number, best_sequence, best_path) and the device tensors."""
        low, high = self.env.action_space.low, self.env.action_space.high
        A = navigator.mpc_sample_actions(1, self.N, self.horizon, low, high, self.seed, 0, self._t, self.device)
        S = self.dyn_model.do_forward_sim(np.asarray(curr_nn_state, np.float32), A)
        wp = self.desired_states
        if len(wp) < 2:   # the reference would raise IndexError at desired_states[b + 1]
            wp = np.concatenate([wp, wp], axis=0)
            left = np.asarray([0.0, 0.0])
        else:
            left = self.distances_left
        ps = navigator.MpcProblemSet([wp], [left], [self.radii], [self.current_desired_state_index],
                                     device=self.device, theta=self.theta, gamma=self.gamma,
                                     horizontal_penalty_factor=self.horizontal_penalty_factor,
                                     per_row_projection=self.per_row_projection)
        scores, best, _ = navigator.mpc_score(ps, S)
        return A, S, scores, best

    def get_action_with_predicted_states(self, state):
        """:339-358"""
        self.actions_done_for_current_waypoint += 1
        A, S, scores, best = self.get_best_sim_actions(state)
        noise = self.noise_amount if self.actions_ag in ('nn', 'nc') else 0.0
        action, path = navigator.mpc_select_action(A, S, best, 1, noise, self.seed, 0, self._t)
        self._t += 1
        return action[0].double().cpu().numpy(), path[0].double().cpu().numpy()

    def observe(self, state, action, reward, new_state, done):
        """:360-373"""
        self.replay_buffer.add(self, state, action, reward, done, new_state)
        distance_to_current = self.distance_function(new_state, self.current_desired_state)
        distance_to_next = self.distance_function(new_state, self.next_desired_state)
        if self.move_to_next(new_state, self.current_desired_state_index, distance_to_current, distance_to_next) or \
                (self.actions_done_for_current_waypoint > self.steps_before_giving_up_on_waypoint and
                 self.current_desired_state_index != len(self.desired_states) - 1):
            self.current_desired_state_index += 1
            self.actions_done_for_current_waypoint = 0

    def render(self, env, **kwargs):
        env.render()

    def get_param_dict(self):
        return self.param_dict

    def aggregated_dataset(self, rng=None):
        """NND_MB_agent.train_dynamics_model :442-460: the replay buffer's (s, a, s2 - s) rows, optionally with
        ``add_noise`` on states and deltas (:451-453), z-scored with the statistics of the initial data set."""
        if len(self.replay_buffer) == 0:
            s = np.zeros((0, self.state_dim)); a = np.zeros((0, self.act_dim)); s2 = np.zeros((0, self.state_dim))
        else:
            s, a, _, _, s2 = self.replay_buffer.all_batch()
            s, a, s2 = (np.asarray(v, np.float64).reshape(len(s), -1) for v in (s, a, s2))
        new_x, new_z = s, s2 - s
        if self.make_aggregated_dataset_noisy:
            new_x = add_noise(new_x, self.noiseToSignal, rng)
            new_z = add_noise(new_z, self.noiseToSignal, rng)
        nm = self.dyn_model.norm
        col = lambda name, n: np.asarray([getattr(nm, name)[i] for i in range(n)], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            nz = lambda v, m, sd: np.nan_to_num((v - m) / sd)
            x = nz(new_x, col("mean_x", self.state_dim), col("std_x", self.state_dim))
            y = nz(a, col("mean_y", self.act_dim), col("std_y", self.act_dim))
            z = nz(new_z, col("mean_z", self.state_dim), col("std_z", self.state_dim))
        return np.concatenate([x, y], axis=1), z

    def train_dynamics_model(self, dataX_new=None, dataZ_new=None, nEpoch=None, fraction_use_new=None, batchsize=512,
                             lr=0.001, rng=None):
        """NND_MB_agent.train_dynamics_model (:437-480; no TF saver): trains the model on the stored
        (normalised) initial data set mixed with the aggregated rows through ``Dyn_Model.train``'s batching
        (DynamicsModel.train -> ssc_mlp_train_step).  Without arguments the aggregated rows come from the
        replay buffer exactly as in the reference (``aggregated_dataset``); ``dataX_new`` / ``dataZ_new`` pass
        already normalised (x||y, z) rows instead."""
        if self.use_existing_dynamics_model:                     # :463-468: restore instead of training
            self.dyn_model.load(os.path.join(self.load_dir, "models", "finalModel.npz"))
            return 0
        args = self._dynamics_training_args(dataX_new, dataZ_new, nEpoch, fraction_use_new, rng)
        loss = self.dyn_model.train(*args, batchsize=batchsize, lr=lr, rng=rng)
        self._save_trained_dynamics_model()
        return loss

    def _dynamics_training_args(self, dataX_new, dataZ_new, nEpoch, fraction_use_new, rng):
        """(dataX, dataZ, dataX_new, dataZ_new, nEpoch, fraction_use_new) of ``DynamicsModel.train`` for this agent"""
        if self._train_inputs is None:
            raise RuntimeError("NND_MB_agent was built without training_data")
        if dataX_new is None and dataZ_new is None:
            xn, zn = self.aggregated_dataset(rng)
        else:
            in_dim, out_dim = self.dyn_model.in_dim, self.dyn_model.out_dim
            xn = np.zeros((0, in_dim)) if dataX_new is None else np.asarray(dataX_new)
            zn = np.zeros((0, out_dim)) if dataZ_new is None else np.asarray(dataZ_new)
        nEpoch = self.nEpochs if nEpoch is None else nEpoch
        fraction_use_new = self.fraction_use_new if fraction_use_new is None else fraction_use_new
        return self._train_inputs, self._train_outputs, xn, zn, nEpoch, fraction_use_new

    def _save_trained_dynamics_model(self):
        if self.save_resulting_dynamics_model:                   # :475-480 (an .npz instead of a TF checkpoint)
            d = os.path.join(self.save_dir, "models")
            os.makedirs(d, exist_ok=True)
            n_train = 1 + self.num_episodes_finished // self.num_episodes_for_aggregation
            self.dyn_model.save(os.path.join(d, "model_numTrain%d.npz" % n_train))
            self.dyn_model.save(os.path.join(d, "finalModel.npz"))


def train_dynamics_models(nnd_agents, rngs, dataX_new=None, dataZ_new=None, nEpoch=None, fraction_use_new=None, batchsize=512,
                          lr=0.001, population=None):
    """``agent.train_dynamics_model(..., rng=rngs[p])`` for every ``NND_MB_agent`` of a list (the seeds of a sweep), the
    training itself through ``navigator.DynamicsModelPopulation``: one launch per Adam step for all of them.  Per agent
    as before: ``use_existing_dynamics_model`` restores instead of training (its loss is 0), the aggregated data set is
    drawn with the agent's own rng, the trained model is saved where the agent saves it.  ``dataX_new`` / ``dataZ_new``:
    ``None`` or one entry per agent; ``nEpoch``, ``fraction_use_new``, ``batchsize``, ``lr``: one value, or one per agent.
    ``population``: a ``DynamicsModelPopulation`` over the TRAINED agents' models kept from an earlier call (its item
    tables stay on the device).  Returns the list of losses."""
    n = len(nnd_agents)
    if not isinstance(rngs, (list, tuple)) or len(rngs) != n:
        raise ValueError("train_dynamics_models: one rng per agent")
    per = lambda v, what: navigator._per_model(v, n, what)
    xs, zs = per(dataX_new, "dataX_new"), per(dataZ_new, "dataZ_new")
    epochs, fracs, sizes, lrs = per(nEpoch, "nEpoch"), per(fraction_use_new, "fraction_use_new"), per(batchsize, "batchsize"), per(lr, "lr")
    losses, train = [0] * n, []
    for p, a in enumerate(nnd_agents):
        if a.use_existing_dynamics_model:
            a.dyn_model.load(os.path.join(a.load_dir, "models", "finalModel.npz"))
        else:
            train.append(p)
    if not train:
        return losses
    args = [nnd_agents[p]._dynamics_training_args(xs[p], zs[p], epochs[p], fracs[p], rngs[p]) for p in train]
    if population is None:
        population = navigator.DynamicsModelPopulation([nnd_agents[p].dyn_model for p in train])
    elif [id(m) for m in population.models] != [id(nnd_agents[p].dyn_model) for p in train]:
        raise ValueError("train_dynamics_models: population does not hold the trained agents' models")
    got = population.train([a[:4] for a in args], [a[4] for a in args], [a[5] for a in args], batchsize=[sizes[p] for p in train],
                           lr=[lrs[p] for p in train], rngs=[rngs[p] for p in train])
    for p, loss in zip(train, got):
        losses[p] = loss
        nnd_agents[p]._save_trained_dynamics_model()
    return losses
