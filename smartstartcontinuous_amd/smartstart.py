"""``SmartStartContinuous`` (smartstart/smartexploration/smartexplorationcontinuous.py): with
probability ``eta`` an episode starts by navigating (NND_MB MPC) back to a "smart start" state
chosen by UCB1 over the critic value and a kernel-density visitation count, then hands over to the
base agent.  Same constructor keywords and RLAgent methods as the reference; selection runs on the
GPU (``ssc_critic_forward`` / ``ssc_kde_evaluate`` / ``ssc_ucb_argmax``)."""
from __future__ import annotations

import ctypes
import time

import numpy as np
import torch

from . import _ffi
from .agents import NND_MB_agent, ReplayBufferRLAgent, RLAgent
from .numerical import volume_of_n_dimensional_hyperellipsoid
from .replay_buffer import DeviceReplayBuffer, ReplayBuffer
from .vec_env import StepGraphs


def kde_scott_bandwidth(data):
    """``scipy.stats.gaussian_kde(data.T, bw_method='scott')`` bandwidth [third-party; :260]:
    covariance = cov(data, ddof=1) * n^(-2/(d+4)).  The O(|D|) moments are reduced on the device in
    fp64; the d x d algebra is host-side.  Returns (whitening [d,d] fp32, norm)."""
    x = data.double()
    n, d = x.shape
    # two-pass covariance with elementwise kernels and column sums (torch.cov goes through an f64 GEMM that takes 5.5 ms
    # for a [2, 100 000] matrix on this stack -- 85 % of a whole smart-start selection; this is ~0.1 ms)
    xc = x - x.mean(dim=0, keepdim=True)
    cov = ((xc.unsqueeze(2) * xc.unsqueeze(1)).sum(dim=0) / (n - 1)).cpu().numpy() * (n ** (-1.0 / (d + 4))) ** 2
    inv = np.linalg.inv(cov)
    wh = np.linalg.cholesky(inv).T
    norm = 1.0 / (n * np.sqrt(np.linalg.det(2 * np.pi * cov)))
    return np.ascontiguousarray(wh, np.float32), float(norm)


def kde_evaluate(data, points, whitening, norm):
    """pdf of ``points`` [m, d] under the Gaussian KDE of ``data`` [n, d] (device tensors, fp32)."""
    data = data.float().contiguous()
    points = points.float().contiguous()
    n, d = data.shape
    m = points.shape[0]
    pdf = torch.empty(m, dtype=torch.float32, device=data.device)
    wh = (ctypes.c_float * (d * d))(*np.asarray(whitening, np.float32).reshape(-1).tolist())
    with torch.cuda.device(data.device):
        _ffi.check(_ffi.lib().ssc_kde_evaluate(d, n, _ffi.ptr(data), m, _ffi.ptr(points), wh, float(norm),
                                               _ffi.ptr(pdf), _ffi.stream()))
    return pdf


def ucb_argmax(values, pdf, buffer_len, volume, exploitation_param, exploration_param):
    """:275-280 -> (ucb [m], best index tensor [1])"""
    m = values.numel()
    ucb = torch.empty(m, dtype=torch.float32, device=values.device)
    best = torch.empty(1, dtype=torch.int32, device=values.device)
    with torch.cuda.device(values.device):
        _ffi.check(_ffi.lib().ssc_ucb_argmax(m, _ffi.ptr(values.float().contiguous()), _ffi.ptr(pdf),
                                             float(exploitation_param), float(exploration_param), float(buffer_len),
                                             float(volume), _ffi.ptr(ucb), _ffi.ptr(best), _ffi.stream()))
    return ucb, best


def device_smart_start_path(replay, agent, radii, n_ss, exploitation_param=1., exploration_param=2.):
    """``get_smart_start_path`` (smartexplorationcontinuous.py:223-305) with everything up to the chosen path on the
    device: candidates from the device ring's episode index (``DeviceReplayBuffer.get_possible_smart_start_indices``),
    V = Q(s, pi(s)) (``agent.state_value_device``), the Gaussian KDE over every state in the ring, UCB1 argmax, and the
    episodic path of the winner gathered out of the ring -- the replay contents never visit the host (the reference
    re-reads its whole buffer per episode, :258-260).  -> (path [L + 1, obs_dim] device tensor, buffer index) or None."""
    if not isinstance(replay, DeviceReplayBuffer) or not replay.track_episodes:
        raise TypeError("device_smart_start_path needs a DeviceReplayBuffer(track_episodes=True)")
    if len(replay) == 0:
        return None
    idx = replay.get_possible_smart_start_indices(n_ss)                                       # :243-246
    if idx is None:
        return None
    all_states = replay.get_all_states()                                                      # :258
    wh, norm = kde_scott_bandwidth(all_states)                                                # :260
    volume = volume_of_n_dimensional_hyperellipsoid(radii) if radii is not None else 1         # :262-268
    cand = replay.s2[replay.physical(idx)]                                                     # :272-273
    values = agent.state_value_device(cand)                                                    # :274
    pdf = kde_evaluate(all_states, cand, wh, norm)                                             # :275
    _, best = ucb_argmax(values, pdf, len(replay), volume, exploitation_param, exploration_param)   # :276-280
    chosen = idx[best.long()]                                                                  # stays on the device
    return replay.get_episodic_path_to_buffer_index(chosen), chosen


class SmartStartContinuous(RLAgent):
    def __init__(self, agent, env, sess=None, buffer_size=500000, exploitation_param=1., exploration_param=2.,
                 eta=0.5, eta_decay_factor=1., n_ss=1000, print_ss_stuff=True, device="cuda", **nnd_mb_kwargs):
        """``nnd_mb_*`` keywords are forwarded to :class:`NND_MB_agent` with the prefix stripped
        (smartexplorationcontinuous.py:55-198); navigator-only extras (``nnd_mb_training_data``,
        ``nnd_mb_weights`` ...) are accepted the same way."""
        self.param_dict = dict(buffer_size=buffer_size, exploitation_param=exploitation_param,
                               exploration_param=exploration_param, eta=eta, eta_decay_factor=eta_decay_factor,
                               n_ss=n_ss, agent=agent.get_param_dict())
        self.exploitation_param, self.exploration_param = exploitation_param, exploration_param
        self.eta, self.eta_decay_factor = eta, eta_decay_factor
        self.agent, self.env = agent, env
        self.device = torch.device(device)
        if isinstance(agent, ReplayBufferRLAgent):              # :140-144
            self.replay_buffer = agent.replay_buffer
            agent.set_replay_buffer_main_agent(self)
        else:
            self.replay_buffer = ReplayBuffer(self, buffer_size)
        self.n_ss, self.print_ss_stuff = n_ss, print_ss_stuff
        self.smart_start_pathing = False
        self.smart_start_path = None
        nav_kwargs = {k[len("nnd_mb_"):]: v for k, v in nnd_mb_kwargs.items() if k.startswith("nnd_mb_")}
        unknown = [k for k in nnd_mb_kwargs if not k.startswith("nnd_mb_")]
        if unknown:
            raise TypeError("unexpected keyword arguments: %s" % unknown)
        self.nnd_mb_agent = NND_MB_agent(env, sess, replay_buffer=self.replay_buffer, device=device, **nav_kwargs)
        self.times_for_smart_start = []

    def get_param_dict(self):
        return self.param_dict

    def get_summary_name(self):
        base = self.agent.get_summary_name() if hasattr(self.agent, 'get_summary_name') else self.agent.__class__.__name__
        return "SmartStartC_" + base

    @property
    def normal_agent_pathing(self):
        return not self.smart_start_pathing

    def reduce_eta(self):
        self.eta = self.eta * self.eta_decay_factor

    # ------------------------------------------------------------------------- selection --
    def smart_start_scores(self, possible_start_indices):
        """The device part of get_smart_start_path (:256-280) -> (ucb tensor, best position)."""
        all_states = torch.as_tensor(self.replay_buffer.get_all_states(), dtype=torch.float32, device=self.device)
        wh, norm = kde_scott_bandwidth(all_states)                                            # :260
        radii = self.nnd_mb_agent.radii
        volume = volume_of_n_dimensional_hyperellipsoid(radii) if radii is not None else 1      # :262-268
        _, _, _, _, s2 = self.replay_buffer._gather(np.asarray(possible_start_indices))
        cand = torch.as_tensor(s2, dtype=torch.float32, device=self.device)                    # :272-273
        values = torch.as_tensor(self.agent.get_state_value(cand), device=self.device).reshape(-1)   # :274
        pdf = kde_evaluate(all_states, cand, wh, norm)                                         # :275
        ucb, best = ucb_argmax(values, pdf, len(self.replay_buffer), volume, self.exploitation_param,
                               self.exploration_param)                                         # :276-280
        return ucb, int(best.item())

    def get_smart_start_path(self):
        """:223-305"""
        if isinstance(self.replay_buffer, DeviceReplayBuffer):
            got = device_smart_start_path(self.replay_buffer, self.agent, self.nnd_mb_agent.radii, self.n_ss,
                                          self.exploitation_param, self.exploration_param)
            return None if got is None else [row for row in got[0].double().cpu().numpy()]
        if len(self.replay_buffer) == 0:
            return None
        possible_start_indices = self.replay_buffer.get_possible_smart_start_indices(self.n_ss)
        if possible_start_indices is None:
            return None
        _, best = self.smart_start_scores(possible_start_indices)
        return self.replay_buffer.get_episodic_path_to_buffer_index(int(possible_start_indices[best]))

    # --------------------------------------------------------------------------- RLAgent --
    def get_action(self, state):
        """:307-317"""
        if self.smart_start_pathing:
            return self.nnd_mb_agent.get_action(state)
        return self.agent.get_action(state)

    def observe(self, state, action, reward, new_state, done):
        """:319-339"""
        self.replay_buffer.add(self, state, action, reward, done, new_state)
        self.agent.observe(state, action, reward, new_state, done)
        if self.smart_start_pathing:
            self.nnd_mb_agent.observe(state, action, reward, new_state, done)
            if self.nnd_mb_agent.close_enough_to_goal(new_state):
                self.smart_start_pathing = False

    def start_new_episode(self, state):
        """:341-370"""
        self.smart_start_pathing = False
        self.smart_start_path = None
        if np.random.rand() <= self.eta:
            t0 = time.time()
            self.smart_start_path = self.get_smart_start_path()
            self.times_for_smart_start.append(time.time() - t0)
            if self.smart_start_path:
                self.nnd_mb_agent.start_new_episode_plan(state, self.smart_start_path)
                if not self.nnd_mb_agent.close_enough_to_goal(state):
                    self.smart_start_pathing = True
        self.agent.start_new_episode(state)
        self.replay_buffer.start_new_episode(self)

    def end_episode(self):
        """:372-376"""
        self.reduce_eta()
        self.agent.end_episode()
        self.smart_start_pathing = False
        self.smart_start_path = None

    def render(self, env, **kwargs):
        return env.render()


class SmartStartSelection:
    """What ONE SmartStart pair does between rollout chunks, on its own agent, replay ring, dynamics model and plan pool:
    smart-start selection and plan geometry, the acting descriptor, dynamics-model aggregation, the eta decay.  Shared by
    :class:`VecSmartStart` (one pair, a pool of its own) and the pairs of :class:`VecSmartStartPopulation` (a window of the
    population's pool each).  Needs ``env`` (step count and episode limit), ``agent``, ``model``, ``pool``, ``nav.seed`` and
    the selection / geometry settings as attributes."""

    # ------------------------------------------------------------------------- selection --
    def plan_from_path(self, path):
        """NND_MB_agent.start_new_episode_plan's geometry (NND_MB_agent.py:385-418) -> (waypoints, distances_left, radii)."""
        from .numerical import (distances_left, elliptical_euclidean_distance_function_generator,
                                get_start_waypoints_final_states_steps, path_deltas_stds_and_means_per_dim,
                                path_shortcutter, radii_calc)
        path = np.asarray(path, np.float64)
        stds, means = path_deltas_stds_and_means_per_dim(path)
        radii = radii_calc(means, stds, self.mean_per_stepsize, self.std_per_stepsize, self.stepsizes_in_waypoint_radii)
        dist = elliptical_euclidean_distance_function_generator(radii)
        if self.path_shortcutting:
            path = path_shortcutter(path, dist, self.pool.theta)
        wp = np.asarray(get_start_waypoints_final_states_steps(path, self.steps_per_waypoint))
        return wp, distances_left(wp, dist), radii

    def select_plans(self, replay):
        """One smart-start selection on the device ring (get_smart_start_path, :223-305) -> up to ``n_plans`` plans
        (waypoints, distances_left, radii) as host arrays, or None when the ring holds no complete episode start yet.
        The device part runs on the CURRENT stream (rl_train_vec_smartstart(overlap_selection=True) makes that a side
        stream) and the host reads its results; nothing here writes what a rollout in flight reads."""
        if len(replay) == 0:
            return None
        idx = replay.get_possible_smart_start_indices(self.n_ss)                                  # :243-246
        if idx is None:
            return None
        all_states = replay.get_all_states()                                                      # :258
        if self.kde_max_states is not None and all_states.shape[0] > self.kde_max_states:
            stride = -(-all_states.shape[0] // int(self.kde_max_states))
            all_states = all_states[::stride].contiguous()
        wh, norm = kde_scott_bandwidth(all_states)                                                # :260
        volume = volume_of_n_dimensional_hyperellipsoid(self.last_radii) if self.last_radii is not None else 1   # :262-268
        cand = replay.s2[replay.physical(idx)]                                                    # :272-273
        values = self.agent.state_value_device(cand)                                              # :274
        pdf = kde_evaluate(all_states, cand, wh, norm)                                            # :275
        ucb, best = ucb_argmax(values, pdf, len(replay), volume, self.exploitation_param, self.exploration_param)
        if self.n_plans == 1:
            chosen = idx[best.long()]
        else:
            chosen = idx[torch.topk(ucb, min(self.n_plans, ucb.numel())).indices]
        self.last_chosen = chosen
        plans = []
        for c in chosen.reshape(-1):
            path = replay.get_episodic_path_to_buffer_index(c.reshape(1))
            if path is None or path.shape[0] < 2:
                continue
            plans.append(self.plan_from_path(path.double().cpu().numpy()))
        return plans

    def publish_plans(self, plans):
        """Put ``plans`` on offer (writes the pool on the current stream)."""
        if plans:
            self.pool.publish(plans, now=self.env.t, min_age=(self.env.spec.max_episode_steps or 1000))
            self.last_radii = plans[0][2]
            self.selections += 1

    def refresh_plans(self, replay):
        """``select_plans`` + ``publish_plans``.  Returns the chosen buffer indices (device tensor) or None when the ring
        holds no complete episode start yet."""
        self.last_chosen = None
        plans = self.select_plans(replay)
        if plans is None:
            return None
        self.publish_plans(plans)
        return self.last_chosen

    def acting_desc(self):
        """The actor descriptor the per-step launch reads: over ``perturbed_actor_flat`` for a base agent with parameter
        noise (pi, ddpg_editted.py:256-259) -- the same pointer slots for the life of the agent, so a captured step graph
        stays valid while every perturbation changes the array's contents -- else the agent's own.  The selection
        (``state_value_device``) always evaluates the PLAIN actor: get_q_value is not an acting path."""
        a = self.agent
        return a._perturbed_desc if getattr(a, "param_noise", None) is not None else a._desc

    # ------------------------------------------------------------- dynamics-model aggregation --
    def train_dynamics_model(self, replay, max_rows=65536, n_epoch=1, batchsize=512, lr=0.001, noise_to_signal=0.0):
        """NND_MB_agent.train_dynamics_model (NND_MB_agent.py:437-480) for the vectorised loop: the navigator's model is
        retrained on transitions the envs themselves produced -- an evenly strided sample of up to ``max_rows`` records of
        the device replay ring as (s, a, s2 - s) rows (:442-449), optionally with ``add_noise`` (:451-453), z-scored with
        the model's EXISTING statistics (:455-461) -- ``n_epoch`` passes of Adam steps on the device
        (``DynamicsModel.train_steps``).  Nothing leaves HBM; the packed MFMA weight image is refreshed in place before
        the next rollout, so the captured step graph keeps reading the right bytes.  Returns the mean loss of the last
        epoch (a device -> host read) or None when the ring is still smaller than one batch."""
        from .collect_samples import TrainingSet, add_noise_device
        size = len(replay)
        if size < batchsize:
            return None
        stride = max(1, -(-size // int(max_rows)))
        sel = torch.arange(0, size, stride, device=replay.s.device)
        s, a, s2 = replay.s[sel].contiguous(), replay.a[sel].contiguous(), replay.s2[sel].contiguous()
        dz = (s2 - s).contiguous()
        if noise_to_signal:
            self._agg_calls = getattr(self, "_agg_calls", 0) + 1
            add_noise_device(s, noise_to_signal, self.nav.seed, 2 * self._agg_calls)
            add_noise_device(dz, noise_to_signal, self.nav.seed, 2 * self._agg_calls + 1)
        nm, m = self.model.norm, self.model
        norm = {k: [getattr(nm, k)[i] for i in range(n)] for k, n in (("mean_x", m.state_dim), ("std_x", m.state_dim),
                                                                       ("mean_y", m.act_dim), ("std_y", m.act_dim),
                                                                       ("mean_z", m.state_dim), ("std_z", m.state_dim))}
        X, Z = TrainingSet(s, a, dz, None, None).normalised(norm)
        rows = X.shape[0]
        n_batches = rows // batchsize
        gen = torch.Generator(device=X.device)
        gen.manual_seed(int(self.nav.seed) + 7919 * getattr(self, "_trainings", 0))
        losses = None
        for _ in range(int(n_epoch)):
            perm = torch.randperm(rows, generator=gen, device=X.device)[: n_batches * batchsize]
            losses = self.model.train_steps(X, Z, perm.view(n_batches, batchsize).to(torch.int32), lr=lr)
        self._trainings = getattr(self, "_trainings", 0) + 1
        return None if losses is None else float(losses.mean().item())

    def end_of_generation(self):
        """SmartStartContinuous.end_episode (:372-376) once per episode PER ENV: eta decays."""
        self.eta *= self.eta_decay_factor


class VecSmartStart(SmartStartSelection):
    """``SmartStartContinuous`` for the N envs of a :class:`VecEnv` at once (smartexplorationcontinuous.py:307-376,
    vectorised): every env is either navigating to a smart-start state (per-env mode 1: the NND_MB MPC picks its
    action) or handed over to the base DDPG agent (mode 0: actor + OU noise); an env that finishes an episode starts
    the next one -- inside the step kernel, without the host -- with a smart start with probability ``eta``.

    What one env does is what the scalar agent does: ``get_action`` by mode (:307-317), waypoint bookkeeping and the
    hand-over test after every navigated step (:319-339), ``start_new_episode`` on the reset state (:341-370).  What is
    batched is the smart-start SELECTION (:223-305): instead of one selection per finished episode, ``refresh_plans``
    runs it once per rollout chunk on the device replay ring (candidates, Q(s, pi(s)), Gaussian KDE, UCB1), turns the
    ``n_plans`` best candidates' episodic paths into plans (radii, optional shortcutting, waypoints, distances_left --
    NND_MB_agent.start_new_episode_plan's host geometry) and publishes them in a :class:`navigator.PlanPool`; the envs
    finishing during the chunk draw from those.  ``n_plans = 1`` is the reference's argmax for every episode that starts
    before the next refresh.  One step = five launches -- compaction of the navigating envs (``ssc_nav_compact``), actor
    forward, forward simulation drawing its own candidates, scoring (one launch for N <= 64 candidates, two above), and
    ``ssc_smartstart_rollout_step`` -- captured once as a HIP graph and replayed K times per chunk.  (Evaluating the actor
    inside the step kernel was built and measured in round 4: 42.5 us against 21.3 + 10.8 us for the two launches -- the
    step kernel is a one-wave-per-SIMD latency chain and the actor's weight fetch lengthens it; NOTEBOOK section 10.)
    """

    def __init__(self, env, agent, dyn_model, eta=0.5, eta_decay_factor=1.0, n_ss=1000, exploitation_param=1.,
                 exploration_param=2., n_plans=1, n_slots=None, w_max=None, num_control_samples=64, horizon=4,
                 noise_amount=0.005, steps_before_giving_up_on_waypoint=5, final_steps=10, theta=1.0, gamma=0.75,
                 horizontal_penalty_factor=0.5, path_shortcutting=True, mean_per_stepsize=1, std_per_stepsize=1,
                 stepsizes_in_waypoint_radii=1, steps_per_waypoint=1, chunk_steps=64, seed=1234, log_modes=False,
                 kde_max_states=500000):
        from . import navigator as nav
        if getattr(agent, "ret_rms", None) is not None:
            # the selection kernels rank candidates by the RAW critic output; with return normalisation / Pop-Art that is
            # the normalised Q, and the denormalising read-out is not in those kernels yet
            raise NotImplementedError("VecSmartStart: a base agent with normalize_returns / Pop-Art is not supported "
                                      "(the selection reads the raw critic)")
        self.env, self.agent, self.model = env, agent, dyn_model
        self.eta, self.eta_decay_factor = float(eta), float(eta_decay_factor)
        self.n_ss, self.n_plans = int(n_ss), int(n_plans)
        self.exploitation_param, self.exploration_param = exploitation_param, exploration_param
        self.path_shortcutting, self.steps_per_waypoint = path_shortcutting, steps_per_waypoint
        self.mean_per_stepsize, self.std_per_stepsize = mean_per_stepsize, std_per_stepsize
        self.stepsizes_in_waypoint_radii = stepsizes_in_waypoint_radii
        dev = env.device
        max_steps = env.spec.max_episode_steps or 1000
        w_max = int(w_max) if w_max is not None else max_steps + 1
        if n_slots is None:        # a published plan must outlive every episode that started on it
            n_slots = self.n_plans * (-(-max_steps // max(int(chunk_steps), 1)) + 2)
        self.pool = nav.PlanPool(env.n, n_slots, w_max, env.obs_dim, dev, theta=theta, gamma=gamma,
                                 horizontal_penalty_factor=horizontal_penalty_factor)
        self.nav = nav.NavigatorBatch(dyn_model, self.pool, num_control_samples=num_control_samples, horizon=horizon,
                                      action_low=env.action_space.low, action_high=env.action_space.high,
                                      noise_amount=noise_amount,
                                      steps_before_giving_up_on_waypoint=steps_before_giving_up_on_waypoint,
                                      final_steps=final_steps, seed=seed, problem_id0=env.env_id0)
        self.nav.start_idx.zero_()
        self.mode = torch.zeros(env.n, dtype=torch.uint8, device=dev)
        self.pool.active = self.mode     # the MPC launches skip the envs that are not navigating (where the kernels can)
        # ... and spend their threads on the navigating envs only: every step starts by compacting ``mode`` into a list
        # (``ssc_nav_compact``); simulation (fused small-network kernel) and scoring (one-launch scorer) then cover
        # list[0 .. count) with the launch geometry of all envs (HIP-graph safe: blocks past the count exit at once).
        # The step kernel -- the last launch of a step -- leaves the counter at zero for the next step.
        self.live_list = torch.zeros(env.n, dtype=torch.int32, device=dev)
        self.n_live = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pool.live_list, self.pool.n_live = self.live_list, self.n_live
        self.actor_out = torch.zeros((env.n, 1), dtype=torch.float32, device=dev)
        self.d_eta = torch.tensor([self.eta], dtype=torch.float32, device=dev)
        self.d_eps = torch.tensor([0.0], dtype=torch.float32, device=dev)
        self.log_modes = bool(log_modes)
        # The reference estimates the visitation density from EVERY state in its buffer (<= 100 000 there, :258-260); a
        # device ring sized for 65 536 envs holds tens of millions, and the n_ss x |D| kernel then is most of a selection.
        # kde_max_states bounds |D| by an evenly strided subsample of the ring (a density estimate does not depend on the
        # sample count).  Default 500 000 = the reference's own replay capacity (SmartStartContinuous(buffer_size=500000),
        # :55), i.e. the most states its KDE can ever see; None = every state in the ring.
        self.kde_max_states = kde_max_states
        self.mode_log = None
        self.last_radii = None
        self._graphs = StepGraphs(keep=4)
        self.selections = 0

    # ------------------------------------------------------------------------------ steps --
    def _step_struct(self, chunk_k):
        e, a = self.env, self.agent
        ss = _ffi.SmartStartStep()
        ss.mode, ss.plan_of = self.mode.data_ptr(), self.pool.plan_of.data_ptr()
        ss.d_actor_out, ss.d_eta, ss.d_ou_epsilon = self.actor_out.data_ptr(), self.d_eta.data_ptr(), self.d_eps.data_ptr()
        ss.d_pool = self.pool.pool.data_ptr()
        n = a.decaying_ou_action_noise
        ss.ou.mu, ss.ou.sigma, ss.ou.theta, ss.ou.dt = float(a.ou["mu"]), float(a.ou["sigma"]), float(a.ou["theta"]), float(n.dt)
        ss.act_low, ss.act_high = float(e.action_space.low[0]), float(e.action_space.high[0])
        ss.d_n_live = self.n_live.data_ptr()
        if self.log_modes:
            if self.mode_log is None or self.mode_log.shape != (chunk_k, e.n):
                self.mode_log = torch.zeros((chunk_k, e.n), dtype=torch.uint8, device=e.device)
            ss.d_mode_log, ss.mode_log_stride = self.mode_log.data_ptr(), e.n
        return ss

    def graph_key(self, K, chunk, ring):
        """The navigator's key (``NavigatorBatch.graph_key``) plus everything this class's own launches bake into a captured
        ``fused_step``: the acting actor's descriptor by value (ten pointers, dims, flags), the observation statistics
        block, the mode / plan-pool / live-list / hand-over tensors, the mode log, the OU scalars and the action bounds.
        tests/test_gpu_smartstart_vec.py (test_graph_keys_cover_what_the_step_launches_bake_in) lists them all and
        replaces them one at a time: what a launch starts to use belongs here AND there."""
        ptr = lambda t: None if t is None else t.data_ptr()
        e, a, p = self.env, self.agent, self.pool
        rms = getattr(a, "obs_rms", None)
        return (K, self.nav.graph_key(e, chunk, ring), bytes(self.acting_desc()), None if rms is None else ptr(rms.block),
                tuple(ptr(x) for x in (self.mode, p.plan_of, p.wp_len, p.pool, p.active, p.live_list, p.n_live, self.live_list,
                                       self.n_live, self.actor_out, self.d_eps, self.d_eta, self.mode_log)), self.log_modes,
                float(a.ou["mu"]), float(a.ou["sigma"]), float(a.ou["theta"]), float(a.decaying_ou_action_noise.dt),
                float(e.action_space.low[0]), float(e.action_space.high[0]))

    def fused_step(self, chunk, ring):
        """Enqueue ONE step for every env (five launches); step index and log row are device counters."""
        from . import navigator as nav
        env, b, lib = self.env, self.nav, _ffi.lib()
        fb = b._fused_buffers(env.device)
        with torch.cuda.device(env.device):
            _ffi.check(lib.ssc_nav_compact(env.n, _ffi.ptr(self.mode), _ffi.ptr(self.live_list), _ffi.ptr(self.n_live), _ffi.stream()))
            rms = getattr(self.agent, "obs_rms", None)
            desc = self.acting_desc()
            if rms is None:
                _ffi.check(lib.ssc_actor_forward(ctypes.byref(desc), env.n, _ffi.ptr(fb["plan"]),
                                                 _ffi.ptr(self.actor_out), _ffi.stream()))
            else:   # normalize_observations: the kernel reads the block at launch (valid inside the captured graph)
                _ffi.check(lib.ssc_actor_forward_rms(ctypes.byref(desc), env.n, _ffi.ptr(fb["plan"]),
                                                     _ffi.ptr(self.actor_out), _ffi.stream(), _ffi.ptr(rms.block)))
        sp = nav.mpc_sampling(b.N, b.low, b.high, b.seed, b.problem_id0, 0, t_base=fb["t"], active=self.mode,
                              live_list=self.live_list, n_live=self.n_live)
        S = self.model.do_forward_sim_sampled(fb["plan"], sp, b.P * b.N, b.H, out=b._S, A_out=fb["A"])
        ss = self._step_struct(chunk.K if chunk is not None else 1)
        b._score_and_step(env, chunk, ring, S, lib.ssc_smartstart_rollout_step, ctypes.byref(ss))

    def _state_tensors(self):
        e, b = self.env, self.nav
        fb = b._fused_buffers(e.device)
        return [e.s0, e.s1, e.steps, e.ep_ret, e.ou_x, e.stats, self.pool.cur_idx, self.pool.plan_of, b.actions_done,
                b.at_goal, self.mode, fb["plan"], fb["t"], fb["k"], self.n_live]

    def rollout(self, K, out, ring=None, graph=True):
        """K steps of every env into the TransitionChunk ``out`` (one graph replay per step when ``graph``)."""
        env, b = self.env, self.nav
        if env._needs_reset:
            env.reset()
        if (out.K, out.N, out.obs_dim) != (K, env.n, env.obs_dim):
            raise ValueError("out chunk has the wrong shape")
        out.step0, out.env_id0 = env.t, env.env_id0
        b.begin_chunk(env)
        self.d_eps.fill_(float(max(self.agent.decaying_ou_action_noise.epsilon, 0.0)))
        self.d_eta.fill_(self.eta)
        if not graph:
            for _ in range(K):
                self.fused_step(out, ring)
            env.t += K
            return out
        self._graphs.replay(K, env.device, lambda: self.graph_key(K, out, ring), lambda: self.fused_step(out, ring),
                            self._state_tensors(), ring)
        env.t += K
        return out


# A kernel class of the per-step actor launch goes through ONE ssc_actor_forward_many when it has at least this many pairs;
# smaller groups act through ssc_actor_forward[_rms] on their slices (the same bits).  Measured on an MI355X
# (profiles/smartstart_population/actor.json; P = 1, 2, 4, 16, 64 actors x 16 and x 1024 rows; a case is won when the slowest
# many-call window beats the fastest per-pair window): 2 is the smallest group that wins at every measured shape of the
# fp32 64-32 class (x2.2 at P = 2), the bf16 64-32 class (x1.7-1.8), the bf16 200-100 class (x2.05) and the generic class at
# 1024 rows (x2.0); a lone bf16 64-32 actor LOSES 5-10 % in the many-call (4.8 against 4.3-4.6 us) and belongs in its own call.
SMARTSTART_POPULATION_ACTOR_MIN_GROUP = 2
# ... except for generic-class pairs of <= 32 envs each: their own call is actor_row_kernel (4.3 us for 16 rows, a block per
# row) where the many-call runs the one-row-per-lane generic body (34 us whatever the row count), so P = 2 and 4 lose
# (x0.24, x0.49) and 16 is the smallest measured group that wins (x1.9; 64: x7.7)
SMARTSTART_POPULATION_ACTOR_MIN_GROUP_FEW_ROWS = 16


# A population of at least this many pairs selects its smart starts through ``select_plans_many``
# (``VecSmartStartPopulation.refresh_plans``); a smaller one runs the per-pair calls.  Measured on an MI355X
# (tools/exp_smartstart_population_selection.py, profiles/smartstart_population/selection.json; P = 1, 2, 16, 64 pairs, rings
# of 4 096, 65 536 and 500 000 states, 64-32 and 200-100 agents, n_ss 1000, n_plans 1 and 8; a case is won when the slowest
# grouped window beats the fastest per-pair window, host geometry left out of both): every case with P >= 2 is won (x1.29 ..
# x3.6 at 2 pairs, x3.3 .. x11.8 at 64); P = 1 LOSES on the 500 000-state rings with n_plans = 1 (x0.77 and x0.91: the
# one-workgroup covariance scan costs more there than the host waits it saves), wins nine of the other ten by x1.09 .. x2.8 and misses the tenth by one slow window.
SMARTSTART_POPULATION_SELECTION_MIN_GROUP = 2


class _SelectManyBuffers:
    """Device and pinned buffers of ``select_plans_many`` for one list of pairs: pooled per-slot arrays (row0 of pair p =
    the slots of the pairs before it) and ONE byte block [chosen | len | status | n_cand | paths] that goes to the host in
    one copy.  Rebuilt when a shape changes."""

    def __init__(self, shapes, obs_dim, act_dim, device):
        from .population import DeviceItems
        self.shapes, self.obs_dim, self.act_dim, self.device = shapes, obs_dim, act_dim, device
        P = len(shapes)
        self.row0 = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int64)
        self.plan0 = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.int64)
        path_elems = [s[1] * (s[2] + 1) * obs_dim for s in shapes]
        self.path0 = np.concatenate([[0], np.cumsum(path_elems)]).astype(np.int64)
        m, k = int(self.row0[-1]), int(self.plan0[-1])
        self.m = m
        lib = _ffi.lib()
        ws = [int(lib.ssc_replay_smart_start_workspace_bytes(int(s[0]))) for s in shapes]
        self.ws0 = np.concatenate([[0], np.cumsum(ws)]).astype(np.int64)
        f = lambda n, dt: torch.zeros(max(int(n), 1), dtype=dt, device=device)
        self.idx, self.cand, self.act = f(m, torch.int32), f(m * obs_dim, torch.float32), f(m * act_dim, torch.float32)
        self.value, self.pdf, self.ucb = f(m, torch.float32), f(m, torch.float32), f(m, torch.float32)
        self.wh, self.norm = f(P * obs_dim * obs_dim, torch.float32), f(P, torch.float64)
        self.workspace = f(self.ws0[-1], torch.uint8)
        # the block the host reads: int32 chosen [k] | len [k] | status [P] | n_cand [P] | float paths
        self.o_len, self.o_status, self.o_ncand, self.o_path = 4 * k, 8 * k, 8 * k + 4 * P, 8 * k + 8 * P
        nbytes = self.o_path + 4 * int(self.path0[-1])
        self.block = f(nbytes, torch.uint8)
        self.host = torch.zeros(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        self.items = DeviceItems(_ffi.SelectManyItem, P, device)
        self.sent = None
        self.actor_items, self.actor_sent = {}, {}
        with torch.cuda.device(device):
            self.done = torch.cuda.Event()


def select_plans_many(pairs, replays):
    """``SmartStartSelection.select_plans`` for all ``pairs`` (each on its own ring of ``replays``) in one launch per stage:
    candidates + gather (``ssc_replay_smart_start_indices_many``), Scott bandwidth on the device
    (``ssc_kde_scott_bandwidth_many``), the plain actors (``ssc_actor_forward_many`` per kernel class, by the population's
    grouping rule), critics, KDE (the rings read in place), UCB1 top-k and the chosen paths -- then ONE device-to-host copy of
    status, chosen indices, path lengths and paths into pinned memory and ONE wait, and ``plan_from_path`` per chosen path on
    the host.  Returns per pair a plan list, or None where ``select_plans`` returns None (empty ring, ``n_ss <= 0``, no valid
    candidate).  ``replay._queries`` and ``pair.last_chosen`` move as the per-pair calls move them.  A pair whose bandwidth
    has no Cholesky factor raises ``numpy.linalg.LinAlgError`` naming the pair, after the read.  The bandwidth is the only
    stage whose bits differ from ``kde_scott_bandwidth`` (its own fixed summation order); every other stage returns the
    per-pair call's bits on the same input."""
    pairs, replays = list(pairs), list(replays)
    P = len(pairs)
    if P == 0 or len(replays) != P:
        raise ValueError("select_plans_many: one replay ring per pair, at least one pair")
    for r in replays:
        if not isinstance(r, DeviceReplayBuffer) or not r.track_episodes:
            raise TypeError("select_plans_many needs DeviceReplayBuffer(track_episodes=True) rings")
    dev = replays[0].device
    od, ad = replays[0].obs_dim, pairs[0].agent.act_dim
    if any(r.obs_dim != od or pr.agent.act_dim != ad for r, pr in zip(replays, pairs)):
        raise ValueError("select_plans_many: the pairs of one call share obs_dim and act_dim")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("select_plans_many reads its results on the host; it cannot run inside a graph capture")
    for pr in pairs:
        if int(pr.n_ss) > 4096:
            raise ValueError("n_ss <= 4096 on the device path")
        if not 1 <= int(pr.n_plans) <= 64:
            raise ValueError("select_plans_many: n_plans in 1..64")
    shapes = tuple((max(int(pr.n_ss), 0), int(pr.n_plans), int(r.max_path_len)) for pr, r in zip(pairs, replays))
    owner = pairs[0]
    buf = getattr(owner, "_select_many", None)
    if buf is None or buf.shapes != shapes or (buf.obs_dim, buf.act_dim, buf.device) != (od, ad, dev) or \
            getattr(owner, "_select_many_pairs", None) != [id(pr) for pr in pairs]:
        buf = owner._select_many = _SelectManyBuffers(shapes, od, ad, dev)
        owner._select_many_pairs = [id(pr) for pr in pairs]
    lib = _ffi.lib()
    live = [len(r) > 0 and s[0] > 0 for r, s in zip(replays, shapes)]
    fresh = (_ffi.SelectManyItem * P)()
    base = buf.block.data_ptr()
    for p, (it, pr, r) in enumerate(zip(fresh, pairs, replays)):
        n_ss, n_plans, max_len = shapes[p]
        size = len(r)
        it.ring, it.count, it.n = r.ring_struct(), (r.count if live[p] else 0), r.n_envs
        it.n_ss, it.n_plans, it.max_len = (n_ss if live[p] else 0), n_plans, max_len
        if not live[p]:
            continue
        it.seed, it.counter = r.seed ^ 0x5353, r._queries
        rows = size + 1
        stride = 1
        if pr.kde_max_states is not None and rows > pr.kde_max_states:
            stride = -(-rows // int(pr.kde_max_states))
        n_data = -(-rows // stride)
        it.stride, it.n_data = stride, n_data
        it.scott = (n_data ** (-1.0 / (od + 4))) ** 2
        a = pr.agent
        rms = getattr(a, "obs_rms", None)
        it.actor, it.critic = a._desc, a._critic_desc
        it.d_rms = None if rms is None else rms.block.data_ptr()
        it.alpha, it.beta = float(pr.exploitation_param), float(pr.exploration_param)
        it.volume = float(volume_of_n_dimensional_hyperellipsoid(pr.last_radii)) if pr.last_radii is not None else 1.0
        r0, k0 = int(buf.row0[p]), int(buf.plan0[p])
        it.row0 = r0
        it.d_idx, it.d_cand = buf.idx.data_ptr() + 4 * r0, buf.cand.data_ptr() + 4 * r0 * od
        it.d_value, it.d_pdf, it.d_ucb = (t.data_ptr() + 4 * r0 for t in (buf.value, buf.pdf, buf.ucb))
        it.d_wh, it.d_norm = buf.wh.data_ptr() + 4 * p * od * od, buf.norm.data_ptr() + 8 * p
        it.d_chosen, it.d_len = base + 4 * k0, base + buf.o_len + 4 * k0
        it.d_status, it.d_n_cand = base + buf.o_status + 4 * p, base + buf.o_ncand + 4 * p
        it.d_path = base + buf.o_path + 4 * int(buf.path0[p])
        it.d_workspace, it.workspace_bytes = buf.workspace.data_ptr() + int(buf.ws0[p]), int(buf.ws0[p + 1] - buf.ws0[p])
    if not any(live):
        return [None] * P
    image = bytes(fresh)
    di = buf.items
    with torch.cuda.device(dev):
        st = _ffi.stream(dev)
        if buf.sent != image:
            di.wait()
            ctypes.memmove(di.h_ptr, ctypes.addressof(fresh), len(image))
            di.upload()
            buf.sent = image
        _ffi.check(lib.ssc_replay_smart_start_indices_many(di.h_ptr, di.d_ptr, P, st))
        _ffi.check(lib.ssc_kde_scott_bandwidth_many(di.h_ptr, di.d_ptr, P, st))
        _select_many_actors(buf, pairs, live, st)
        _ffi.check(lib.ssc_critic_forward_many(di.h_ptr, di.d_ptr, P, buf.m, _ffi.ptr(buf.act), st))
        _ffi.check(lib.ssc_kde_evaluate_many(di.h_ptr, di.d_ptr, P, st))
        _ffi.check(lib.ssc_ucb_topk_many(di.h_ptr, di.d_ptr, P, st))
        _ffi.check(lib.ssc_replay_episode_path_many(di.h_ptr, di.d_ptr, P, st))
        chosen64 = buf.block[:buf.o_len].view(torch.int32).long()      # every pair's last_chosen is a slice of this
        buf.host.copy_(buf.block, non_blocking=True)
        buf.done.record()
    for p, r in enumerate(replays):
        if live[p]:
            r._queries += 1
    buf.done.synchronize()                                             # the ONE host wait of the refresh
    h = buf.host.numpy()
    K = int(buf.plan0[-1])
    h_chosen, h_len = h[:4 * K].view(np.int32), h[buf.o_len:buf.o_len + 4 * K].view(np.int32)
    h_status, h_ncand = h[buf.o_status:buf.o_status + 4 * P].view(np.int32), h[buf.o_ncand:buf.o_ncand + 4 * P].view(np.int32)
    h_path = h[buf.o_path:].view(np.float32)
    out = []
    for p, pr in enumerate(pairs):
        if not live[p] or h_ncand[p] == 0:
            out.append(None)
            continue
        if h_status[p] != 0:
            raise np.linalg.LinAlgError("select_plans_many: pair %d: the KDE covariance has no Cholesky factor" % p)
        n_ss, n_plans, max_len = shapes[p]
        k0 = int(buf.plan0[p])
        n_chosen = int((h_chosen[k0:k0 + n_plans] >= 0).sum())
        pr.last_chosen = chosen64[k0:k0 + n_chosen]
        paths = h_path[int(buf.path0[p]):int(buf.path0[p + 1])].reshape(n_plans, max_len + 1, od)
        plans = []
        for j in range(n_chosen):
            rows = int(h_len[k0 + j])
            if rows == 0:
                raise ValueError(": (   -   the episode start of this record is no longer in the ring")
            if rows < 2:
                continue
            plans.append(pr.plan_from_path(paths[j, :rows].astype(np.float64)))
        out.append(plans)
    return out


def _select_many_actors(buf, pairs, live, st):
    """The plain actors on the pooled candidate matrix: one ``ssc_actor_forward_many`` per kernel class with enough pairs
    (the population's grouping rule), the rest alone on their slices -- the same bits either way."""
    from .population import DeviceItems
    lib, groups = _ffi.lib(), {}
    od, ad = buf.obs_dim, buf.act_dim
    for p, pr in enumerate(pairs):
        if not live[p]:
            continue
        rms = getattr(pr.agent, "obs_rms", None)
        groups.setdefault(lib.ssc_actor_many_class(ctypes.byref(pr.agent._desc), int(rms is not None)), []).append(p)
    for key in [k for k in buf.actor_items if k not in groups]:
        del buf.actor_items[key]
        buf.actor_sent.pop(key, None)
    for cls, members in sorted(groups.items()):
        few_rows = cls // 2 == 8 and all(buf.shapes[p][0] <= 32 for p in members)
        need = SMARTSTART_POPULATION_ACTOR_MIN_GROUP_FEW_ROWS if few_rows else SMARTSTART_POPULATION_ACTOR_MIN_GROUP
        if cls < 0 or len(members) < need:
            for p in members:
                a = pairs[p].agent
                rms = getattr(a, "obs_rms", None)
                r0, rows = int(buf.row0[p]), buf.shapes[p][0]
                obs, out = buf.cand.data_ptr() + 4 * r0 * od, buf.act.data_ptr() + 4 * r0 * ad
                if rms is None:
                    _ffi.check(lib.ssc_actor_forward(ctypes.byref(a._desc), rows, obs, out, st))
                else:
                    _ffi.check(lib.ssc_actor_forward_rms(ctypes.byref(a._desc), rows, obs, out, st, _ffi.ptr(rms.block)))
            continue
        fresh = (_ffi.ActorManyItem * len(members))()
        for it, p in zip(fresh, members):
            rms = getattr(pairs[p].agent, "obs_rms", None)
            it.actor, it.d_rms = pairs[p].agent._desc, (None if rms is None else rms.block.data_ptr())
            it.row0, it.rows = int(buf.row0[p]), buf.shapes[p][0]
        di = buf.actor_items.get(cls)
        if di is None or di.n != len(members):
            di = buf.actor_items[cls] = DeviceItems(_ffi.ActorManyItem, len(members), buf.device)
            buf.actor_sent.pop(cls, None)
        image = bytes(fresh)
        if buf.actor_sent.get(cls) != image:
            di.wait()
            ctypes.memmove(di.h_ptr, ctypes.addressof(fresh), len(image))
            di.upload()
            buf.actor_sent[cls] = image
        _ffi.check(lib.ssc_actor_forward_many(di.h_ptr, di.d_ptr, di.n, buf.m, _ffi.ptr(buf.cand), _ffi.ptr(buf.act), st))


def _per_pair(value, n, what):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != n:
            raise ValueError("%s: one value or one per pair (%d), got %d" % (what, n, len(value)))
        return list(value)
    return [value] * n


class PopulationPair(SmartStartSelection):
    """One pair of a :class:`VecSmartStartPopulation`: its agent, dynamics model, envs [env0, env0 + n) of the population's
    VecEnv and its window of the population's plan pool.  Everything it does is :class:`SmartStartSelection`'s.  (Its row of
    the device table is an ``_ffi.SmartStartPair``, the mirror of ``ssc_smartstart_pair``.)"""

    def __init__(self, population, index, agent, model, env0, n, pool, eta, eta_decay_factor, n_ss, n_plans, exploitation_param,
                 exploration_param, path_shortcutting, steps_per_waypoint, mean_per_stepsize, std_per_stepsize,
                 stepsizes_in_waypoint_radii, kde_max_states):
        self.population, self.index = population, index
        self.env, self.nav = population.env, population.nav
        self.agent, self.model, self.env0, self.n, self.pool = agent, model, int(env0), int(n), pool
        self.eta, self.eta_decay_factor = float(eta), float(eta_decay_factor)
        self.n_ss, self.n_plans = int(n_ss), int(n_plans)
        self.exploitation_param, self.exploration_param = exploitation_param, exploration_param
        self.path_shortcutting, self.steps_per_waypoint = path_shortcutting, steps_per_waypoint
        self.mean_per_stepsize, self.std_per_stepsize = mean_per_stepsize, std_per_stepsize
        self.stepsizes_in_waypoint_radii = stepsizes_in_waypoint_radii
        self.kde_max_states = kde_max_states
        self.last_radii = None
        self.selections = 0


class VecSmartStartPopulation:
    """P SmartStart pairs -- the seeds and hyper-parameters of a sweep
    (examples/continuous/SmartStart_DDPG_Baselines_experimenter.py) -- stepping from ONE captured graph.  ONE
    :class:`VecEnv` holds the envs of all pairs, pair p owning the next ``envs_per_pair[p]`` of them; one set of plan arrays
    holds every pair's slots (``navigator.PlanPool.window``); every RNG stream is keyed by the global env id.  Env e of pair
    p gets, bit for bit, what a :class:`VecSmartStart` of its own on ``VecEnv(n_p, env_id0 = env.env_id0 + env0_p)`` with the
    same seed gives it.  One step = four launches: the actors (``ssc_actor_forward_many`` per kernel class of at least
    ``SMARTSTART_POPULATION_ACTOR_MIN_GROUP`` pairs, else the pair's own call on its slice), the forward simulation of all
    dynamics models (``navigator.NavigatorPopulation``), the scorer, and ``ssc_smartstart_rollout_step_many``.  The mask
    ``mode`` lets simulation and scoring skip what is not navigating; there is NO compact live list (the many-simulation
    refuses it).  ``eta``, ``eta_decay_factor``, ``n_ss``, ``n_plans`` and the exploitation / exploration parameters take one
    value or one per pair; the navigator settings are shared.  Selection, plan geometry and dynamics-model aggregation of
    pair p: ``pairs[p]`` (:class:`SmartStartSelection`)."""

    def __init__(self, env, agents, dyn_models, envs_per_pair, eta=0.5, eta_decay_factor=1.0, n_ss=1000, exploitation_param=1.,
                 exploration_param=2., n_plans=1, n_slots=None, w_max=None, num_control_samples=64, horizon=4,
                 noise_amount=0.005, steps_before_giving_up_on_waypoint=5, final_steps=10, theta=1.0, gamma=0.75,
                 horizontal_penalty_factor=0.5, path_shortcutting=True, mean_per_stepsize=1, std_per_stepsize=1,
                 stepsizes_in_waypoint_radii=1, steps_per_waypoint=1, chunk_steps=64, seed=1234, log_modes=False,
                 kde_max_states=500000):
        from . import navigator as nav
        from .population import DeviceItems
        agents, dyn_models = list(agents), list(dyn_models)
        P = len(agents)
        if P == 0 or len(dyn_models) != P:
            raise ValueError("VecSmartStartPopulation: one dynamics model per agent, at least one pair")
        for a in agents:
            if getattr(a, "ret_rms", None) is not None:
                raise NotImplementedError("VecSmartStartPopulation: a base agent with normalize_returns / Pop-Art is not "
                                          "supported (the selection reads the raw critic)")
        counts = [int(c) for c in _per_pair(envs_per_pair, P, "envs_per_pair")]
        if min(counts) < 1 or sum(counts) != env.n:
            raise ValueError("VecSmartStartPopulation: envs_per_pair %s for %d envs" % (counts, env.n))
        self.env, self.agents, self.models, self.envs_per_pair = env, agents, dyn_models, counts
        dev = env.device
        max_steps = env.spec.max_episode_steps or 1000
        w_max = int(w_max) if w_max is not None else max_steps + 1
        plans = [int(x) for x in _per_pair(n_plans, P, "n_plans")]
        if n_slots is None:        # a published plan must outlive every episode that started on it (VecSmartStart's rule)
            slots = [k * (-(-max_steps // max(int(chunk_steps), 1)) + 2) for k in plans]
        else:
            slots = [int(x) for x in _per_pair(n_slots, P, "n_slots")]
        self.pool = nav.PlanPool(env.n, sum(slots), w_max, env.obs_dim, dev, theta=theta, gamma=gamma,
                                 horizontal_penalty_factor=horizontal_penalty_factor)
        self.nav = nav.NavigatorPopulation(dyn_models, self.pool, counts, num_control_samples=num_control_samples,
                                           horizon=horizon, action_low=env.action_space.low, action_high=env.action_space.high,
                                           noise_amount=noise_amount,
                                           steps_before_giving_up_on_waypoint=steps_before_giving_up_on_waypoint,
                                           final_steps=final_steps, seed=seed, problem_id0=env.env_id0)
        self.nav.start_idx.zero_()
        self.mode = torch.zeros(env.n, dtype=torch.uint8, device=dev)
        self.pool.active = self.mode     # simulation skips dead waves, the one-launch scorer dead problems; no live list
        self.actor_out = torch.zeros((env.n, 1), dtype=torch.float32, device=dev)
        self.stats = torch.zeros((P, 4), dtype=torch.float64, device=dev)
        per = lambda v, what: _per_pair(v, P, what)
        etas, decays, nss = per(eta, "eta"), per(eta_decay_factor, "eta_decay_factor"), per(n_ss, "n_ss")
        xi, xr = per(exploitation_param, "exploitation_param"), per(exploration_param, "exploration_param")
        self.pairs, env0, slot0 = [], 0, 0
        for p in range(P):
            self.pool.plan_of[env0:env0 + counts[p]] = slot0
            self.pairs.append(PopulationPair(
                self, p, agents[p], dyn_models[p], env0, counts[p], self.pool.window(env0, counts[p], slot0, slots[p]),
                eta=float(etas[p]), eta_decay_factor=float(decays[p]), n_ss=int(nss[p]), n_plans=plans[p],
                exploitation_param=xi[p], exploration_param=xr[p], path_shortcutting=path_shortcutting,
                steps_per_waypoint=steps_per_waypoint, mean_per_stepsize=mean_per_stepsize, std_per_stepsize=std_per_stepsize,
                stepsizes_in_waypoint_radii=stepsizes_in_waypoint_radii, kde_max_states=kde_max_states))
            env0, slot0 = env0 + counts[p], slot0 + slots[p]
        self.log_modes = bool(log_modes)
        self.mode_log = None
        self.pair_table = DeviceItems(_ffi.SmartStartPair, P, dev)
        self._actor_items, self._actor_sent, self._actor_plan = {}, {}, []
        self._graphs = StepGraphs(keep=4)

    # ------------------------------------------------------------------------------ tables --
    def sync_pair_table(self):
        """The device table ``ssc_smartstart_rollout_step_many`` reads at every launch: each pair's env range, plan window
        and triple, eta, the agent's current OU epsilon and OU process.  Rewritten and uploaded in front of a chunk, outside
        the capture: a replayed graph follows the host's decay schedules and pool refreshes through it."""
        t = self.pair_table
        t.wait()
        for it, pr in zip(t.items, self.pairs):
            a = pr.agent
            it.env0, it.n_envs, it.slot0 = pr.env0, pr.n, pr.pool.slot0
            it.pool_first, it.pool_count, it.pool_slots = pr.pool.triple
            it.eta, it.ou_epsilon = pr.eta, float(max(a.decaying_ou_action_noise.epsilon, 0.0))
            it.ou.mu, it.ou.sigma, it.ou.theta = float(a.ou["mu"]), float(a.ou["sigma"]), float(a.ou["theta"])
            it.ou.dt = float(a.decaying_ou_action_noise.dt)
        t.upload()
        return t

    def sync_actor_items(self):
        """How the step's actor launch serves every pair -> [("many", class, DeviceItems) | ("alone", pair index)]: one
        item table per kernel class with at least ``SMARTSTART_POPULATION_ACTOR_MIN_GROUP`` pairs (generic-class pairs of <= 32
        envs each: ``SMARTSTART_POPULATION_ACTOR_MIN_GROUP_FEW_ROWS``), re-uploaded only when its
        bytes change and never inside a capture."""
        from .population import DeviceItems
        lib, groups = _ffi.lib(), {}
        for p, pr in enumerate(self.pairs):
            rms = getattr(pr.agent, "obs_rms", None)
            c = lib.ssc_actor_many_class(ctypes.byref(pr.acting_desc()), int(rms is not None))
            groups.setdefault((c, pr.acting_desc().obs_dim, pr.acting_desc().act_dim), []).append(p)
        plan = []
        for key, members in sorted(groups.items()):
            few_rows = key[0] // 2 == 8 and all(self.pairs[p].n <= 32 for p in members)      # generic class, row-kernel sized pairs
            need = SMARTSTART_POPULATION_ACTOR_MIN_GROUP_FEW_ROWS if few_rows else SMARTSTART_POPULATION_ACTOR_MIN_GROUP
            if key[0] < 0 or len(members) < need:
                plan += [("alone", p) for p in members]
                continue
            fresh = (_ffi.ActorManyItem * len(members))()
            for it, p in zip(fresh, members):
                pr = self.pairs[p]
                rms = getattr(pr.agent, "obs_rms", None)
                it.actor, it.d_rms = pr.acting_desc(), (None if rms is None else rms.block.data_ptr())
                it.row0, it.rows = pr.env0, pr.n
            di = self._actor_items.get(key)
            if di is None or di.n != len(members):
                di = self._actor_items[key] = DeviceItems(_ffi.ActorManyItem, len(members), self.env.device)
                self._actor_sent.pop(key, None)
            image = bytes(fresh)
            if self._actor_sent.get(key) != image:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("VecSmartStartPopulation: an actor item table changed inside a graph capture; "
                                       "call sync_actor_items() in front of it")
                di.wait()
                ctypes.memmove(di.h_ptr, ctypes.addressof(fresh), len(image))
                di.upload()
                self._actor_sent[key] = image
            plan.append(("many", key, di))
        for key in [k for k in self._actor_items if k not in groups]:
            del self._actor_items[key]
            self._actor_sent.pop(key, None)
        self._actor_plan = plan
        return plan

    # -------------------------------------------------------------------------- selection --
    def refresh_plans(self, replays):
        """``refresh_plans`` of every pair on its ring of ``replays``: ONE grouped selection (``select_plans_many``: one
        launch per stage, one host wait for the whole population), then ``publish_plans`` pair by pair.  A population of
        fewer than ``SMARTSTART_POPULATION_SELECTION_MIN_GROUP`` pairs runs the per-pair calls.  Returns every pair's
        ``last_chosen`` (None where its ring holds no complete episode start yet)."""
        replays = list(replays)
        if len(replays) != len(self.pairs):
            raise ValueError("VecSmartStartPopulation.refresh_plans: one replay ring per pair")
        if len(self.pairs) < SMARTSTART_POPULATION_SELECTION_MIN_GROUP:
            return [pr.refresh_plans(r) for pr, r in zip(self.pairs, replays)]
        for pr in self.pairs:
            pr.last_chosen = None
        for pr, plans in zip(self.pairs, select_plans_many(self.pairs, replays)):
            if plans is not None:
                pr.publish_plans(plans)
        return [pr.last_chosen for pr in self.pairs]

    # ------------------------------------------------------------------------------ steps --
    def _step_struct(self, chunk_k):
        e = self.env
        ss = _ffi.SmartStartStep()
        ss.mode, ss.plan_of, ss.d_actor_out = self.mode.data_ptr(), self.pool.plan_of.data_ptr(), self.actor_out.data_ptr()
        ss.act_low, ss.act_high = float(e.action_space.low[0]), float(e.action_space.high[0])
        if self.log_modes:
            if self.mode_log is None or self.mode_log.shape != (chunk_k, e.n):
                self.mode_log = torch.zeros((chunk_k, e.n), dtype=torch.uint8, device=e.device)
            ss.d_mode_log, ss.mode_log_stride = self.mode_log.data_ptr(), e.n
        return ss

    def graph_key(self, K, chunk, ring):
        """What ``VecSmartStart.graph_key`` covers, per pair, plus the item and pair tables' addresses: the navigator's key,
        every pair's acting descriptor by value and statistics block, the split, the shared tensors, and how the actor
        launch is grouped (class, members, table addresses).  eta, epsilon, the OU process and the pool triples are NOT
        here: they reach a replay through the pair table."""
        ptr = lambda t: None if t is None else t.data_ptr()
        e, p = self.env, self.pool
        pairs = tuple((bytes(pr.acting_desc()), ptr(getattr(getattr(pr.agent, "obs_rms", None), "block", None)), pr.env0, pr.n,
                       pr.pool.slot0, pr.pool.n_slots) for pr in self.pairs)
        actors = tuple((w[0], w[1]) if w[0] == "alone" else (w[0], w[1], w[2].h_ptr, w[2].d_ptr, w[2].n) for w in self._actor_plan)
        return (K, self.nav.graph_key(e, chunk, ring), pairs, actors, (self.pair_table.h_ptr, self.pair_table.d_ptr),
                tuple(ptr(x) for x in (self.mode, p.plan_of, p.wp_len, p.active, self.actor_out, self.stats, self.mode_log)),
                self.log_modes, float(e.action_space.low[0]), float(e.action_space.high[0]))

    def fused_step(self, chunk, ring):
        """Enqueue ONE step for every env of every pair (four launches when every actor class is grouped)."""
        from . import navigator as nav
        env, b, lib = self.env, self.nav, _ffi.lib()
        fb = b._fused_buffers(env.device)
        d = env.obs_dim
        with torch.cuda.device(env.device):
            for way in self._actor_plan:
                if way[0] == "many":
                    di = way[2]
                    _ffi.check(lib.ssc_actor_forward_many(di.h_ptr, di.d_ptr, di.n, env.n, _ffi.ptr(fb["plan"]),
                                                          _ffi.ptr(self.actor_out), _ffi.stream()))
                    continue
                pr = self.pairs[way[1]]
                rms, desc = getattr(pr.agent, "obs_rms", None), pr.acting_desc()
                obs, out = fb["plan"].data_ptr() + 4 * d * pr.env0, self.actor_out.data_ptr() + 4 * pr.env0
                if rms is None:
                    _ffi.check(lib.ssc_actor_forward(ctypes.byref(desc), pr.n, obs, out, _ffi.stream()))
                else:
                    _ffi.check(lib.ssc_actor_forward_rms(ctypes.byref(desc), pr.n, obs, out, _ffi.stream(), _ffi.ptr(rms.block)))
        sp = nav.mpc_sampling(b.N, b.low, b.high, b.seed, b.problem_id0, 0, t_base=fb["t"], active=self.mode)
        S = b._simulate(fb["plan"], sp, A_out=fb["A"])
        ss = self._step_struct(chunk.K if chunk is not None else 1)
        t = self.pair_table
        b._score_and_step(env, chunk, ring, S, lib.ssc_smartstart_rollout_step_many, ctypes.byref(ss), t.h_ptr, t.d_ptr, t.n,
                          stats=self.stats)

    def _state_tensors(self):
        e, b = self.env, self.nav
        fb = b._fused_buffers(e.device)
        return [e.s0, e.s1, e.steps, e.ep_ret, e.ou_x, self.stats, self.pool.cur_idx, self.pool.plan_of, b.actions_done,
                b.at_goal, self.mode, fb["plan"], fb["t"], fb["k"]]

    def rollout(self, K, out, ring=None, graph=True):
        """K steps of every env of every pair into the TransitionChunk ``out`` (one graph replay per step when ``graph``).
        The pair table (eta, epsilon, OU process, pool triple of every pair) and the actor item tables are refreshed here,
        outside the capture."""
        env, b = self.env, self.nav
        if env._needs_reset:
            env.reset()
        if (out.K, out.N, out.obs_dim) != (K, env.n, env.obs_dim):
            raise ValueError("out chunk has the wrong shape")
        out.step0, out.env_id0 = env.t, env.env_id0
        b.begin_chunk(env)
        self.sync_pair_table()
        self.sync_actor_items()
        if not graph:
            for _ in range(K):
                self.fused_step(out, ring)
            env.t += K
            return out
        self._graphs.replay(K, env.device, lambda: self.graph_key(K, out, ring), lambda: self.fused_step(out, ring),
                            self._state_tensors(), ring)
        env.t += K
        return out
