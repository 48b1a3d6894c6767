"""The training-loop driver: ``rlTrain`` with the reference's signature and control flow
(smartstart/reinforcementLearningCore/rlTrain.py:13-133) for any ``gym.Env``-shaped env and any
``RLAgent``, plus ``rl_train_vec`` -- the same loop over N device envs in fused chunks.
``Episode`` / ``Summary`` keep the per-episode quantities of smartstart/utilities/datacontainers.py
(:41-49, :61-80, :173-193) and read/write the reference's Summary JSON files (:257-374)."""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np


class Episode:
    """datacontainers.py:16-80"""

    def __init__(self):
        self.obs, self.action, self.reward, self.obs_tp1, self.done = [], [], [], [], []

    def append(self, obs, action, reward, obs_tp1, done):
        self.obs.append(np.ravel(obs).tolist())
        self.action.append(np.ravel(action).tolist())
        self.reward.append(float(reward))
        self.obs_tp1.append(np.ravel(obs_tp1).tolist())
        self.done.append(bool(done))

    def total_reward(self):
        return sum(self.reward)

    def average_reward(self):
        return sum(self.reward) / max(len(self.reward), 1)

    def path(self):
        return self.obs + [self.obs_tp1[-1]] if self.obs else []

    def __len__(self):
        return len(self.reward)


class Summary:
    """smartstart/utilities/datacontainers.py:130-374: per-episode (steps, total_reward), best path, the
    last ``last_x`` paths, SmartStart episode indices and the agent's hyper-parameters -- with the
    reference's attribute names, so that ``to_json`` / ``save`` / ``load`` read and write the same JSON
    files as the reference (``data/**/*.json``); the GCS upload is out of scope."""

    def __init__(self, name=None, last_x=5):
        self.name = name
        self._pending = []      # (lengths, returns) numpy chunks from the fused rollouts, not yet turned into tuples
        self.episodes = []
        self.best_path = None
        self.best_reward = -sys.maxsize                      # :163
        self.last_x = max(last_x, 1)
        self.last_paths = [[None]] * last_x                  # :167 (oldest first)
        self.last_rewards = [None] * last_x
        self.smart_start_episodes = []
        self.name_of_agent = ""
        self.param_dict = {}

    def set_agent(self, agent):
        """:173-176"""
        self.name_of_agent = str(agent.__class__.__name__)
        try:
            pd = agent.get_param_dict()
        except NotImplementedError:
            pd = None
        if pd is not None:
            self.param_dict = {**pd, **self.param_dict}

    def add_params_to_param_dict(self, **kwargs):
        self.param_dict = {**kwargs, **self.param_dict}

    def start_smart_start_episode(self):
        self.smart_start_episodes.append(len(self.episodes))

    def append(self, episode):
        """:180-203"""
        total = episode.total_reward()
        self.episodes.append((len(episode), total))
        if total > self.best_reward:
            self.best_path, self.best_reward = episode.path(), total
        self.last_paths = self.last_paths[1:] + [episode.path()]
        self.last_rewards = self.last_rewards[1:] + [total]

    def append_record(self, length, total_reward):
        """A finished episode reported by the fused rollout kernel's episode ring (no path)."""
        self.episodes.append((int(length), float(total_reward)))
        if total_reward > self.best_reward:
            self.best_reward = float(total_reward)

    def extend_records(self, lengths, total_rewards):
        """Many finished episodes at once (numpy arrays from the episode ring).  A 65 536-env chunk can finish
        65 536 of them; building that many Python tuples per chunk would dominate the loop, so the arrays are
        kept and turned into the reference's list of ``(steps, total_reward)`` tuples when ``episodes`` is read."""
        if len(lengths) == 0:
            return
        self._pending.append((np.asarray(lengths).copy(), np.asarray(total_rewards).copy()))
        best = float(total_rewards.max())
        if best > self.best_reward:
            self.best_reward = best

    @property
    def episodes(self):
        if self._pending:
            pend, self._pending = self._pending, []
            for lengths, rets in pend:
                self._episodes.extend(zip(lengths.tolist(), rets.tolist()))
        return self._episodes

    @episodes.setter
    def episodes(self, value):
        self._pending = []
        self._episodes = value

    # ---- accessors (:205-255) ---------------------------------------------------------------------
    def total_episode_reward(self):
        return [reward for _, reward in self.episodes]

    def total_reward(self):
        return sum(self.total_episode_reward())

    def average_reward(self):
        return self.total_reward() / len(self)

    def average_episode_reward(self):
        return [reward / steps for steps, reward in self.episodes]

    def steps_episode(self):
        return [steps for steps, _ in self.episodes]

    def get_best_path_and_reward(self):
        return self.best_path, self.best_reward

    def get_last_path(self, x):
        return self.last_paths[-(x + 1)]

    def get_last_reward(self, x):
        return self.last_rewards[-(x + 1)]

    def __len__(self):
        return len(self._episodes) + sum(len(l) for l, _ in self._pending)

    # ---- persistence (:257-374) ---------------------------------------------------------------------
    def to_json(self):
        def plain(o):
            return o.tolist() if isinstance(o, np.ndarray) else float(o) if isinstance(o, np.floating) else \
                int(o) if isinstance(o, np.integer) else str(o)
        d = {k: v for k, v in self.__dict__.items() if k not in ("_episodes", "_pending")}
        d["episodes"] = self.episodes
        return json.dumps(d, default=plain)

    @classmethod
    def from_json(cls, data):
        summary = cls()
        fields = json.loads(data)
        summary.episodes = fields.pop("episodes", [])
        summary.__dict__.update(fields)
        return summary

    def save(self, directory=".", post_fix=0, extra_name_append="", last_name_section=False):
        """:288-326: <name><extra>_<post_fix>.json, post_fix auto-incremented past existing files."""
        def make_name(pf):
            name = self.name.split("_")[-1] if last_name_section else self.name
            return os.path.join(directory, name + extra_name_append + "_" + str(pf) + ".json")
        fp = make_name(post_fix)
        while os.path.exists(fp):
            post_fix += 1
            fp = make_name(post_fix)
        with open(fp, "x") as f:
            f.write(self.to_json())
        return fp

    @classmethod
    def load(cls, fp):
        with open(fp, "r") as f:
            return cls.from_json(f.read())


def rlTrain(agent, env, render=False, render_episode=False, print_results=True, print_steps=True,
            num_episodes=500, max_steps=1000, progress_bar=False, id=None, num_ticks=100, print_time=False):
    """rlTrain.py:13-133, minus the console plotting."""
    name = agent.get_summary_name() if hasattr(agent, 'get_summary_name') else agent.__class__.__name__
    spec_id = env.spec.id if getattr(env, "spec", None) is not None else type(env).__name__
    summary = Summary(name + "_" + spec_id)                      # :50-55
    summary.set_agent(agent)
    times = [time.time()]
    for i_episode in range(num_episodes):                        # :63
        episode = Episode()
        observation = env.reset()                                # :68
        agent.start_new_episode(observation)                     # :71
        if getattr(agent, "smart_start_pathing", False):
            summary.start_smart_start_episode()
        for step in range(max_steps):                            # :75
            if render:
                render = agent.render(env)
            action = agent.get_action(observation)               # :81
            new_observation, reward, done, _ = env.step(action)  # :84
            if print_steps:
                print("        Step: {}, State: {}, Action: {}, New_State: {}, Reward: {}".format(
                    step, observation, action, new_observation, reward))
            agent.observe(observation, action, reward, new_observation, done)   # :91
            episode.append(observation, action, reward, new_observation, done)  # :94
            if done:
                break
            observation = new_observation
        agent.end_episode()                                      # :101
        if print_results:
            print("Episode: %d, steps: %d, reward: %.2f" % (i_episode, len(episode), episode.average_reward()))
        summary.append(episode)                                  # :114
        if print_time:
            times.append(time.time())
            print("took: " + str(times[-1] - times[-2]))
    return summary


def rl_train_vec(env, policy, num_chunks, chunk_steps=1024, ring_capacity=1 << 20, on_chunk=None):
    """The rlTrain loop for N parallel device envs: ``num_chunks`` fused rollouts of ``chunk_steps``
    steps each (auto-reset on done); every finished episode lands in the Summary as (len, return).
    ``on_chunk(chunk, env)`` -- if given -- sees each TransitionChunk (e.g. to feed a replay buffer)."""
    from .vec_env import EpisodeRing, TransitionChunk
    summary = Summary("vec_" + env.spec.id)
    ring = EpisodeRing(ring_capacity, env.device)
    chunk = TransitionChunk(env.obs_dim, chunk_steps, env.n, env.device) if on_chunk is not None else None
    pd = env.policy_desc(policy)
    dropped = 0
    for _ in range(num_chunks):
        out = env.rollout(chunk_steps, out=chunk, ring=ring, log=on_chunk is not None, policy_desc=pd)
        if on_chunk is not None:
            on_chunk(out, env)
        (ids, lens, rets), d = ring.drain()
        dropped += d
        summary.extend_records(lens, rets)
    summary.dropped_episode_records = dropped
    return summary


class DecaySchedule:
    """The per-episode decays of the reference -- ``reduce_epsilon`` (DDPG_Baselines_agent.py:77-78, from end_episode
    :255-258) and ``reduce_eta`` (smartexplorationcontinuous.py:372-376) -- for a loop over n parallel envs, kept on the
    DEVICE: one decay per GENERATION = ``per_generation`` finished episodes (once per episode per env), computed by
    ``ssc_decay_schedule`` from the finished-episode counter the rollout kernel accumulates (``env.stats[3]``).  The
    arithmetic is the host's (fp64 ``value = max(value * factor, floor)``, one application per generation), so the
    values equal ``reduce_epsilon()`` called ``generations`` times -- but no chunk boundary needs the host any more.

    ``entries``: list of (start value, factor, floor, out) with ``out`` a 1-element fp32 device tensor (or None) that
    receives the current value -- e.g. ``agent.d_epsilon``, which ``agent.as_policy(device_epsilon=True)`` hands to the
    rollout kernel."""

    def __init__(self, device, per_generation, entries):
        import ctypes
        import torch
        from . import _ffi
        self._ffi, self._torch = _ffi, torch
        self.device = torch.device(device)
        self.per_generation = float(per_generation)
        self.n = len(entries)
        if not 1 <= self.n <= 4:
            raise ValueError("1..4 schedules")
        self._factor = (ctypes.c_double * self.n)(*[float(e[1]) for e in entries])
        self._floor = (ctypes.c_double * self.n)(*[float(e[2]) for e in entries])
        self.state = torch.tensor([0.0] + [float(e[0]) for e in entries], dtype=torch.float64, device=self.device)
        self.outs = [e[3] for e in entries]
        self._out_ptrs = (ctypes.c_void_p * self.n)(*[None if o is None else o.data_ptr() for o in self.outs])
        for e in entries:
            if e[3] is not None:
                e[3].fill_(float(e[0]))

    def update(self, finished, finished0=0.0):
        """Enqueue the decay on the current stream; ``finished``: device fp64 view of the finished-episode counter,
        ``finished0``: what it read when the loop started."""
        ffi, torch = self._ffi, self._torch
        with torch.cuda.device(self.device):
            ffi.check(ffi.lib().ssc_decay_schedule(ffi.ptr(finished), float(finished0), self.per_generation, self.n, self._factor, self._floor,
                                                   ffi.ptr(self.state), self._out_ptrs,
                                                   ffi.stream(self.device)))

    def read(self):
        """(generations applied, [current values]) -- a device -> host read (synchronises the current stream)."""
        st = self.state.cpu().tolist()
        return int(st[0]), st[1:]


class DecayScheduleGroup:
    """P :class:`DecaySchedule` objects updated by ONE launch (``ssc_decay_schedule_many``, one thread per schedule set):
    states and outputs end up exactly as after ``schedule.update`` one by one.  Nothing in the descriptors changes from
    chunk to chunk, so they are built on the first call (and again when a counter, ``finished0`` or the stream changes).
    Schedules that share a state array update one by one; ``fused`` tells which way the last call went."""

    def __init__(self, schedules):
        self.schedules = list(schedules)
        if not self.schedules:
            raise ValueError("a group needs at least one schedule")
        s0 = self.schedules[0]
        self._ffi, self._torch, self.device = s0._ffi, s0._torch, s0.device
        self.fused = None
        self._sig = self._items = None

    def update(self, finished, finished0=None):
        """``schedules[p].update(finished[p], finished0[p])`` for every p."""
        ffi, torch, ss = self._ffi, self._torch, self.schedules
        finished = list(finished)
        finished0 = [0.0] * len(ss) if finished0 is None else [float(x) for x in finished0]
        sig = (torch.cuda.current_stream(self.device).cuda_stream, tuple(f.data_ptr() for f in finished), tuple(finished0))
        if sig != self._sig:
            from .population import DeviceItems
            self._sig, self._items = sig, None
            self.fused = (len({s.state.data_ptr() for s in ss}) == len(ss) and all(s.device == self.device for s in ss))
            if self.fused:
                items = DeviceItems(ffi.DecayItem, len(ss), self.device)
                for it, s, f, f0 in zip(items.items, ss, finished, finished0):
                    it.d_finished, it.finished0, it.per_generation, it.n_sched = f.data_ptr(), f0, s.per_generation, s.n
                    for i in range(s.n):
                        it.factor[i], it.floor[i], it.d_out[i] = s._factor[i], s._floor[i], s._out_ptrs[i]
                    it.d_state = s.state.data_ptr()
                items.upload()
                self._items = items
        if not self.fused:
            for s, f, f0 in zip(ss, finished, finished0):
                s.update(f, f0)
            return
        with torch.cuda.device(self.device):
            ffi.check(ffi.lib().ssc_decay_schedule_many(self._items.h_ptr, self._items.d_ptr, len(ss), ffi.stream(self.device)))


def epsilon_schedule(agent, per_generation, device=None):
    """DecaySchedule of one agent's OU epsilon, starting from its current host value and writing ``agent.d_epsilon``."""
    n = agent.decaying_ou_action_noise
    return DecaySchedule(device if device is not None else agent.device, per_generation,
                         [(float(n.epsilon), n.epsilon_decay_factor, n.min_epsilon, agent.d_epsilon)])


def default_drain_every(ring_capacity, n_envs, chunk_steps, shortest_episode=64):
    """How many chunks an episode ring of ``ring_capacity`` records holds when no episode is shorter than
    ``shortest_episode`` steps (clamped to 1..16)."""
    per_chunk = n_envs * -(-int(chunk_steps) // shortest_episode)
    return int(max(1, min(16, ring_capacity // max(per_chunk, 1))))


def update_obs_rms(agent, chunk, last_steps=None):
    """store_transition's ``obs_rms.update(obs0)`` (ddpg_editted.py:281-285) for exactly the records
    ``DeviceReplayBuffer.append_chunk(chunk, last_steps=...)`` stored; nothing for an agent without
    normalize_observations.  Stream-ordered after the append, before the learner iterations of the chunk."""
    rms = getattr(agent, "obs_rms", None)
    if rms is None:
        return
    k = chunk.K if last_steps is None else min(int(last_steps), chunk.K)
    if k <= 0:                                    # append_chunk stored nothing
        return
    rms.update_chunk(chunk, chunk.K - k, chunk.K)


def vec_loop_buffers(env, chunk_steps, replay_capacity, ring_capacity, seed, track_episodes):
    """What a vectorised loop keeps in HBM -> (episode ring, transition chunk, device replay ring)."""
    from .replay_buffer import DeviceReplayBuffer
    from .vec_env import EpisodeRing, TransitionChunk
    replay = DeviceReplayBuffer(replay_capacity, env.obs_dim, 1, env.device, seed=seed, track_episodes=track_episodes,
                                n_envs=env.n, max_path_len=(env.spec.max_episode_steps or 1000) + 1)
    return EpisodeRing(ring_capacity, env.device), TransitionChunk(env.obs_dim, chunk_steps, env.n, env.device), replay


def adapt_and_perturb(agent, replay, dst=None, cycle=True):
    """The next chunk's acting copy ``dst`` (default ``agent.perturbed_actor_flat``): the stddev adapted on the obs0 of ONE
    fresh replay batch (ddpg_editted.py:360-376), then actor + noise of the adapted stddev -- in one launch
    (``agent.param_noise_cycle``) when ``cycle``, else ``adapt_param_noise`` + a perturbation.  Only the perturbation
    while the ring holds fewer than ``batch_size`` records.  Stream-ordered, no host read."""
    if len(replay) >= agent.batch_size:
        obs0 = replay.s.index_select(0, replay.sample_indices(1, agent.batch_size)[0].long())
        if cycle:
            agent.param_noise_cycle(obs0, dst=dst)
            return
        agent.adapt_param_noise(obs0)
    agent.perturbed_generation = agent._perturb(agent.perturbed_actor_flat if dst is None else dst)


def rl_train_vec_ddpg(env, agent, num_chunks, chunk_steps=256, replay_capacity=1 << 20, train_iters=None,
                      replay_last_steps=None, seed=0, ring_capacity=1 << 20, track_episodes=False, overlap=False,
                      drain_every=None, on_chunk=None, stats_every=None, eval_env=None, eval_every=None, eval_steps=None,
                      param_noise_cycle=False):
    """Actor-learner loop entirely in HBM: every chunk is a fused rollout of ``chunk_steps`` steps of all
    ``env.n`` envs under the agent's current actor (+ OU noise), appended to a device replay ring, followed
    by ``train_iters`` DDPG iterations (default ``agent.num_train_iterations``) on batches drawn from it.
    The vectorised counterpart of rlTrain + DDPG_Baselines_agent.observe/train
    (rlTrain.py:75-100, DDPG_Baselines_agent.py:238-273).  ``track_episodes`` keeps the episode index in the device
    ring as well, so that ``smartstart.device_smart_start_path(replay, agent, radii, n_ss)`` can pick a smart-start
    state and recover the path to it without the replay contents leaving HBM.

    Nothing at a chunk boundary needs the host: epsilon decays once per generation of finished episodes ON THE DEVICE
    (:class:`DecaySchedule` behind each rollout, the kernel reads ``agent.d_epsilon``), and the finished-episode records
    are read back every ``drain_every`` chunks only (default: as many chunks as the episode ring holds,
    :func:`default_drain_every`; a ring that overflows drops records and counts them in
    ``summary.dropped_episode_records``).  The host therefore runs ahead of the GPU and the chunk costs what its
    kernels cost.  The host-side ``agent.decaying_ou_action_noise.epsilon`` is brought up to date when the loop ends.

    ``overlap=True`` rolls chunk i+1 on a second stream WHILE the learner runs its iterations on chunk i: the rollout
    then acts with a snapshot of the actor taken before those iterations (one chunk stale -- the single-GPU form of
    ``rl_train_sharded_ddpg(pipelined=True)``); everything else (replay contents, epsilon decay per finished
    generation, sampling) is ordered as in the synchronous loop, and the result is deterministic.  The default follows
    the reference's order: act with the weights of the last completed train().
    ``on_chunk(i, chunk, env)`` -- if given -- is called once chunk i's rollout, append and learner iterations are enqueued.

    An agent with parameter-space noise (``param_noise_stddev``) rolls every chunk with its PERTURBED actor, one
    perturbation for all envs of the chunk -- the chunk is the vector analogue of the reference's per-episode reset and
    of its adaption interval (training_editted.py:100-112): behind the learner iterations of chunk i the stddev is adapted
    on the obs0 of one freshly sampled batch (``agent.adapt_param_noise``) and the acting copy is perturbed anew with the
    adapted stddev -- both stream-ordered, no host read.  The learner trains ``actor_flat`` only.
    The adaption batch comes from the replay ring's own index stream (``replay.sample_indices``), so with the same seed the
    learner's later batches differ from those of an agent without parameter noise; the run stays deterministic.
    ``param_noise_cycle=True`` does the adapt and the re-perturb of the synchronous loop in ONE launch
    (``agent.param_noise_cycle``) instead of the composed sequence; stddev and acting copy carry the composed sequence's
    bits whenever both agree on which side of the desired distance the measured one lies (``ssc.h``).  It is the
    single-agent run :func:`rl_train_vec_ddpg_population` is defined against; ``overlap=True`` uses the cycle anyway.

    ``overlap=True`` with parameter noise: the rollouts act with one of TWO perturbed copies (chunk i with copy i & 1).
    On the learner stream, behind the iterations of chunk i, ONE launch (``agent.param_noise_cycle``) adapts the stddev on
    a fresh batch and writes copy (i + 1) & 1 -- the one rollout i + 1 reads -- and that rollout waits for the event
    recorded behind it, so no copy is read while it is written.  The acting copy is perturbed from the actor as of the END
    of train i: the noise centre is NOT one chunk stale, while the plain overlap snapshot is; the price is that rollout
    i + 1 starts behind the learner iterations of chunk i instead of beside them (the rollout still runs on its own
    stream, and the host still runs ahead).  With normalize_observations the cycle reads the live statistics block on the
    learner stream and the rollout the snapshot.  As in the synchronous loop, only the adaption is skipped while the ring
    holds fewer than ``batch_size`` records.  When the loop ends ``agent.perturbed_actor_flat`` holds the last copy.

    ``stats_every=k``: the training diagnostics of the reference (``agent.get_stats_device``, training_editted.py:144)
    behind the learner iterations -- and the adapt / re-perturb, so the perturbed actor measured is the one the next chunk
    acts with -- of every chunk i with (i + 1) % k == 0, written into row i // k of a DEVICE log
    [ceil(num_chunks / k), SSC_DDPG_N_STATS] on the learner's stream; no host read.  The sample is fixed at the first such
    chunk whose ring holds ``batch_size`` records (drawn under a key of its own: the learner's batches do not move; a sample
    the agent already has is kept); rows before that, and a last row whose chunk the loop never reaches, stay NaN.  The log
    is copied to the host once, when the loop ends: ``summary.agent_stats`` (name -> float64 array, one entry per row) and
    ``summary.agent_stats_chunks`` (the chunk number of each row).  Everything else the loop computes is bit-identical to
    the run without it.

    A Pop-Art agent (``normalize_returns`` with ``enable_popart``: the learner moves the return statistics and rescales both
    critics' output layers, four launches per iteration) runs in both loop forms: the critic and the block are touched on
    the learner's stream only.  With ``stats_every`` the fp32 (mean, std) of ``agent.ret_rms`` is logged on the device beside
    every diagnostics row: ``summary.ret_rms`` (``mean``, ``std`` arrays, NaN where the row is).

    ``eval_env`` + ``eval_every=k``: the evaluation block of the reference (training_editted.py:122-138, 160-164) --
    ``agent.evaluate_device(eval_env, eval_steps)``: the plain actor without noise on a VecEnv of its own, eval/return,
    eval/Q, eval/episodes -- behind the learner iterations (and the adapt / re-perturb) of every chunk i with
    (i + 1) % k == 0, into row i // k of a DEVICE log [ceil(num_chunks / k), SSC_DDPG_N_EVAL] pre-filled with NaN, on the
    learner's stream; in the overlapped loop behind the ``snap_ready`` record, so rollout i + 1 does not wait for it.
    ``eval_steps`` defaults to ``eval_env.spec.max_episode_steps`` or 1000.  No host read; the log is copied out once, when
    the loop ends: ``summary.eval_stats`` (name -> float64 array) and ``summary.eval_chunks``.  The eval envs keep
    their episodes from one evaluation to the next.  Everything else the loop computes is bit-identical to the run without it.
    Returns (Summary, losses per chunk, replay)."""
    param_noise = getattr(agent, "param_noise", None) is not None
    if stats_every is not None and (int(stats_every) != stats_every or stats_every < 1):
        raise ValueError("stats_every must be None or a positive integer")
    if (eval_env is None) != (eval_every is None):
        raise ValueError("eval_env and eval_every come together")
    if eval_env is not None:
        if eval_env is env:
            raise ValueError("eval_env must be an env of its own, not the training env")
        for what in ("observation_space", "action_space"):
            ea, eb = getattr(eval_env, what), getattr(env, what)
            if tuple(ea.shape) != tuple(eb.shape) or not (np.array_equal(ea.low, eb.low) and np.array_equal(ea.high, eb.high)):
                raise ValueError(f"eval_env's {what} differs from the training env's")
        if eval_steps is None:
            eval_steps = getattr(getattr(eval_env, "spec", None), "max_episode_steps", None) or 1000
        for name, v in (("eval_every", eval_every), ("eval_steps", eval_steps)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be a positive integer")
        eval_every, eval_steps = int(eval_every), int(eval_steps)
    elif eval_steps is not None:
        raise ValueError("eval_steps needs eval_env and eval_every")
    if param_noise and overlap and not hasattr(agent, "param_noise_cycle"):
        raise NotImplementedError("rl_train_vec_ddpg: overlap=True with param_noise needs an agent with param_noise_cycle "
                                  "(the one-launch adapt and re-perturb)")
    import torch
    summary = Summary("vec_ddpg_" + env.spec.id)
    ring, chunk, replay = vec_loop_buffers(env, chunk_steps, replay_capacity, ring_capacity, seed, track_episodes)
    losses = []
    if drain_every is None:
        drain_every = default_drain_every(ring_capacity, env.n, chunk_steps)
    schedule = epsilon_schedule(agent, env.n, env.device)   # once per episode PER ENV (DDPG_Baselines_agent.py:255-258)
    finished, finished0 = env.stats[3:4], float(env.stats[3].item())   # the env may have run before: count from here
    dropped = 0

    def after_rollout():
        schedule.update(finished, finished0)

    def drain():
        nonlocal dropped
        (ids, lens, rets), d = ring.drain()
        dropped += d
        summary.extend_records(lens, rets)

    stats_log = None
    if stats_every is not None:
        from ._ffi import SSC_DDPG_N_STATS
        stats_every = int(stats_every)
        stats_log = torch.full((-(-num_chunks // stats_every), SSC_DDPG_N_STATS), float("nan"), dtype=torch.float64,
                               device=env.device)
    # Pop-Art: (mean, std) of the return statistics beside every diagnostics row, formed on the device
    ret_rms = getattr(agent, "ret_rms", None)
    ret_log = None
    if stats_log is not None and ret_rms is not None:
        ret_log = torch.full((stats_log.shape[0], 2), float("nan"), dtype=torch.float32, device=env.device)

    def log_stats(i, perturbed=None):
        """the diagnostics of chunk i, enqueued on the current (learner) stream"""
        if stats_log is None or (i + 1) % stats_every != 0:
            return
        if getattr(agent, "stats_sample", None) is None and len(replay) < agent.batch_size:
            return                                               # no sample yet: the row stays NaN
        agent.get_stats_device(replay, out=stats_log[i // stats_every], perturbed=perturbed)
        if ret_log is not None:
            mean, std = ret_rms.mean_std_device()
            ret_log[i // stats_every, 0:1].copy_(mean)
            ret_log[i // stats_every, 1:2].copy_(std)

    eval_log = None
    if eval_env is not None:
        from ._ffi import SSC_DDPG_N_EVAL
        eval_log = torch.full((-(-num_chunks // eval_every), SSC_DDPG_N_EVAL), float("nan"), dtype=torch.float64,
                              device=env.device)

    def log_eval(i):
        """the evaluation behind chunk i, enqueued on the current (learner) stream"""
        if eval_log is not None and (i + 1) % eval_every == 0:
            agent.evaluate_device(eval_env, eval_steps, out=eval_log[i // eval_every])

    def finish():
        drain()
        summary.dropped_episode_records = dropped
        _g, (eps,) = schedule.read()
        agent.decaying_ou_action_noise.epsilon = eps
        if stats_log is not None:
            host = stats_log.cpu().numpy()
            summary.agent_stats = {name: host[:, j].copy() for j, name in enumerate(agent.STATS_NAMES)}
            summary.agent_stats_chunks = [(r + 1) * stats_every - 1 for r in range(host.shape[0])]
        if ret_log is not None:
            host = ret_log.cpu().numpy()
            summary.ret_rms = {"mean": host[:, 0].copy(), "std": host[:, 1].copy()}
        if eval_log is not None:
            host = eval_log.cpu().numpy()
            summary.eval_stats = {name: host[:, j].copy() for j, name in enumerate(agent.EVAL_NAMES)}
            summary.eval_chunks = [(r + 1) * eval_every - 1 for r in range(host.shape[0])]

    if overlap:
        import dataclasses
        from .agents import views_like
        from .vec_env import TransitionChunk
        cur = torch.cuda.current_stream(env.device)
        with torch.cuda.device(env.device):              # env.device need not be the process's current device
            act = torch.cuda.Stream(env.device)          # the rollouts' stream
        chunks = [chunk, TransitionChunk(env.obs_dim, chunk_steps, env.n, env.device)]
        snap = agent.actor_flat.clone()                  # the weights the NEXT rollout acts with
        rms = getattr(agent, "obs_rms", None)
        rms_snap = rms.block.clone() if rms is not None else None   # ... and the observation statistics (normalize_observations)
        rolled2 = [torch.cuda.Event(), torch.cuda.Event()]
        appended = [torch.cuda.Event(), torch.cuda.Event()]
        snap_ready = torch.cuda.Event()
        live = agent.as_policy(device_epsilon=True)

        def policy_over(flat):                           # the live policy over another flat array and the statistics snapshot
            return env.policy_desc(dataclasses.replace(live, weights=views_like(flat, agent.weights), d_obs_rms=rms_snap))

        if param_noise:                                  # rollout i acts with perturbed copy i & 1
            acting = [agent.perturbed_actor_flat, torch.empty_like(agent.perturbed_actor_flat)]
            pds = [policy_over(acting[0]), policy_over(acting[1])]
            agent.perturb_policy()                       # copy 0, as the synchronous loop perturbs in front of chunk 0
        else:
            pds = [policy_over(snap)] * 2
        act.wait_stream(cur)

        drained = torch.cuda.Event()

        def launch_rollout(b, wait_for):
            for e in wait_for:
                act.wait_event(e)
            with torch.cuda.stream(act):
                env.rollout(chunk_steps, out=chunks[b], ring=ring, policy_desc=pds[b])
                after_rollout()
                rolled2[b].record(act)

        snap_ready.record(cur)
        launch_rollout(0, [snap_ready])
        for i in range(num_chunks):
            b = i & 1
            cur.wait_event(rolled2[b])
            replay.append_chunk(chunks[b], reward_scale=agent.reward_scale, last_steps=replay_last_steps)
            update_obs_rms(agent, chunks[b], replay_last_steps)
            appended[b].record(cur)
            if not param_noise:
                snap.copy_(agent.actor_flat)             # behind train i-1 on this stream, in front of train i
            if rms_snap is not None:
                rms_snap.copy_(rms.block)                # (the side-stream rollout must not read the block while it is updated)
            if not param_noise:
                snap_ready.record(cur)
            l = agent.train_from(replay, train_iters)
            if l is not None:
                losses.append(l)
            if param_noise:                              # copy b ^ 1 = actor as of the end of train i + noise of the adapted stddev
                adapt_and_perturb(agent, replay, dst=acting[b ^ 1])
                snap_ready.record(cur)
            log_stats(i, acting[b ^ 1] if param_noise else None)   # behind the event: rollout i + 1 does not wait for it
            log_eval(i)                                  # likewise
            if on_chunk is not None:
                on_chunk(i, chunks[b], env)
            extra = []
            if (i + 1) % drain_every == 0:               # the ring holds the records of chunks <= i; rollout i+1 is not queued yet
                drain()
                drained.record(cur)                      # ... and must not start before the cursor reset
                extra = [drained]
            if i + 1 < num_chunks:                       # chunk buffer b^1 was last read by append i-1
                launch_rollout(b ^ 1, [snap_ready] + extra + ([appended[b ^ 1]] if i >= 1 else []))
        cur.wait_stream(act)
        if param_noise and num_chunks & 1:               # the last perturbation went into the second copy
            acting[0].copy_(acting[1])
        finish()
        return summary, losses, replay

    if param_noise:
        pd = env.policy_desc(agent.as_policy(device_epsilon=True, perturbed=True))   # views into perturbed_actor_flat
        agent.perturb_policy()
    else:
        pd = env.policy_desc(agent.as_policy(device_epsilon=True))   # weights are views into the flat parameter arrays
    for i in range(num_chunks):
        out = env.rollout(chunk_steps, out=chunk, ring=ring, policy_desc=pd)
        after_rollout()
        replay.append_chunk(out, reward_scale=agent.reward_scale, last_steps=replay_last_steps)
        update_obs_rms(agent, out, replay_last_steps)
        l = agent.train_from(replay, train_iters)
        if l is not None:
            losses.append(l)
        if param_noise:                                          # the next chunk's actor, with the adapted stddev
            adapt_and_perturb(agent, replay, cycle=bool(param_noise_cycle))
        log_stats(i)
        log_eval(i)
        if on_chunk is not None:
            on_chunk(i, out, env)
        if (i + 1) % drain_every == 0:
            drain()
    finish()
    return summary, losses, replay


# The population loop's rollouts, decays, appends and statistics updates: one launch per phase for all pairs (True), or the
# per-pair calls pair by pair as before those launches existed (False: the yardstick of tools/exp_ddpg_population.py).
POPULATION_FUSED_CHUNK = True


class PopulationMonitor:
    """What :func:`rl_train_vec_ddpg_population` logs beside the training of its P pairs -- the two things a sweep's agents
    are compared by -- with the meaning the keywords of the same names have in :func:`rl_train_vec_ddpg`, for all pairs at
    once: ``stats_every=k`` logs the training diagnostics, ``eval_envs`` + ``eval_every=k`` the evaluation block
    (``eval_steps`` steps of every eval env; default: the eval envs' ``spec.max_episode_steps`` or 1000).  ``eval_envs``: one
    VecEnv per pair, each an env of its own -- not a training env, none used twice -- with the spaces of its pair's training
    env."""

    def __init__(self, eval_envs=None, eval_every=None, eval_steps=None, stats_every=None):
        self.eval_envs = None if eval_envs is None else list(eval_envs)
        self.eval_every, self.eval_steps, self.stats_every = eval_every, eval_steps, stats_every

    def checked(self, envs):
        """(eval_envs, eval_every, eval_steps, stats_every) validated against the training envs as the single loop validates
        its keywords; ValueError otherwise."""
        stats_every, eval_envs, eval_every, eval_steps = self.stats_every, self.eval_envs, self.eval_every, self.eval_steps
        if stats_every is not None and (int(stats_every) != stats_every or stats_every < 1):
            raise ValueError("stats_every must be None or a positive integer")
        if (eval_envs is None) != (eval_every is None):
            raise ValueError("eval_envs and eval_every come together")
        if eval_envs is None:
            if eval_steps is not None:
                raise ValueError("eval_steps needs eval_envs and eval_every")
            return None, None, None, None if stats_every is None else int(stats_every)
        if len(eval_envs) != len(envs):
            raise ValueError("eval_envs: one eval env per pair")
        if any(e is t for e in eval_envs for t in envs):
            raise ValueError("eval_envs must be envs of their own, not training envs")
        if len({id(e) for e in eval_envs}) != len(eval_envs):
            raise ValueError("eval_envs: no eval env may serve two pairs")
        for p, (ev, env) in enumerate(zip(eval_envs, envs)):
            for what in ("observation_space", "action_space"):
                ea, eb = getattr(ev, what), getattr(env, what)
                if tuple(ea.shape) != tuple(eb.shape) or not (np.array_equal(ea.low, eb.low) and np.array_equal(ea.high, eb.high)):
                    raise ValueError(f"pair {p}: eval env's {what} differs from the training env's")
        if eval_steps is None:
            steps = {getattr(getattr(ev, "spec", None), "max_episode_steps", None) or 1000 for ev in eval_envs}
            if len(steps) != 1:
                raise ValueError("the eval envs' episode limits differ: give eval_steps (one value for the population)")
            eval_steps = steps.pop()
        for name, v in (("eval_every", eval_every), ("eval_steps", eval_steps)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be a positive integer")
        return eval_envs, int(eval_every), int(eval_steps), None if stats_every is None else int(stats_every)


def rl_train_vec_ddpg_population(envs, agents, num_chunks, chunk_steps=256, replay_capacity=1 << 20, train_iters=None,
                                 replay_last_steps=None, seed=0, ring_capacity=1 << 20, track_episodes=False, overlap=False,
                                 drain_every=None, on_chunk=None, stats_every=None, eval_env=None, eval_every=None,
                                 eval_steps=None, monitor=None, param_noise_cycle=False):
    """The synchronous :func:`rl_train_vec_ddpg` for P (env, agent) pairs -- seeds x hyper-parameter grids, the reference's
    experimenter.py fan-out -- with ONE learner launch per chunk for the whole population
    (:class:`agents.DDPGPopulation`): per chunk every pair rolls out, decays its epsilon, appends to its own replay ring
    and updates its observation statistics exactly as the single loop does, then ``population.train_from`` trains all
    agents.  Every pair's parameters, losses, Summary and final epsilon are bit for bit those of its own
    ``rl_train_vec_ddpg`` run with the same arguments.  ``seed``: one replay seed for all pairs or one per pair.
    A population the one launch does not serve is split by ``train_from`` itself (see :class:`agents.DDPGPopulation`): the
    agents on the multi-workgroup kernels -- wider layers, other batch sizes, LayerNorm, critic_l2_reg, clip_norm -- train
    together in grouped launches, those of the shipped shape in one-workgroup launches per (obs_dim, lastLayerTanh,
    statistics) key, and only the rest (Pop-Art, a lone wide agent, ...) agent by agent; this loop needs, and has, no code
    of its own for that.  The rollouts, epsilon decays, replay appends and statistics updates
    of a chunk are ONE launch each for all pairs too (``vec_env.VecEnvPopulation``, ``DecayScheduleGroup``,
    ``replay_buffer.DeviceReplayPopulation``, ``obs_rms.ObsRmsGroup``; two launches for the statistics), each falling back to
    the per-pair calls for a population it does not serve (mixed env kinds, another actor shape or precision, mixed
    statistics, shared arrays).

    ``monitor``: a :class:`PopulationMonitor` -- diagnostics and evaluation for all pairs, each ONE call of
    ``population.get_stats_device`` / ``population.evaluate_device`` (two launches for the whole population) behind the
    learner launch of every chunk i with (i + 1) % k == 0, into DEVICE logs [ceil(num_chunks / k), P, .] pre-filled with
    NaN; no host read inside the loop.  A pair whose replay ring holds fewer than ``batch_size`` records and has no sample yet
    keeps a NaN diagnostics row.  When the loop ends every pair's Summary gets ``agent_stats``, ``agent_stats_chunks``,
    ``eval_stats`` and ``eval_chunks`` (and ``ret_rms`` for a Pop-Art agent) exactly as :func:`rl_train_vec_ddpg` fills them
    for ``stats_every=`` / ``eval_env=`` / ``eval_every=`` / ``eval_steps=``, bit for bit; everything else the loop computes
    is bit-identical to the run without a monitor.

    ``param_noise_cycle=True``: agents with parameter-space noise may be part of the population, mixed with plain ones.  The
    keyword has the meaning it has in :func:`rl_train_vec_ddpg` -- adapt and re-perturb in the one-launch cycle form -- and the
    population loop has no other form: without it a noisy agent keeps raising NotImplementedError, as the single loop's default
    (the composed sequence, other bits wherever the two forms disagree on the side of the desired distance) is not what this
    loop would compute.  A noisy pair rolls out with its perturbed actor, and ONE ``population.param_noise_cycle`` (one sampling launch and one cycle launch for all noisy agents)
    stands in front of chunk 0 (every ring is empty: perturb only, the single loop's ``perturb_policy()``) and behind the
    learner launch of every chunk, in front of the monitor -- so the diagnostics see the copy the next chunk acts with.
    Such a pair equals, bit for bit, its own ``rl_train_vec_ddpg(..., param_noise_cycle=True)`` run.

    Not in this form: ``overlap`` (NotImplementedError).  The single loop's keywords
    ``stats_every`` and ``eval_env`` / ``eval_every`` / ``eval_steps`` take one value, not one per pair: they raise
    NotImplementedError too and point to ``monitor``.  ``on_chunk(i, chunks, envs)`` gets the lists.  Returns
    [(Summary, losses per chunk, replay)] per pair."""
    from .agents import DDPGPopulation
    envs, agents = list(envs), list(agents)
    if len(envs) != len(agents) or not agents:
        raise ValueError("one env per agent, at least one pair")
    for what, on in (("stats_every", stats_every is not None),
                     ("eval_env / eval_every / eval_steps", not (eval_env is None and eval_every is None and eval_steps is None))):
        if on:
            raise NotImplementedError(f"rl_train_vec_ddpg_population: {what} is a keyword of the single loop; the population loop "
                                      "takes monitor=PopulationMonitor(eval_envs=, eval_every=, eval_steps=, stats_every=)")
    if overlap:
        raise NotImplementedError("rl_train_vec_ddpg_population: overlap=True is not part of the population loop; "
                                  "run that pair through rl_train_vec_ddpg")
    if not param_noise_cycle and any(getattr(a, "param_noise", None) is not None for a in agents):
        raise NotImplementedError("rl_train_vec_ddpg_population: an agent with parameter-space noise runs in the cycle form only: pass "
                                  "param_noise_cycle=True (each pair then equals its rl_train_vec_ddpg(..., param_noise_cycle=True) run), "
                                  "or run that pair through rl_train_vec_ddpg")
    eval_envs, eval_every, eval_steps, stats_every = (monitor if monitor is not None else PopulationMonitor()).checked(envs)
    P = len(agents)
    seeds = [int(seed)] * P if isinstance(seed, (int, np.integer)) else [int(s) for s in seed]
    if len(seeds) != P:
        raise ValueError("seed: one value or one per pair")
    population = DDPGPopulation(agents)
    summaries = [Summary("vec_ddpg_" + env.spec.id) for env in envs]
    bufs = [vec_loop_buffers(env, chunk_steps, replay_capacity, ring_capacity, s, track_episodes) for env, s in zip(envs, seeds)]
    rings, chunks, replays = ([b[k] for b in bufs] for k in range(3))
    losses = [[] for _ in range(P)]
    every = [default_drain_every(ring_capacity, env.n, chunk_steps) if drain_every is None else drain_every for env in envs]
    schedules = [epsilon_schedule(agent, env.n, env.device) for env, agent in zip(envs, agents)]
    finished0 = [float(env.stats[3].item()) for env in envs]
    dropped = [0] * P

    def drain(p):
        (_ids, lens, rets), d = rings[p].drain()
        dropped[p] += d
        summaries[p].extend_records(lens, rets)

    noisy = [getattr(a, "param_noise", None) is not None for a in agents]
    # a noisy pair acts with its perturbed copy (views into perturbed_actor_flat)
    pds = [env.policy_desc(agent.as_policy(device_epsilon=True, perturbed=True) if pn else agent.as_policy(device_epsilon=True))
           for env, agent, pn in zip(envs, agents, noisy)]
    # the rest of the chunk, one launch per phase for all pairs (a population a launch does not serve: pair by pair inside)
    from .obs_rms import ObsRmsGroup
    from .population import PairCursors
    from .replay_buffer import DeviceReplayPopulation
    from .vec_env import VecEnvPopulation
    env_pop, replay_pop, decays = VecEnvPopulation(envs), DeviceReplayPopulation(replays), DecayScheduleGroup(schedules)
    normed = [p for p, a in enumerate(agents) if getattr(a, "obs_rms", None) is not None]
    rms_group = ObsRmsGroup([agents[p].obs_rms for p in normed]) if normed else None
    cursors = PairCursors(P, envs[0].device) if POPULATION_FUSED_CHUNK and all(e.device == envs[0].device for e in envs) else None
    scales = [a.reward_scale for a in agents]
    # the monitor's device logs [rows, P, .]: each call writes ONE block [P, .] the population keeps its descriptors over,
    # copied into its row on the stream (NaN where a pair has no sample yet)
    import torch
    from ._ffi import SSC_DDPG_N_EVAL, SSC_DDPG_N_STATS
    dev = envs[0].device
    nan_log = lambda every, cols: (torch.full((-(-num_chunks // every), P, cols), float("nan"), dtype=torch.float64, device=dev),
                                   torch.full((P, cols), float("nan"), dtype=torch.float64, device=dev))
    stats_log, stats_block = nan_log(stats_every, SSC_DDPG_N_STATS) if stats_every is not None else (None, None)
    eval_log, eval_block = nan_log(eval_every, SSC_DDPG_N_EVAL) if eval_envs is not None else (None, None)
    popart = [p for p, a in enumerate(agents) if getattr(a, "ret_rms", None) is not None] if stats_log is not None else []
    ret_log = torch.full((stats_log.shape[0], P, 2), float("nan"), dtype=torch.float32, device=dev) if popart else None

    def log_monitor(i):
        """the diagnostics and the evaluation behind chunk i, enqueued behind its learner launch"""
        if stats_log is not None and (i + 1) % stats_every == 0:
            population.get_stats_device(replays, out=stats_block)
            stats_log[i // stats_every].copy_(stats_block)
            for p in popart:
                if getattr(agents[p], "stats_sample", None) is not None:
                    mean, std = agents[p].ret_rms.mean_std_device()
                    ret_log[i // stats_every, p, 0:1].copy_(mean)
                    ret_log[i // stats_every, p, 1:2].copy_(std)
        if eval_log is not None and (i + 1) % eval_every == 0:
            population.evaluate_device(eval_envs, eval_steps, out=eval_block)
            eval_log[i // eval_every].copy_(eval_block)

    if any(noisy):
        population.param_noise_cycle(replays)     # every ring is empty: the perturbation in front of chunk 0
    for i in range(num_chunks):
        if cursors is None:                       # the per-pair calls, pair by pair
            for p, (env, agent) in enumerate(zip(envs, agents)):
                out = env.rollout(chunk_steps, out=chunks[p], ring=rings[p], policy_desc=pds[p])
                schedules[p].update(env.stats[3:4], finished0[p])
                replays[p].append_chunk(out, reward_scale=agent.reward_scale, last_steps=replay_last_steps)
                update_obs_rms(agent, out, replay_last_steps)
        else:
            # what changes with the chunk: 16 bytes per pair, known before the rollout -- the one upload of a steady-state chunk
            cursors.stage(step0=[env.t for env in envs], replay_start=[r.count for r in replays]).upload()
            outs = env_pop.rollout(chunk_steps, pds, chunks, rings, cursors=cursors)
            decays.update([env.stats[3:4] for env in envs], finished0)
            replay_pop.append_chunks(outs, reward_scale=scales, last_steps=replay_last_steps, cursors=cursors)
            kept = chunk_steps if replay_last_steps is None else min(int(replay_last_steps), chunk_steps)
            if rms_group is not None and kept > 0:
                rms_group.update_chunks([outs[p] for p in normed], chunk_steps - kept, chunk_steps)
        for p, l in enumerate(population.train_from(replays, train_iters, copy=True)):
            if l is not None:
                losses[p].append(l)
        if any(noisy):                            # the next chunk's acting copies, with the adapted stddevs
            population.param_noise_cycle(replays)
        log_monitor(i)
        if on_chunk is not None:
            on_chunk(i, chunks, envs)
        for p in range(P):
            if (i + 1) % every[p] == 0:
                drain(p)
    stats_host, ret_host, eval_host = (None if log is None else log.cpu().numpy() for log in (stats_log, ret_log, eval_log))
    for p, agent in enumerate(agents):
        drain(p)
        summaries[p].dropped_episode_records = dropped[p]
        _g, (eps,) = schedules[p].read()
        agent.decaying_ou_action_noise.epsilon = eps
        if stats_host is not None:
            summaries[p].agent_stats = {name: stats_host[:, p, j].copy() for j, name in enumerate(agent.STATS_NAMES)}
            summaries[p].agent_stats_chunks = [(r + 1) * stats_every - 1 for r in range(stats_host.shape[0])]
        if ret_host is not None and p in popart:
            summaries[p].ret_rms = {"mean": ret_host[:, p, 0].copy(), "std": ret_host[:, p, 1].copy()}
        if eval_host is not None:
            summaries[p].eval_stats = {name: eval_host[:, p, j].copy() for j, name in enumerate(agent.EVAL_NAMES)}
            summaries[p].eval_chunks = [(r + 1) * eval_every - 1 for r in range(eval_host.shape[0])]
    return [(summaries[p], losses[p], replays[p]) for p in range(P)]


def rl_train_vec_smartstart(env, smart, num_chunks, chunk_steps=64, replay_capacity=1 << 20, train_iters=None,
                            replay_last_steps=None, seed=0, ring_capacity=1 << 20, refresh_every=1, graph=True,
                            on_chunk=None, aggregate_every=0, aggregate_kwargs=None, overlap_selection=False):
    """The vectorised SmartStart loop: rlTrain (rlTrain.py:63-114) with ``SmartStartContinuous(DDPG_Baselines_agent)``
    (smartexplorationcontinuous.py:307-376) for all envs of ``env`` at once, everything in HBM.  Per chunk:
    smart-start selection on the device replay ring -> plans on offer (``smart.refresh_plans``, every ``refresh_every``
    chunks), ``chunk_steps`` steps of every env in its own mode (``smart.rollout``), the chunk appended to the ring
    (episode index kept on the device), ``train_iters`` DDPG iterations, and the finished episodes read back for the
    epsilon / eta decay (once per episode per env, like DDPG_Baselines_agent.end_episode :255-258 and
    SmartStartContinuous.end_episode :372-376).  ``aggregate_every`` > 0 retrains the navigator's dynamics model on the
    ring every that many chunks (``smart.train_dynamics_model``: the reference does it every
    ``num_episodes_for_aggregation`` planned episodes, NND_MB_agent.py:420-423).  ``smart``: :class:`smartstart.VecSmartStart`.

    ``overlap_selection=True``: the selection of chunk c runs WHILE chunk c rolls -- its kernels (candidates, Q(s, pi(s)),
    KDE, UCB) on a side stream that fills the gaps between the rollout's launches, its host part (episodic paths, path
    shortcutting, waypoints) while the GPU works through the queued steps -- and the plans it produces go on offer for chunk
    c + 1 (published on the rollout's stream behind chunk c: deterministic).  The selection then sees the ring as of chunk
    c - 1 and its plans are used one chunk later than in the sequential loop; the chunk costs max(rollout, selection)
    instead of their sum.

    A base agent with parameter-space noise (``param_noise_stddev``): the per-step actor launch of the envs in agent mode
    reads the PERTURBED actor (``VecSmartStart.acting_desc``), and once per chunk, behind the learner iterations, ONE launch
    (``agent.param_noise_cycle``) adapts the stddev on the obs0 of a fresh replay batch and perturbs the acting copy anew
    (only the perturbation while the ring holds fewer than ``batch_size`` records).  The OU noise is still added as
    configured; navigating steps are untouched; the selection's Q(s, pi(s)) uses the plain actor.
    Returns (Summary, losses per chunk, replay)."""
    base = getattr(smart, "agent", None)
    if getattr(base, "ret_rms", None) is not None:
        raise NotImplementedError("rl_train_vec_smartstart: a base agent with normalize_returns / Pop-Art is not supported "
                                  "(the selection reads the raw critic)")
    if getattr(base, "param_noise", None) is not None and not hasattr(base, "param_noise_cycle"):
        raise NotImplementedError("rl_train_vec_smartstart: a base agent with param_noise needs param_noise_cycle "
                                  "(the one-launch adapt and re-perturb)")
    import torch
    agent = smart.agent
    summary = Summary("vec_smartstart_" + env.spec.id)
    ring, chunk, replay = vec_loop_buffers(env, chunk_steps, replay_capacity, ring_capacity, seed, True)
    losses, generations = [], 0.0
    if overlap_selection:
        main = torch.cuda.current_stream(env.device)
        with torch.cuda.device(env.device):
            side = torch.cuda.Stream(env.device)
        learned = torch.cuda.Event()
    for c in range(num_chunks):
        if aggregate_every and c > 0 and c % aggregate_every == 0:
            smart.train_dynamics_model(replay, **(aggregate_kwargs or {}))
        plans = None
        if overlap_selection:
            out = smart.rollout(chunk_steps, chunk, ring=ring, graph=graph)         # chunk c is queued; the host is free
            if c % refresh_every == 0 and c > 0:
                side.wait_event(learned)                                            # the ring and the networks as of chunk c - 1
                with torch.cuda.stream(side):
                    plans = smart.select_plans(replay)                              # kernels on the side stream, host geometry meanwhile
                main.wait_stream(side)                                              # (already complete: the host read its results)
            if plans:
                smart.publish_plans(plans)                                          # main stream, behind chunk c: on offer from chunk c + 1
        else:
            if c % refresh_every == 0:
                smart.refresh_plans(replay)
            out = smart.rollout(chunk_steps, chunk, ring=ring, graph=graph)
        replay.append_chunk(out, reward_scale=agent.reward_scale, last_steps=replay_last_steps)
        update_obs_rms(agent, out, replay_last_steps)
        l = agent.train_from(replay, train_iters)
        if overlap_selection:
            learned.record(main)
        if getattr(agent, "param_noise", None) is not None:      # the next chunk's acting copy, with the adapted stddev
            adapt_and_perturb(agent, replay)
        if l is not None:
            losses.append(l)
        if on_chunk is not None:
            on_chunk(c, out, smart)
        (ids, lens, rets), _d = ring.drain()
        summary.extend_records(lens, rets)
        generations += len(lens) / float(env.n)
        while generations >= 1.0:
            agent.decaying_ou_action_noise.reduce_epsilon()
            smart.end_of_generation()
            generations -= 1.0
    return summary, losses, replay


def rl_train_vec_smartstart_population(env, smart_population, num_chunks, chunk_steps=64, replay_capacity=1 << 20,
                                       train_iters=None, replay_last_steps=None, seed=0, ring_capacity=1 << 20, refresh_every=1,
                                       graph=True, on_chunk=None, aggregate_every=0, aggregate_kwargs=None,
                                       overlap_selection=False, grouped_selection=False):
    """The synchronous loop of :func:`rl_train_vec_smartstart` for ALL pairs of a :class:`smartstart.VecSmartStartPopulation`
    -- the seeds and hyper-parameters of SmartStart_DDPG_Baselines_experimenter.py -- on the ONE ``env`` that holds every
    pair's envs.  Per chunk: every pair's smart-start selection on its own ring (every ``refresh_every`` chunks; its
    dynamics-model aggregation every ``aggregate_every``), ONE rollout of all pairs (one captured graph), every pair's
    replay append from a strided column view of the one chunk (``TransitionChunk.from_columns`` over ``[..., env0:env0 + n]``,
    row stride kept), ``ObsRmsGroup`` for the normalising pairs, ``DDPGPopulation.train_from``,
    ``DDPGPopulation.param_noise_cycle`` for the noisy pairs, ONE drain of the episode ring split by env id into the pairs'
    Summaries, and every pair's epsilon / eta decay once per episode per env of the pair.  Every pair's Summary, losses,
    replay ring, agent parameters and final eta / epsilon are those of its own ``rl_train_vec_smartstart`` run on
    ``VecEnv(n_p, env_id0 + env0_p)`` with the same arguments.  ``seed``: one replay seed for all pairs or one per pair.
    ``on_chunk(c, out, smart_population)``.  Not in this form: ``overlap_selection=True`` (NotImplementedError).
    ``grouped_selection=True``: every due ``train_dynamics_model`` runs first (each touches only its own model, which the
    selection does not read), then ONE ``smart_population.refresh_plans(replays)`` selects for all pairs in one launch per
    stage with one host wait; the Scott bandwidth is then summed in the device's fixed order, so pdf, ucb and possibly the
    chosen starts differ in the last bits from the default, which keeps the per-pair calls and their bits.
    Returns [(Summary, losses per chunk, replay)] per pair."""
    if overlap_selection:
        raise NotImplementedError("rl_train_vec_smartstart_population: overlap_selection=True is not part of the population loop; "
                                  "run that pair through rl_train_vec_smartstart")
    from .agents import DDPGPopulation
    from .obs_rms import ObsRmsGroup
    from .replay_buffer import DeviceReplayBuffer
    from .vec_env import EpisodeRing, TransitionChunk
    pop, pairs = smart_population, smart_population.pairs
    agents, P = [pr.agent for pr in pairs], len(pairs)
    for a in agents:
        if getattr(a, "ret_rms", None) is not None:
            raise NotImplementedError("rl_train_vec_smartstart_population: a base agent with normalize_returns / Pop-Art is not "
                                      "supported (the selection reads the raw critic)")
        if getattr(a, "param_noise", None) is not None and not hasattr(a, "param_noise_cycle"):
            raise NotImplementedError("rl_train_vec_smartstart_population: a base agent with param_noise needs param_noise_cycle")
    seeds = [int(seed)] * P if isinstance(seed, (int, np.integer)) else [int(s) for s in seed]
    if len(seeds) != P:
        raise ValueError("seed: one value or one per pair")
    population = DDPGPopulation(agents)
    summaries = [Summary("vec_smartstart_" + env.spec.id) for _ in pairs]
    ring, chunk = EpisodeRing(ring_capacity, env.device), TransitionChunk(env.obs_dim, chunk_steps, env.n, env.device)
    replays = [DeviceReplayBuffer(replay_capacity, env.obs_dim, 1, env.device, seed=s, track_episodes=True, n_envs=pr.n,
                                  max_path_len=(env.spec.max_episode_steps or 1000) + 1) for pr, s in zip(pairs, seeds)]
    sl = [slice(pr.env0, pr.env0 + pr.n) for pr in pairs]
    views = [TransitionChunk.from_columns(chunk.obs[..., s], chunk.act[:, s], chunk.rew[:, s], chunk.obs2[..., s], chunk.done[:, s])
             for s in sl]
    normed = [p for p, a in enumerate(agents) if getattr(a, "obs_rms", None) is not None]
    rms_group = ObsRmsGroup([agents[p].obs_rms for p in normed]) if normed else None
    noisy = any(getattr(a, "param_noise", None) is not None for a in agents)
    kept = chunk_steps if replay_last_steps is None else min(int(replay_last_steps), chunk_steps)
    losses, generations = [[] for _ in pairs], [0.0] * P
    for c in range(num_chunks):
        if grouped_selection:
            if aggregate_every and c > 0 and c % aggregate_every == 0:
                for p, pr in enumerate(pairs):
                    pr.train_dynamics_model(replays[p], **(aggregate_kwargs or {}))
            if c % refresh_every == 0:
                pop.refresh_plans(replays)
        else:
            for p, pr in enumerate(pairs):
                if aggregate_every and c > 0 and c % aggregate_every == 0:
                    pr.train_dynamics_model(replays[p], **(aggregate_kwargs or {}))
                if c % refresh_every == 0:
                    pr.refresh_plans(replays[p])
        out = pop.rollout(chunk_steps, chunk, ring=ring, graph=graph)
        for p, pr in enumerate(pairs):
            views[p].step0, views[p].env_id0 = out.step0, out.env_id0 + pr.env0
            replays[p].append_chunk(views[p], reward_scale=agents[p].reward_scale, last_steps=replay_last_steps)
        if rms_group is not None and kept > 0:
            rms_group.update_chunks([views[p] for p in normed], chunk_steps - kept, chunk_steps)
        for p, l in enumerate(population.train_from(replays, train_iters, copy=True)):
            if l is not None:
                losses[p].append(l)
        if noisy:                                 # the next chunk's acting copies, with the adapted stddevs
            population.param_noise_cycle(replays)
        if on_chunk is not None:
            on_chunk(c, out, pop)
        (ids, lens, rets), _d = ring.drain()
        for p, pr in enumerate(pairs):
            mine = (ids >= env.env_id0 + pr.env0) & (ids < env.env_id0 + pr.env0 + pr.n)
            summaries[p].extend_records(lens[mine], rets[mine])
            generations[p] += int(mine.sum()) / float(pr.n)
            while generations[p] >= 1.0:
                agents[p].decaying_ou_action_noise.reduce_epsilon()
                pr.end_of_generation()
                generations[p] -= 1.0
    return [(summaries[p], losses[p], replays[p]) for p in range(P)]
