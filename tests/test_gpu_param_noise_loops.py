"""Parameter-space noise on the overlapped DDPG loop and on the vectorised SmartStart loop: MountainCar, 256 envs, chunks of
32 steps, 4 chunks, batch 64, fixed seeds."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests.test_gpu_navigator import make_mlp, make_norm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_ENVS, K, CHUNKS, BATCH, ITERS = 256, 32, 4, 64, 2
ENV = "MountainCarContinuous-v0"


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def make_agent(ssc, noise=True, **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    args = dict(batch_size=BATCH, num_train_iterations=ITERS, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32,
                lastLayerTanh=True, seed=7)
    if noise:
        args["param_noise_stddev"] = 0.2
    args.update(kw)
    return DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, **args)


RING = ("s", "a", "r", "t", "s2")


def run_overlapped(ssc):
    agent = make_agent(ssc)
    env = ssc.VecEnv(ENV, N_ENVS, seed=5)
    seen = []
    _, losses, replay = ssc.rl_train_vec_ddpg(env, agent, CHUNKS, chunk_steps=K, train_iters=ITERS, seed=3, overlap=True,
                                              replay_capacity=1 << 16,
                                              on_chunk=lambda i, c, e: seen.append(agent.d_param_noise_distance.clone()))
    torch.cuda.synchronize()
    return agent, replay, [float(d.item()) for d in seen], losses


def replay_by_hand(ssc):
    """The same stream-ordered calls, one after the other on one stream: rollout with perturbed copy b, append, train,
    cycle into copy b ^ 1."""
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    from smartstartcontinuous_amd.rl_train import epsilon_schedule
    from smartstartcontinuous_amd.vec_env import ActorPolicy, EpisodeRing, TransitionChunk
    agent = make_agent(ssc)
    env = ssc.VecEnv(ENV, N_ENVS, seed=5)
    ring = EpisodeRing(1 << 20, env.device)
    chunk = TransitionChunk(env.obs_dim, K, env.n, env.device)
    replay = DeviceReplayBuffer(1 << 16, env.obs_dim, 1, env.device, seed=3, track_episodes=False, n_envs=env.n,
                                max_path_len=(env.spec.max_episode_steps or 1000) + 1)
    schedule = epsilon_schedule(agent, env.n, env.device)
    finished, finished0 = env.stats[3:4], float(env.stats[3].item())
    live = agent.as_policy(device_epsilon=True)
    acting = [agent.perturbed_actor_flat, torch.empty_like(agent.perturbed_actor_flat)]

    def policy_over(flat):
        views, o = {}, 0
        for k, v in agent.weights.items():
            views[k] = flat[o:o + v.numel()].view(v.shape)
            o += v.numel()
        return env.policy_desc(ActorPolicy(views, last_layer_tanh=live.last_layer_tanh, precision=live.precision, ou_mu=live.ou_mu,
                                           ou_sigma=live.ou_sigma, ou_theta=live.ou_theta, ou_dt=live.ou_dt,
                                           obs_clip=live.obs_clip, d_ou_epsilon=agent.d_epsilon, d_obs_rms=None))
    pds = [policy_over(acting[0]), policy_over(acting[1])]
    agent.perturb_policy()
    distances, stddevs = [], []
    for i in range(CHUNKS):
        b = i & 1
        env.rollout(K, out=chunk, ring=ring, policy_desc=pds[b])
        schedule.update(finished, finished0)
        replay.append_chunk(chunk, reward_scale=agent.reward_scale, last_steps=None)
        agent.train_from(replay, ITERS)
        assert len(replay) >= BATCH
        rows = replay.sample_indices(1, BATCH)[0].long()
        distances.append(float(agent.param_noise_cycle(replay.s.index_select(0, rows), dst=acting[b ^ 1]).item()))
        stddevs.append(float(agent.d_param_noise_stddev.item()))
    torch.cuda.synchronize()
    return agent, replay, distances, stddevs, acting[CHUNKS & 1]


def test_overlapped_loop_with_param_noise(ssc):
    from smartstartcontinuous_amd.agents import AdaptiveParamNoiseSpec
    agent, replay, distances, losses = run_overlapped(ssc)
    again, replay2, distances2, _ = run_overlapped(ssc)
    hand, replay_h, distances_h, stddevs_h, last_copy = replay_by_hand(ssc)
    assert len(losses) == CHUNKS and len(distances) == CHUNKS and all(np.isfinite(d) and d > 0 for d in distances)
    assert distances == distances2 == distances_h
    for other, ring in ((again, replay2), (hand, replay_h)):
        for name in ("actor_flat", "d_param_noise_stddev", "critic_flat"):
            assert np.array_equal(bits(getattr(agent, name)), bits(getattr(other, name))), name
        assert len(ring) == len(replay) == N_ENVS * K * CHUNKS
        for col in RING:
            assert np.array_equal(bits(getattr(replay, col)), bits(getattr(ring, col))), col
        assert (agent.param_noise_generation, agent.perturbed_generation) == (other.param_noise_generation, other.perturbed_generation)
    # construction 0, in front of chunk 0: 1, then (adaptive, acting) = (2 + 2i, 3 + 2i) behind chunk i
    assert agent.perturbed_generation == 2 * CHUNKS + 1 and agent.param_noise_generation == 2 * CHUNKS + 2
    # when the loop ends the agent's own acting copy holds the last perturbation
    assert np.array_equal(bits(agent.perturbed_actor_flat), bits(last_copy))
    assert not np.array_equal(bits(agent.perturbed_actor_flat), bits(agent.actor_flat))
    assert not np.array_equal(bits(agent.actor_flat), bits(make_agent(ssc).actor_flat))          # the learner trained it
    # the stddev after 4 chunks: initial * coefficient^k, k dictated by the replayed distances (fp32, step by step)
    host = AdaptiveParamNoiseSpec(0.2, 0.2, 1.01)
    k = 0
    for d, sd in zip(distances_h, stddevs_h):
        host.adapt(d)
        k += -1 if np.float32(d) > np.float32(0.2) else 1
        assert sd == host.current_stddev
    assert float(agent.d_param_noise_stddev.item()) == host.current_stddev
    assert abs(host.current_stddev - 0.2 * 1.01 ** k) <= 1e-6 and k in range(-CHUNKS, CHUNKS + 1, 2)


def test_overlapped_loop_with_param_noise_and_observation_statistics(ssc):
    """normalize_observations: the cycle reads the live block, the rollout the snapshot; the run is deterministic"""
    def run():
        agent = make_agent(ssc, normalize_observations=True)
        env = ssc.VecEnv(ENV, N_ENVS, seed=5)
        ssc.rl_train_vec_ddpg(env, agent, CHUNKS, chunk_steps=K, train_iters=ITERS, seed=3, overlap=True, replay_capacity=1 << 16)
        torch.cuda.synchronize()
        return agent
    a, b = run(), run()
    for name in ("actor_flat", "perturbed_actor_flat", "d_param_noise_stddev"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert np.isfinite(float(a.d_param_noise_distance.item())) and float(a.d_param_noise_distance.item()) > 0
    assert float(a.d_param_noise_stddev.item()) != float(np.float32(0.2))


# ------------------------------------------------------------------------------------------------ SmartStart loop --
MAX_STEPS, EPS = 24, 0.8


def smart_setup(ssc, noise=True):
    from smartstartcontinuous_amd import navigator as nav
    rng = np.random.default_rng(2)
    env = ssc.VecEnv(ENV, N_ENVS, seed=2, max_episode_steps=MAX_STEPS, env_id0=40)
    env.reset()
    agent = make_agent(ssc, noise=noise, seed=5, ou_mu=0.4, ou_sigma=0.6, ou_epsilon=EPS, ou_epsilon_decay_factor=1.0,
                       precision="f32")
    Ws, bs = make_mlp(rng, (3, 32, 2))                               # the 1 x 32 dynamics model
    model = nav.DynamicsModel(Ws, bs, make_norm(rng, 2, 1), state_dim=2, act_dim=1, precision="f32")
    smart = ssc.VecSmartStart(env, agent, model, eta=0.9, n_plans=2, num_control_samples=16, horizon=3,
                              steps_before_giving_up_on_waypoint=2, final_steps=4, chunk_steps=K, seed=3, log_modes=True,
                              w_max=MAX_STEPS + 1)
    return env, agent, smart


def run_smart(ssc, graph):
    env, agent, smart = smart_setup(ssc)
    snaps = []

    def on_chunk(c, out, sm):
        # stream-ordered behind chunk c's cycle: the copies chunk c + 1 acts with, and chunk c's log
        snaps.append(dict(perturbed=agent.perturbed_actor_flat.clone(), plain=agent.actor_flat.clone(), ou=env.ou_x.clone(),
                          obs=out.obs.clone(), act=out.act.clone(), done=out.done.clone(), modes=sm.mode_log.clone(),
                          step0=out.step0, sd=agent.d_param_noise_stddev.clone(), gen=agent.perturbed_generation))
    _, losses, replay = ssc.rl_train_vec_smartstart(env, smart, CHUNKS, chunk_steps=K, replay_capacity=1 << 16,
                                                    train_iters=ITERS, seed=3, graph=graph, on_chunk=on_chunk)
    torch.cuda.synchronize()
    return env, agent, smart, snaps, losses


def weights64(agent, flat):
    out, o = {}, 0
    for k, v in agent.weights.items():
        out[k] = flat[o:o + v.numel()].reshape(v.shape).astype(np.float64)
        o += v.numel()
    return out


def test_smartstart_loop_acts_with_the_perturbed_actor(ssc):
    env, agent, smart, snaps, losses = run_smart(ssc, graph=True)
    assert len(losses) == CHUNKS and len(snaps) == CHUNKS
    assert [s["gen"] for s in snaps] == [2 * c + 2 for c in range(CHUNKS)]              # construction 0, then a pair per chunk
    sds = [float(s["sd"].item()) for s in snaps]
    assert all(a != b for a, b in zip([float(np.float32(0.2))] + sds, sds))             # every chunk adapted
    # chunk 3 re-derived: it acted with the copy chunk 2's cycle left behind
    c = CHUNKS - 1
    prev, cur = snaps[c - 1], snaps[c]
    obs, act = cur["obs"].cpu().numpy(), cur["act"].cpu().numpy()
    done, modes = cur["done"].cpu().numpy().astype(bool), cur["modes"].cpu().numpy().astype(bool)
    wp = weights64(agent, prev["perturbed"].cpu().numpy())
    wplain = weights64(agent, prev["plain"].cpu().numpy())
    ou = prev["ou"].cpu().numpy().astype(np.float64)
    ids = np.uint64(env.env_id0) + np.arange(N_ENVS, dtype=np.uint64)
    worst, largest_shift, n_agent, n_nav = 0.0, 0.0, 0, 0
    for k in range(K):
        t = cur["step0"] + k
        g = O.ou_gaussian(env._seed, ids, np.uint64(t))
        a_pert = O.actor_forward(obs[:, k, :].T, **wp, obs_clip=5.0)[:, 0]
        a_plain = O.actor_forward(obs[:, k, :].T, **wplain, obs_clip=5.0)[:, 0]
        acting = ~modes[k]
        ou = np.where(acting, O.ou_step(ou, g, 0.4, 0.6), ou)
        expect = O.ddpg_action(a_pert, ou, EPS)
        worst = max(worst, float(np.max(np.abs(expect - act[k])[acting])))
        largest_shift = max(largest_shift, float(np.max(np.abs(a_pert - a_plain)[acting])))
        n_agent += int(acting.sum())
        n_nav += int(modes[k].sum())
        for i in np.flatnonzero(modes[k])[:2]:                  # navigating steps are the MPC's: a drawn candidate + noise
            A = O.mpc_action_samples(smart.nav.seed, int(ids[i]), smart.nav.N, smart.nav.H, 1, t, [-1.0], [1.0])
            noise = 0.005 * O.mpc_noise_gaussian(smart.nav.seed, np.array([ids[i]], np.uint64), t, 0)[0]
            assert np.min(np.abs(A[:, 0, 0] + noise - act[k, i])) <= 1e-6, (k, i)
        ou = np.where(done[k], 0.0, ou)
    print(f"smartstart + param noise, chunk {c}: {n_agent} agent steps, {n_nav} navigating steps, max |action - oracle(perturbed)| "
          f"= {worst:.3e}, max |perturbed - plain| (fp64) = {largest_shift:.3e}")
    assert n_agent > 300 and n_nav > 100                        # both kinds of step in numbers (eta 0.9: most envs navigate)
    assert worst <= 2e-5
    assert largest_shift > 1e-3
    # the selection evaluates the PLAIN actor
    probe = torch.from_numpy(np.random.default_rng(1).uniform(-0.5, 0.5, size=(32, 2)).astype(np.float32)).cuda()
    q = agent.state_value_device(probe)
    assert torch.equal(q, agent.critic(probe, agent._forward(agent._desc, probe)).reshape(-1))
    assert not torch.equal(q, agent.critic(probe, agent._forward(agent._perturbed_desc, probe)).reshape(-1))


def test_smartstart_loop_graph_replay_equals_step_by_step(ssc):
    (_, ag, sg, snaps_g, _), (_, ae, se, snaps_e, _) = run_smart(ssc, graph=True), run_smart(ssc, graph=False)
    for a, b in zip(snaps_g, snaps_e):
        for name in ("perturbed", "plain", "ou", "obs", "act", "done", "modes", "sd"):
            assert torch.equal(a[name], b[name]), name
    assert int(snaps_g[-1]["modes"].sum()) > 0
    assert torch.equal(ag.actor_flat, ae.actor_flat) and torch.equal(sg.mode, se.mode)


def test_no_new_cost_without_param_noise(ssc, monkeypatch):
    """An agent without param_noise_stddev: no cycle launch, no new tensor attribute, in either loop."""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    calls = []
    monkeypatch.setattr(DDPG_Baselines_agent, "param_noise_cycle", lambda self, *a, **k: calls.append(a))

    def tensor_attrs(agent):
        return sorted(k for k, v in vars(agent).items() if torch.is_tensor(v))
    agent = make_agent(ssc, noise=False)
    before = tensor_attrs(agent)
    env = ssc.VecEnv(ENV, N_ENVS, seed=5)
    ssc.rl_train_vec_ddpg(env, agent, 2, chunk_steps=K, train_iters=ITERS, seed=3, overlap=True, replay_capacity=1 << 16)
    assert sorted(set(tensor_attrs(agent)) - {"_train_ws"}) == sorted(set(before) - {"_train_ws"})
    env, agent, smart = smart_setup(ssc, noise=False)
    before = tensor_attrs(agent)
    assert smart.acting_desc() is agent._desc
    ssc.rl_train_vec_smartstart(env, smart, 2, chunk_steps=K, replay_capacity=1 << 16, train_iters=ITERS, seed=3)
    torch.cuda.synchronize()
    assert sorted(set(tensor_attrs(agent)) - {"_train_ws"}) == sorted(set(before) - {"_train_ws"})
    assert calls == []
    for name in ("perturbed_actor_flat", "adaptive_actor_flat", "d_param_noise_stddev", "d_param_noise_distance"):
        assert not hasattr(agent, name), name
