"""``rl_train_vec_ddpg(stats_every=k)``: the diagnostics logged on the device change nothing the loop computes, land in the
rows they belong to, and measure the perturbed actor the next chunk acts with.  MountainCar, 257 envs, chunks of 32 steps,
6 chunks, batch 64, 3 iterations; ``max_episode_steps=60`` so that episodes finish and epsilon decays inside the run."""
import numpy as np
import pytest

from oracle import ssc_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_ENVS, K, CHUNKS, BATCH, ITERS = 257, 32, 6, 64, 3
ENV = "MountainCarContinuous-v0"
KINDS = {"plain": {}, "param_noise": dict(param_noise_stddev=0.2), "normalize": dict(normalize_observations=True)}
RING = ("s", "a", "r", "t", "s2")
ENV_STATE = ("s0", "s1", "steps", "ep_ret", "ou_x", "stats")


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


_RUNS = {}


def run(ssc, overlap, kind, stats_every):
    """one loop per variant, computed once and shared by the tests below"""
    key = (overlap, kind, stats_every)
    if key not in _RUNS:
        from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
        agent = DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=BATCH, num_train_iterations=ITERS, actor_h1=64,
                                     actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7, **KINDS[kind])
        env = ssc.VecEnv(ENV, N_ENVS, seed=5, max_episode_steps=60)
        kw = {} if stats_every is None else dict(stats_every=stats_every)
        summary, losses, replay = ssc.rl_train_vec_ddpg(env, agent, CHUNKS, chunk_steps=K, train_iters=ITERS, seed=3,
                                                        overlap=overlap, replay_capacity=1 << 16, drain_every=2, **kw)
        torch.cuda.synchronize()
        _RUNS[key] = dict(agent=agent, env=env, summary=summary, losses=losses, replay=replay)
    return _RUNS[key]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("overlap", [False, True])
def test_results_are_bit_identical_with_and_without_the_log(ssc, overlap, kind):
    base = run(ssc, overlap, kind, None)
    assert not hasattr(base["summary"], "agent_stats")
    assert len(base["losses"]) == CHUNKS and len(base["summary"]) > 0
    for k in (1, 4):
        other = run(ssc, overlap, kind, k)
        names = ["actor_flat", "critic_flat", "target_actor_flat", "target_critic_flat", "d_epsilon"]
        if kind == "param_noise":
            names += ["perturbed_actor_flat", "d_param_noise_stddev"]
        for name in names:
            assert np.array_equal(bits(getattr(base["agent"], name)), bits(getattr(other["agent"], name))), (k, name)
        if kind == "normalize":
            assert np.array_equal(bits(base["agent"].obs_rms.block), bits(other["agent"].obs_rms.block)), k
        assert base["agent"].decaying_ou_action_noise.epsilon == other["agent"].decaying_ou_action_noise.epsilon
        assert len(base["losses"]) == len(other["losses"])
        for la, lb in zip(base["losses"], other["losses"]):
            assert np.array_equal(bits(la), bits(lb)), k
        assert len(base["replay"]) == len(other["replay"]) and base["replay"]._batches_drawn == other["replay"]._batches_drawn
        for col in RING:
            assert np.array_equal(bits(getattr(base["replay"], col)), bits(getattr(other["replay"], col))), (k, col)
        for col in ENV_STATE:
            assert np.array_equal(bits(getattr(base["env"], col)), bits(getattr(other["env"], col))), (k, col)
        # (the episode ring hands out its slots atomically: the records are the same, their order inside a drain is not)
        assert sorted(base["summary"].episodes) == sorted(other["summary"].episodes)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("overlap", [False, True])
def test_log_shape_rows_and_last_row(ssc, overlap, kind):
    from smartstartcontinuous_amd import _ffi
    every = run(ssc, overlap, kind, 1)
    names = every["agent"].STATS_NAMES
    stats, chunks = every["summary"].agent_stats, every["summary"].agent_stats_chunks
    assert list(stats) == list(names) and len(names) == _ffi.SSC_DDPG_N_STATS
    assert chunks == list(range(CHUNKS)) and all(v.shape == (CHUNKS,) and v.dtype == np.float64 for v in stats.values())
    # the first chunk already holds 257 * 32 >= 64 records: every row is written
    assert np.all(np.isfinite(stats["reference_Q_mean"])) and np.all(stats["reference_action_std"] >= 0)
    applies = dict(obs_rms_mean=kind == "normalize", obs_rms_std=kind == "normalize",
                   reference_perturbed_action_mean=kind == "param_noise", reference_perturbed_action_std=kind == "param_noise",
                   param_noise_stddev=kind == "param_noise")
    for name in names:
        assert np.all(np.isfinite(stats[name])) if applies.get(name, True) else np.all(np.isnan(stats[name])), name
    # one sample for the whole run, and the learner moves Q on it
    assert len(set(stats["reference_Q_mean"].tolist())) > 1
    # the last row is what the agent reports after the loop, on the same sample: bit for bit
    after = every["agent"].get_stats_device().cpu().numpy()
    last = np.array([stats[name][-1] for name in names])
    assert np.array_equal(after.view(np.uint64), last.view(np.uint64))
    # k = 4 over 6 chunks: two rows, chunk 3 logged, the second row's chunk (7) is never reached and stays NaN
    sparse = run(ssc, overlap, kind, 4)
    s4 = sparse["summary"].agent_stats
    assert sparse["summary"].agent_stats_chunks == [3, 7] and all(v.shape == (2,) for v in s4.values())
    assert np.isfinite(s4["reference_Q_mean"][0]) and all(np.isnan(v[1]) for v in s4.values())


def test_rows_stay_nan_until_the_ring_holds_a_batch(ssc):
    """3 envs x 8 steps = 24 records per chunk: the ring reaches 64 records with chunk 2, the learner starts there too"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    agent = DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=BATCH, num_train_iterations=ITERS, actor_h1=64, actor_h2=32,
                                 critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7)
    env = ssc.VecEnv(ENV, 3, seed=5)
    summary, losses, replay = ssc.rl_train_vec_ddpg(env, agent, 4, chunk_steps=8, train_iters=ITERS, seed=3, replay_capacity=1 << 10,
                                                    stats_every=1)
    q = summary.agent_stats["reference_Q_mean"]
    assert q.shape == (4,) and np.all(np.isnan(q[:2])) and np.all(np.isfinite(q[2:])) and len(losses) == 2
    assert agent.stats_sample[0].shape == (BATCH, 2)


@pytest.mark.parametrize("overlap", [False, True])
def test_perturbed_action_stats_are_those_of_the_next_acting_copy(ssc, overlap):
    """With parameter noise the last row's reference_perturbed_action_* is the oracle's actor on ``perturbed_actor_flat`` as
    the loop leaves it -- the copy chunk CHUNKS would act with -- within the fp32 actor tolerance (1e-5)."""
    r = run(ssc, overlap, "param_noise", 1)
    agent, stats = r["agent"], r["summary"].agent_stats
    w = {k: v.cpu().numpy() for k, v in agent.perturbed_weights.items()}
    obs = agent.stats_sample[0].cpu().numpy().astype(np.float64)
    a = O.actor_forward(obs, *(w[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")), last_layer_tanh=True, obs_clip=5.0)
    assert abs(stats["reference_perturbed_action_mean"][-1] - a.mean()) <= 1e-5
    assert abs(stats["reference_perturbed_action_std"][-1] - a.std()) <= 1e-5
    plain = {k: v.cpu().numpy() for k, v in agent.weights.items()}
    b = O.actor_forward(obs, *(plain[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")), last_layer_tanh=True, obs_clip=5.0)
    assert abs(stats["reference_action_mean"][-1] - b.mean()) <= 1e-5
    assert abs(a.mean() - b.mean()) > 1e-4         # the perturbed copy is not the plain actor: the two slots can be told apart
    assert stats["param_noise_stddev"][-1] == float(agent.d_param_noise_stddev.item())
