"""``rl_train_vec_ddpg_population`` with parameter-space noise: a noisy pair is DEFINED as its own
``rl_train_vec_ddpg(..., param_noise_cycle=True)`` run, so every comparison is bitwise; the population loop takes the same
keyword, and without it a noisy agent keeps raising.  3 pairs -- two noisy agents with
different stddev and seed, one plain -- on MountainCar with 16 envs, 8 chunks of 4 steps of which the last one is stored:
the rings pass ``batch_size`` 64 with chunk 3 (16 records per chunk), so the perturb-only interval (in front of chunk 0 and
behind chunks 0 .. 2) and the adapting one (behind chunks 3 .. 7) both run, and the learner starts with chunk 3."""
import numpy as np
import pytest

from tests.test_gpu_ddpg_many import assert_agents_equal, make_agent
from tests.test_gpu_ddpg_population_monitor import assert_runs_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MC = "MountainCarContinuous-v0"
P = 3
STDDEV = (0.2, None, 0.05)
KW = dict(num_chunks=8, chunk_steps=4, train_iters=3, replay_capacity=4096, replay_last_steps=1)


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def pairs(ssc):
    envs = [ssc.VecEnv(MC, 16, seed=20 + p, max_episode_steps=20) for p in range(P)]
    for e in envs:
        e.reset()
    # desired 0.02 / 0.5: the first agent's stddev is divided, the third's multiplied, so both branches of the rule run
    agents = [make_agent(ssc, p, reward_scale=0.5 + 0.25 * p, param_noise_stddev=sd,
                         param_noise_desired_action_stddev=None if sd is None else (0.02 if p == 0 else 0.5))
              for p, sd in enumerate(STDDEV)]
    return envs, agents


def noise_state(a):
    return (a.perturbed_actor_flat, a.d_param_noise_stddev, a.d_param_noise_distance)


def assert_noise_equal(agents, twins):
    for p, (a, b) in enumerate(zip(agents, twins)):
        assert (a.param_noise is None) == (b.param_noise is None) == (STDDEV[p] is None)
        if a.param_noise is None:
            continue
        for x, y in zip(noise_state(a), noise_state(b)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), p
        # 1 at construction, 1 in front of chunk 0, 1 behind each of chunks 0 .. 2, 2 behind each of chunks 3 .. 7
        assert a.param_noise_generation == b.param_noise_generation == 15
        assert a.perturbed_generation == b.perturbed_generation == 14


@pytest.mark.parametrize("monitored", [False, True])
def test_noisy_population_loop_is_bitwise_the_single_loops(ssc, monitored):
    from smartstartcontinuous_amd import agents as agents_mod
    envs, agents = pairs(ssc)
    ways = []
    inner = agents_mod.DDPGPopulation

    class Spy(inner):
        def param_noise_cycle(self, *a, **k):
            super().param_noise_cycle(*a, **k)
            ways.append(self.pn_fused)
    agents_mod.DDPGPopulation = Spy
    try:
        monitor = ssc.PopulationMonitor(stats_every=2) if monitored else None
        got = ssc.rl_train_vec_ddpg_population(envs, agents, seed=[3, 4, 5], monitor=monitor, param_noise_cycle=True, **KW)
    finally:
        agents_mod.DDPGPopulation = inner
    assert ways == [True] * 9                                    # in front of chunk 0 and behind every chunk, one launch each
    t_envs, twins = pairs(ssc)
    fields = ("agent_stats", "agent_stats_chunks") if monitored else ()
    for p in range(P):
        want = ssc.rl_train_vec_ddpg(t_envs[p], twins[p], seed=3 + p, param_noise_cycle=True,
                                     stats_every=2 if monitored else None, **KW)
        assert_runs_equal(got[p], want, fields)
        assert len(got[p][1]) == 5                               # the learner ran behind chunks 3 .. 7
        # one adaption batch per learner chunk beside its 3 training batches
        assert got[p][2]._batches_drawn == (20 if STDDEV[p] is not None else 15)                  # (the diagnostics sample has a key of its own)
        assert agents[p].decaying_ou_action_noise.epsilon == twins[p].decaying_ou_action_noise.epsilon
        assert torch.equal(envs[p].s0, t_envs[p].s0) and envs[p].t == t_envs[p].t
        if monitored:
            s = got[p][0].agent_stats
            assert got[p][0].agent_stats_chunks == [1, 3, 5, 7]
            assert np.isnan(s["reference_Q_mean"][0]) and np.all(np.isfinite(s["reference_Q_mean"][1:]))
            noisy = STDDEV[p] is not None
            assert np.all(np.isfinite(s["param_noise_stddev"][1:])) == noisy
            assert np.all(np.isfinite(s["reference_perturbed_action_std"][1:])) == noisy
    assert_agents_equal(agents, twins)
    assert_noise_equal(agents, twins)
    # both branches of the adapt rule were taken: five adaptions each
    f32 = np.float32
    down, up = f32(0.2), f32(0.05)
    for _ in range(5):
        down, up = down / f32(1.01), up * f32(1.01)
    assert agents[0].d_param_noise_stddev.item() == down and agents[2].d_param_noise_stddev.item() == up


def test_overlap_still_raises(ssc):
    envs, agents = pairs(ssc)
    with pytest.raises(NotImplementedError, match="overlap"):
        ssc.rl_train_vec_ddpg_population(envs, agents, 1, chunk_steps=4, overlap=True, param_noise_cycle=True)


def test_noisy_population_is_opt_in(ssc):
    """without ``param_noise_cycle=True`` a noisy population raises as it always did and nothing has moved; a population of
    plain agents takes the keyword and computes what it computes without it"""
    envs, agents = pairs(ssc)
    before = [e.t for e in envs]
    with pytest.raises(NotImplementedError, match="param_noise_cycle=True"):
        ssc.rl_train_vec_ddpg_population(envs, agents, 1, chunk_steps=4)
    assert [e.t for e in envs] == before and agents[0].param_noise_generation == 1
    kw = dict(KW, num_chunks=5)
    runs = []
    for flag in (False, True):
        envs, agents = pairs(ssc)
        runs.append((ssc.rl_train_vec_ddpg_population(envs[1:2], agents[1:2], seed=4, param_noise_cycle=flag, **kw), agents[1:2]))
    assert_runs_equal(runs[0][0][0], runs[1][0][0])
    assert_agents_equal(runs[0][1], runs[1][1])


def test_default_single_loop_keeps_the_composed_sequence(ssc):
    """``rl_train_vec_ddpg`` with default arguments on a noisy agent still runs the composed sequence
    (``adapt_param_noise`` + a perturbation) behind every chunk: the loop's phases are run here by hand on a twin, call by
    call, and the whole run -- replay contents, losses, parameters, both copies, stddev, generations -- is equal."""
    envs, agents = pairs(ssc)
    env, agent = envs[0], agents[0]
    got = ssc.rl_train_vec_ddpg(env, agent, seed=3, **KW)

    t_envs, twins = pairs(ssc)
    t_env, twin = t_envs[0], twins[0]
    from smartstartcontinuous_amd.rl_train import epsilon_schedule, update_obs_rms, vec_loop_buffers
    ring, chunk, replay = vec_loop_buffers(t_env, KW["chunk_steps"], KW["replay_capacity"], 1 << 20, 3, False)
    schedule = epsilon_schedule(twin, t_env.n, t_env.device)
    finished, finished0 = t_env.stats[3:4], float(t_env.stats[3].item())
    pd = t_env.policy_desc(twin.as_policy(device_epsilon=True, perturbed=True))
    twin.perturb_policy()
    losses = []
    for i in range(KW["num_chunks"]):
        out = t_env.rollout(KW["chunk_steps"], out=chunk, ring=ring, policy_desc=pd)
        schedule.update(finished, finished0)
        replay.append_chunk(out, reward_scale=twin.reward_scale, last_steps=KW["replay_last_steps"])
        update_obs_rms(twin, out, KW["replay_last_steps"])
        l = twin.train_from(replay, KW["train_iters"])
        if l is not None:
            losses.append(l)
        if len(replay) >= twin.batch_size:                       # the composed sequence, call by call
            obs0 = replay.s.index_select(0, replay.sample_indices(1, twin.batch_size)[0].long())
            twin.adapt_param_noise(obs0)
        twin.perturb_policy()
    torch.cuda.synchronize()
    assert len(got[1]) == len(losses) == 5 and all(torch.equal(x, y) for x, y in zip(got[1], losses))
    assert got[2].count == replay.count and got[2]._batches_drawn == replay._batches_drawn == 20
    assert torch.equal(got[2].s, replay.s) and torch.equal(got[2].r, replay.r)
    assert_agents_equal([agent], [twin])
    for x, y in zip(noise_state(agent), noise_state(twin)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(agent.adaptive_actor_flat.view(torch.int32), twin.adaptive_actor_flat.view(torch.int32))   # the cycle never writes it
    assert agent.param_noise_generation == twin.param_noise_generation == 15
    # ... and the cycle form differs only in what the header says: the same stddev and acting copy wherever both forms agree on
    # the side of `desired` the distance lies (here it is far away from it: 0.02 against the action distance of a 0.2 stddev)
    c_envs, cyc = pairs(ssc)
    ssc.rl_train_vec_ddpg(c_envs[0], cyc[0], seed=3, param_noise_cycle=True, **KW)
    assert torch.equal(cyc[0].d_param_noise_stddev, agent.d_param_noise_stddev)
    assert torch.equal(cyc[0].perturbed_actor_flat.view(torch.int32), agent.perturbed_actor_flat.view(torch.int32))
