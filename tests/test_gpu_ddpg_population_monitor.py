"""``rl_train_vec_ddpg_population(..., monitor=PopulationMonitor(...))``: diagnostics and evaluation of all pairs behind the
learner launch, logged on the device.  Every pair's logs are DEFINED as what its own ``rl_train_vec_ddpg(..., eval_env=,
eval_every=, eval_steps=, stats_every=)`` run gives, and the monitor changes nothing else, so every comparison is bitwise."""
import numpy as np
import pytest

from tests.test_gpu_ddpg_many import assert_agents_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MC = "MountainCarContinuous-v0"
P = 3
KW = dict(num_chunks=4, chunk_steps=8, train_iters=3, replay_capacity=4096)


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def pairs(ssc, late):
    """3 pairs x 32 training envs and 3 x 20 eval envs.  ``late``: the loop stores the last step of a chunk only (32 records
    per chunk) and the third agent draws batches of 128 -- it has no sample at the first diagnostics row (64 records) and one
    at the second (128); the second agent normalises its observations.  Otherwise every ring holds a batch after chunk 0
    and the population trains in one launch."""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    envs = [ssc.VecEnv(MC, 32, seed=20 + p, max_episode_steps=20) for p in range(P)]
    evals = [ssc.VecEnv(MC, 20, seed=60 + p, env_id0=500 * p, max_episode_steps=6) for p in range(P)]
    for e in envs:
        e.reset()
    agents = [DDPG_Baselines_agent(ssc.make(MC), None, batch_size=128 if late and p == 2 else 64, actor_h1=64, actor_h2=32, critic_h1=64,
                                   critic_h2=32, lastLayerTanh=True, seed=40 + p, actor_lr=1e-4 * (1 + p), critic_lr=1e-3 / (1 + p),
                                   gamma=0.99 - 0.01 * p, tau=0.001 * (1 + p), reward_scale=0.5 + 0.25 * p,
                                   normalize_observations=late and p == 1)
              for p in range(P)]
    return envs, evals, agents


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_runs_equal(got, want, fields=()):
    (g_summary, g_losses, g_replay), (summary, losses, replay) = got, want
    assert len(g_losses) == len(losses) and all(torch.equal(x, y) for x, y in zip(g_losses, losses))
    assert g_summary.episodes == summary.episodes and g_summary.dropped_episode_records == summary.dropped_episode_records == 0
    assert g_replay.count == replay.count and g_replay._batches_drawn == replay._batches_drawn
    assert torch.equal(g_replay.s, replay.s) and torch.equal(g_replay.r, replay.r)
    for name in fields:
        a, b = getattr(g_summary, name), getattr(summary, name)
        if isinstance(b, dict):
            assert list(a) == list(b) and all(np.array_equal(bits(a[k]), bits(b[k])) for k in b), name
        else:
            assert a == b, name


@pytest.mark.parametrize("late", [False, True])
def test_monitored_population_loop_is_bitwise_the_single_loops(ssc, late):
    from smartstartcontinuous_amd import agents as agents_mod
    kw = dict(KW, replay_last_steps=1) if late else KW
    envs, evals, agents = pairs(ssc, late)
    ways = []
    inner = agents_mod.DDPGPopulation

    class Spy(inner):
        def evaluate_device(self, *a, **k):
            out = super().evaluate_device(*a, **k)
            ways.append(("eval", self.eval_fused))
            return out

        def get_stats_device(self, *a, **k):
            out = super().get_stats_device(*a, **k)
            ways.append(("stats", self.stats_fused))
            return out
    agents_mod.DDPGPopulation = Spy
    try:
        monitor = ssc.PopulationMonitor(eval_envs=evals, eval_every=2, eval_steps=9, stats_every=2)
        got = ssc.rl_train_vec_ddpg_population(envs, agents, seed=[3, 4, 5], monitor=monitor, **kw)
    finally:
        agents_mod.DDPGPopulation = inner
    assert ways == [("stats", True), ("eval", True)] * 2         # one call of each behind chunks 1 and 3, in one launch each
    fields = ("agent_stats", "agent_stats_chunks", "eval_stats", "eval_chunks")
    t_envs, t_evals, twins = pairs(ssc, late)
    for p in range(P):
        want = ssc.rl_train_vec_ddpg(t_envs[p], twins[p], seed=3 + p, eval_env=t_evals[p], eval_every=2, eval_steps=9, stats_every=2, **kw)
        assert_runs_equal(got[p], want, fields)
        s = got[p][0]
        assert s.agent_stats_chunks == s.eval_chunks == [1, 3] and s.eval_stats["eval/steps"].tolist() == [180.0, 180.0]
        assert np.all(s.eval_stats["eval/episodes"] >= 20) and np.all(np.isfinite(s.eval_stats["eval/Q"]))
        first = np.isnan(s.agent_stats["reference_Q_mean"][0])
        assert first == (late and p == 2) and np.isfinite(s.agent_stats["reference_Q_mean"][1])
        assert np.all(np.isfinite(s.agent_stats["obs_rms_mean"])) == (late and p == 1)
        assert evals[p].t == t_evals[p].t == 18 and torch.equal(evals[p].s0, t_evals[p].s0)
        if twins[p].obs_rms is not None:
            assert torch.equal(agents[p].obs_rms.block, twins[p].obs_rms.block)
        assert agents[p].decaying_ou_action_noise.epsilon == twins[p].decaying_ou_action_noise.epsilon
    assert_agents_equal(agents, twins)
    # the monitor changes nothing else: the same population loop without it
    b_envs, _, bare = pairs(ssc, late)
    plain = ssc.rl_train_vec_ddpg_population(b_envs, bare, seed=[3, 4, 5], **kw)
    for p in range(P):
        assert_runs_equal(got[p], plain[p])
        assert not hasattr(plain[p][0], "eval_stats") and not hasattr(plain[p][0], "agent_stats")
    assert_agents_equal(agents, bare)


def test_monitor_arguments(ssc):
    envs, evals, agents = pairs(ssc, False)
    run = lambda **kw: ssc.rl_train_vec_ddpg_population(envs, agents, 1, chunk_steps=4, monitor=ssc.PopulationMonitor(**kw))
    pend = ssc.VecEnv("Pendulum-v0", 20, seed=1)
    for kw in (dict(eval_envs=evals), dict(eval_every=2), dict(eval_steps=5), dict(eval_envs=evals[:2], eval_every=1),
               dict(eval_envs=[envs[0]] + evals[1:], eval_every=1),                 # a training env
               dict(eval_envs=[evals[0], envs[2], evals[2]], eval_every=1),         # ... another pair's
               dict(eval_envs=[evals[0], evals[0], evals[2]], eval_every=1),        # one eval env for two pairs
               dict(eval_envs=evals[:2] + [pend], eval_every=1),                    # another kind
               dict(eval_envs=evals, eval_every=0), dict(eval_envs=evals, eval_every=1.5), dict(eval_envs=evals, eval_every=True),
               dict(eval_envs=evals, eval_every=1, eval_steps=0), dict(stats_every=0), dict(stats_every=1.5)):
        with pytest.raises(ValueError):
            run(**kw)
    # the single loop's keywords keep raising and point to the monitor
    for kw in (dict(stats_every=2), dict(eval_env=evals[0], eval_every=1)):
        with pytest.raises(NotImplementedError, match="PopulationMonitor"):
            ssc.rl_train_vec_ddpg_population(envs, agents, 1, chunk_steps=4, **kw)
    # the default eval_steps: the eval envs' episode limit
    got = run(eval_envs=evals, eval_every=1)
    assert [g[0].eval_stats["eval/steps"].tolist() for g in got] == [[120.0]] * P
