"""``smartstart.select_plans_many`` / ``VecSmartStartPopulation.refresh_plans`` /
``rl_train_vec_smartstart_population(grouped_selection=True)``.

Set-up (tests/test_gpu_smartstart_population.py's): MountainCar, max_episode_steps 17, three pairs x 16 envs, chunks of 8
steps, n_plans (1, 3, 1), a replay ring of 512 records (it wraps in the fifth chunk) and kde_max_states = 100 (the KDE data set
is strided from the first chunk on).  Pair 0 normalises its observations, pair 1 carries parameter noise.

* ``select_plans_many`` against the per-pair ``select_plans`` fed the grouped path's own whitening and norm (the bandwidth is
  the one stage whose summation order differs): the same chosen indices, the same plans, the same ``_queries``.
* The loop with ``grouped_selection=True`` on the three pairs against three single-pair populations run the same way on
  ``VecEnv(16, env_id0 + env0_p)``: Summary, losses, ring arrays, agent parameters, eta, epsilon, selections -- bit for bit.
* The default is untouched: without the keyword, and with ``grouped_selection=False``, ``select_plans_many`` is never called
  and both runs agree bit for bit."""
import numpy as np
import pytest

from tests.test_gpu_navigator import make_mlp, make_norm
from tests.test_gpu_smartstart_population import ID0, NAV

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAME, COUNTS, ETAS, PLANS, SEEDS = "MountainCarContinuous-v0", [16, 16, 16], [0.7, 1.0, 0.5], [1, 3, 1], [5, 6, 7]
LOOP = dict(chunk_steps=8, train_iters=3, replay_capacity=512, ring_capacity=4096)


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _setup(ssc, only=None, seed=9, max_steps=17):
    """the population of three pairs, or pair ``only`` as a population of one on its own VecEnv; all objects built afresh"""
    from smartstartcontinuous_amd import navigator as nav
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    agents, models = [], []
    for p in range(3):
        extra = [dict(normalize_observations=True), dict(param_noise_stddev=0.1), dict()][p]
        agents.append(DDPG_Baselines_agent(ssc.make(NAME), None, batch_size=64, num_train_iterations=3, actor_h1=64, actor_h2=32,
                                           critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=21 + p, ou_mu=0.4,
                                           ou_sigma=0.3 + 0.2 * p, ou_epsilon=0.9, ou_epsilon_decay_factor=0.5, precision="f32", **extra))
        rng = np.random.default_rng(200 + p)
        Ws, bs = make_mlp(rng, (3, 32, 2))
        models.append(nav.DynamicsModel(Ws, bs, make_norm(rng, 2, 1), state_dim=2, act_dim=1, precision="f32"))
    kw = dict(n_ss=50, eta_decay_factor=0.9, chunk_steps=8, seed=seed + 1, w_max=max_steps + 1, kde_max_states=100, **NAV)
    sel = range(3) if only is None else [only]
    env0 = 0 if only is None else sum(COUNTS[:only])
    env = ssc.VecEnv(NAME, sum(COUNTS[p] for p in sel), seed=seed, max_episode_steps=max_steps, env_id0=ID0 + env0)
    env.reset()
    pop = ssc.VecSmartStartPopulation(env, [agents[p] for p in sel], [models[p] for p in sel], [COUNTS[p] for p in sel],
                                      eta=[ETAS[p] for p in sel], n_plans=[PLANS[p] for p in sel], **kw)
    return env, pop, [agents[p] for p in sel]


def _arrays(agent):
    from smartstartcontinuous_amd.agents import DDPGPopulation
    return DDPGPopulation._arrays(agent)


def _assert_same_run(got, agents_g, pair_g, want, agent_w, pair_w, what):
    (g_sum, g_losses, g_replay), (summary, losses, replay) = got, want
    assert len(summary.episodes) > 0 and g_sum.episodes == summary.episodes, what
    assert len(losses) > 0 and len(g_losses) == len(losses) and all(torch.equal(a, b) for a, b in zip(g_losses, losses)), what
    assert g_replay.count == replay.count and g_replay._queries == replay._queries > 0, what
    for name in ("s", "a", "r", "t", "s2", "ep_steps"):
        assert torch.equal(getattr(g_replay, name), getattr(replay, name)), (what, name)
    for k, (x, y) in enumerate(zip(_arrays(agents_g), _arrays(agent_w))):
        assert torch.equal(x, y), (what, "agent array", k)
    if agent_w.obs_rms is not None:
        assert torch.equal(agents_g.obs_rms.block, agent_w.obs_rms.block), what
    if agent_w.param_noise is not None:
        assert torch.equal(agents_g.perturbed_actor_flat, agent_w.perturbed_actor_flat), what
    assert pair_g.eta == pair_w.eta and pair_g.selections == pair_w.selections > 0, what
    assert agents_g.decaying_ou_action_noise.epsilon == agent_w.decaying_ou_action_noise.epsilon, what
    assert (pair_g.last_chosen is None) == (pair_w.last_chosen is None)
    if pair_w.last_chosen is not None:
        assert torch.equal(pair_g.last_chosen, pair_w.last_chosen), what
    assert np.array_equal(np.asarray(pair_g.last_radii), np.asarray(pair_w.last_radii)), what


def test_grouped_loop_equals_each_pair_as_a_population_of_one(ssc, monkeypatch):
    from smartstartcontinuous_amd import smartstart as SS
    monkeypatch.setattr(SS, "SMARTSTART_POPULATION_SELECTION_MIN_GROUP", 1)       # a population of one selects grouped, too
    calls = []
    real = SS.select_plans_many
    monkeypatch.setattr(SS, "select_plans_many", lambda pairs, replays: calls.append(len(pairs)) or real(pairs, replays))
    env, pop, agents = _setup(ssc)
    got = ssc.rl_train_vec_smartstart_population(env, pop, 6, seed=SEEDS, grouped_selection=True, **LOOP)
    torch.cuda.synchronize()
    assert calls == [3] * 6 and got[0][2].count > got[0][2].capacity              # the grouped path ran; the rings wrapped
    assert [pr.last_chosen.numel() for pr in pop.pairs] == PLANS
    for p in range(3):
        e, own, (agent,) = _setup(ssc, only=p)
        want = ssc.rl_train_vec_smartstart_population(e, own, 6, seed=[SEEDS[p]], grouped_selection=True, **LOOP)
        torch.cuda.synchronize()
        _assert_same_run(got[p], agents[p], pop.pairs[p], want[0], agent, own.pairs[0], "pair %d" % p)
    assert calls == [3] * 6 + [1] * 18


def test_select_plans_many_against_select_plans_on_the_same_bandwidth(ssc, monkeypatch):
    from smartstartcontinuous_amd import smartstart as SS
    env, pop, agents = _setup(ssc)
    res = ssc.rl_train_vec_smartstart_population(env, pop, 5, seed=SEEDS, **LOOP)
    replays = [r[2] for r in res]
    torch.cuda.synchronize()
    q0 = [r._queries for r in replays]
    radii0 = [None if pr.last_radii is None else np.array(pr.last_radii) for pr in pop.pairs]
    plans = SS.select_plans_many(pop.pairs, replays)
    assert [r._queries for r in replays] == [q + 1 for q in q0]
    chosen = [pr.last_chosen.clone() for pr in pop.pairs]
    buf = pop.pairs[0]._select_many
    wh, norm = buf.wh.cpu().numpy().reshape(3, 2, 2), buf.norm.cpu().numpy()
    for p, pr in enumerate(pop.pairs):
        replays[p]._queries = q0[p]
        assert (radii0[p] is None and pr.last_radii is None) or np.array_equal(radii0[p], pr.last_radii)   # select does not publish
        seen = []

        def grouped_bandwidth(data, p=p, seen=seen):
            seen.append(data.shape[0])
            return wh[p].copy(), float(norm[p])
        monkeypatch.setattr(SS, "kde_scott_bandwidth", grouped_bandwidth)
        want = pr.select_plans(replays[p])
        assert seen == [-(-(len(replays[p]) + 1) // -(-(len(replays[p]) + 1) // 100))] and seen[0] <= 100     # the strided data set
        assert replays[p]._queries == q0[p] + 1
        assert torch.equal(pr.last_chosen.reshape(-1), chosen[p]) and chosen[p].numel() == PLANS[p]
        assert len(plans[p]) == len(want) == PLANS[p]
        for a, b in zip(plans[p], want):
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    # an empty ring, and a pair with n_ss = 0, give None as the per-pair call does -- and nothing of them moves
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    empty = DeviceReplayBuffer(512, 2, 1, env.device, seed=3, track_episodes=True, n_envs=16, max_path_len=18)
    pop.pairs[2].n_ss = 0
    q = replays[2]._queries
    out = SS.select_plans_many(pop.pairs, [replays[0], empty, replays[2]])
    assert out[0] is not None and out[1] is None and out[2] is None and empty._queries == 0 and replays[2]._queries == q
    assert pop.pairs[1].select_plans(empty) is None and pop.pairs[2].select_plans(replays[2]) is None


def test_the_default_loop_never_selects_grouped(ssc, monkeypatch):
    from smartstartcontinuous_amd import smartstart as SS

    def refuse(*a, **k):
        raise AssertionError("the default population loop called select_plans_many")
    monkeypatch.setattr(SS, "select_plans_many", refuse)
    runs = []
    for kw in (dict(), dict(grouped_selection=False)):
        env, pop, agents = _setup(ssc)
        runs.append((ssc.rl_train_vec_smartstart_population(env, pop, 4, seed=SEEDS, **LOOP, **kw), agents, pop))
        torch.cuda.synchronize()
    (a, agents_a, pop_a), (b, agents_b, pop_b) = runs
    for p in range(3):
        _assert_same_run(a[p], agents_a[p], pop_a.pairs[p], b[p], agents_b[p], pop_b.pairs[p], "pair %d" % p)
