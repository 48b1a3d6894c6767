"""``VecSmartStartPopulation`` / ``ssc_smartstart_rollout_step_many`` / ``ssc_actor_forward_many`` inside the step: every
pair's slice of the population equals, BIT FOR BIT, the pair's own ``VecSmartStart`` on ``VecEnv(n_p, env_id0 + env0_p)`` --
env and OU state, mode, waypoint bookkeeping, plan_of - slot0, the transition log, the mode log -- after every step of an
eager run and after a graph run.  Episode-ring records are equal as sets per pair; statistics columns 1-3 exactly, column 0
(a sum of float rewards in f64 atomics, order-free) within 1e-12 relative.  Simulation / candidate scratch of problems that
are not navigating is not compared.

Case A (MountainCar): pairs of 40, 256 and 300 envs (a partial block, exactly one, more than one), f32 64-32 actors and
1x32 fp32 models with different weights and statistics, eta (0, 0.7, 1.0), epsilon (0, 0.8, 0.3), distinct OU sigma.
Case B (Pendulum): bf16 64-32, bf16 200-100 with obs_rms, generic LayerNorm f32 with 20 envs, a second bf16 64-32 with
parameter noise; two 1x32 fp32 and two 1x500 bf16 models."""
import types

import numpy as np
import pytest

from tests.test_gpu_navigator import make_mlp, make_norm
from tests.test_gpu_smartstart_vec import _pend_plans, _plans

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ID0 = 40
NAV = dict(num_control_samples=16, horizon=3, steps_before_giving_up_on_waypoint=2, final_steps=4, log_modes=True)


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _agents_models(ssc, case):
    from smartstartcontinuous_amd import navigator as nav
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    if case == "A":
        name, d, counts = "MountainCarContinuous-v0", 2, [40, 256, 300]
        spec = [dict(actor_h1=64, actor_h2=32, precision="f32", ou_sigma=s) for s in (0.6, 0.3, 0.45)]
        mspec = [((3, 32, 2), "f32")] * 3
    else:
        name, d, counts = "Pendulum-v1", 3, [64, 70, 20, 33]
        spec = [dict(actor_h1=64, actor_h2=32, precision="bf16_mfma", ou_sigma=0.5),
                dict(actor_h1=200, actor_h2=100, precision="bf16_mfma", ou_sigma=0.2, normalize_observations=True),
                dict(actor_h1=48, actor_h2=24, precision="f32", ou_sigma=0.35, layer_norm=True),
                dict(actor_h1=64, actor_h2=32, precision="bf16_mfma", ou_sigma=0.25, param_noise_stddev=0.1)]
        mspec = [((4, 32, 3), "f32"), ((4, 500, 3), "bf16_mfma"), ((4, 32, 3), "f32"), ((4, 500, 3), "bf16_mfma")]
    agents, models = [], []
    for p, (kw, (dims, prec)) in enumerate(zip(spec, mspec)):
        a = DDPG_Baselines_agent(ssc.make(name), None, critic_h1=64, critic_h2=32, lastLayerTanh=bool(p % 2 == 0), seed=11 + p,
                                 training=False, ou_mu=0.4, **kw)
        if getattr(a, "obs_rms", None) is not None:     # statistics that are not the initial block
            a.obs_rms.update_rows(np.random.default_rng(3).normal(0.2, 1.5, (50, d)).astype(np.float32))
        if getattr(a, "param_noise", None) is not None:
            a.perturb_policy()
        agents.append(a)
        rng = np.random.default_rng(100 + p)
        Ws, bs = make_mlp(rng, dims)
        models.append(nav.DynamicsModel(Ws, bs, make_norm(rng, d, 1), state_dim=d, act_dim=1, precision=prec))
    return name, d, counts, agents, models


def _build(ssc, case, seed=9, max_steps=17):
    """the population and every pair's own VecSmartStart, on the same agents, models and plans"""
    name, d, counts, agents, models = _agents_models(ssc, case)
    P = len(counts)
    etas = [0.0, 0.7, 1.0, 0.5][:P]
    eps = [0.0, 0.8, 0.3, 0.6][:P]
    for a, e in zip(agents, eps):
        a.decaying_ou_action_noise.epsilon = e
    env = ssc.VecEnv(name, sum(counts), seed=seed, max_episode_steps=max_steps, env_id0=ID0)
    env.reset()
    pop = ssc.VecSmartStartPopulation(env, agents, models, counts, eta=etas, n_plans=3, chunk_steps=40, seed=seed + 1,
                                      w_max=max(max_steps + 1, 16), **NAV)
    own, env0 = [], 0
    for p in range(P):
        e = ssc.VecEnv(name, counts[p], seed=seed, max_episode_steps=max_steps, env_id0=ID0 + env0)
        e.reset()
        own.append(ssc.VecSmartStart(e, agents[p], models[p], eta=etas[p], n_plans=3, chunk_steps=40, seed=seed + 1,
                                     w_max=max(max_steps + 1, 16), **NAV))
        env0 += counts[p]
    _publish(case, pop, own, seed + 3)
    return env, pop, own, counts


def _publish(case, pop, own, seed):
    for p, (pr, o) in enumerate(zip(pop.pairs, own)):
        rng = np.random.default_rng(seed + 17 * p)
        plans = _plans(rng, 3, near_reset=1) if case == "A" else _pend_plans(rng, 3)
        pr.pool.publish(plans)
        o.pool.publish(plans)
        assert pr.pool.triple == tuple(o.pool.pool.cpu().tolist())


def _rings(ssc, env, own, cap=4096):
    return ssc.EpisodeRing(cap, env.device), [ssc.EpisodeRing(cap, o.env.device) for o in own]


def _compare(pop, own, chunk=None, own_chunks=None, what=""):
    torch.cuda.synchronize()
    e, b = pop.env, pop.nav
    eq = lambda x, y, name, p: np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=f"{what} pair {p}: {name}")
    for p, (pr, o) in enumerate(zip(pop.pairs, own)):
        sl = slice(pr.env0, pr.env0 + pr.n)
        for name in ("s0", "s1", "steps", "ep_ret", "ou_x"):
            eq(getattr(e, name)[sl], getattr(o.env, name), name, p)
        eq(pop.mode[sl], o.mode, "mode", p)
        eq(pop.pool.cur_idx[sl], o.pool.cur_idx, "cur_idx", p)
        eq(b.actions_done[sl], o.nav.actions_done, "actions_done", p)
        eq(b.at_goal[sl], o.nav.at_goal, "at_goal", p)
        eq(pop.pool.plan_of[sl] - pr.pool.slot0, o.pool.plan_of, "plan_of - slot0", p)
        if chunk is not None:
            c = own_chunks[p]
            for name in ("obs", "act", "rew", "done", "obs2"):
                eq(getattr(chunk, name)[..., sl], getattr(c, name), "log " + name, p)
            eq(pop.mode_log[:, sl], o.mode_log, "mode log", p)
        st, so = pop.stats[p].cpu().numpy(), o.env.stats.cpu().numpy()
        assert (st[1:] == so[1:]).all(), (what, p, st, so)
        assert abs(st[0] - so[0]) <= 1e-12 * max(abs(so[0]), 1e-300), (what, p, st[0], so[0])


def _ring_sets(ring, own_rings, pop):
    (ids, lens, rets), dropped = ring.drain()
    assert dropped == 0
    for pr, r in zip(pop.pairs, own_rings):
        (i2, l2, r2), d2 = r.drain()
        mine = (ids >= pop.env.env_id0 + pr.env0) & (ids < pop.env.env_id0 + pr.env0 + pr.n)
        got = sorted(zip(ids[mine].tolist(), lens[mine].tolist(), rets[mine].view(np.int32).tolist()))
        want = sorted(zip(i2.tolist(), l2.tolist(), r2.view(np.int32).tolist()))
        assert d2 == 0 and got == want and (pr.eta == 0 or len(want) > 0)
    return len(ids)


@pytest.mark.parametrize("case", ["A", "B"])
def test_every_eager_step_equals_each_pairs_own_vec_smartstart(ssc, case):
    env, pop, own, counts = _build(ssc, case)
    d, K = env.obs_dim, 40
    ring, own_rings = _rings(ssc, env, own)
    c1 = ssc.TransitionChunk(d, 1, env.n, env.device)
    oc1 = [ssc.TransitionChunk(d, 1, n, env.device) for n in counts]
    navigated = np.zeros(len(counts), bool)
    for k in range(K):
        pop.rollout(1, c1, ring=ring, graph=False)
        for o, c, r in zip(own, oc1, own_rings):
            o.rollout(1, c, ring=r, graph=False)
        _compare(pop, own, c1, oc1, what=f"case {case} step {k}")
        navigated |= np.array([bool(pop.mode_log[0, pr.env0:pr.env0 + pr.n].any()) for pr in pop.pairs])
    assert _ring_sets(ring, own_rings, pop) > 0
    assert not navigated[0] and navigated[1:].all()          # eta 0 never navigates; the others do: both branches ran
    ways = [w[0] for w in pop._actor_plan]
    assert ways == (["many"] if case == "A" else ["many", "alone", "alone"]) or sorted(ways) == ["alone", "alone", "many"], ways


@pytest.mark.parametrize("case", ["A", "B"])
def test_graph_replay_and_table_rewrites_between_chunks(ssc, case):
    """One captured graph: chunk 1 equals the pairs' own graph runs; then eta, epsilon and the pool windows are rewritten on
    the host -- chunk 2 follows them WITHOUT a re-capture and still equals the pairs' own runs."""
    env, pop, own, counts = _build(ssc, case)
    d, K = env.obs_dim, 40
    ring, own_rings = _rings(ssc, env, own)
    chunk = ssc.TransitionChunk(d, K, env.n, env.device)
    ocs = [ssc.TransitionChunk(d, K, n, env.device) for n in counts]

    def run(what):
        # (the pairs' own runs first: they share the model objects, and a model's first call of its own allocates its
        # workspace, which is part of every graph key that covers the model)
        for o, c, r in zip(own, ocs, own_rings):
            o.rollout(K, c, ring=r, graph=True)
        pop.rollout(K, chunk, ring=ring, graph=True)
        _compare(pop, own, chunk, ocs, what=what)
        _ring_sets(ring, own_rings, pop)

    run(f"case {case} chunk 1")
    assert len(pop._graphs.graphs) == 1
    act1 = chunk.act.clone()
    new_eta, new_eps = [1.0, 0.0, 0.4, 0.9], [0.5, 0.1, 0.0, 0.2]
    for p, (pr, o) in enumerate(zip(pop.pairs, own)):
        pr.eta = o.eta = new_eta[p]
        pr.agent.decaying_ou_action_noise.epsilon = new_eps[p]
    _publish(case, pop, own, 1000)                           # new plans: the triples move round-robin inside each window
    assert all(pr.pool.triple[0] == 3 for pr in pop.pairs)
    run(f"case {case} chunk 2")
    assert len(pop._graphs.graphs) == 1                      # the same graph followed the rewritten table
    assert bool(pop.mode_log[:, :counts[0]].any())           # pair 0 (eta 0 -> 1) navigates now
    assert not torch.equal(act1, chunk.act)


def test_graph_key_follows_a_replaced_actor_tensor_and_ret_rms_is_refused(ssc):
    env, pop, own, counts = _build(ssc, "A")
    chunk = ssc.TransitionChunk(2, 4, env.n, env.device)
    pop.sync_actor_items()
    key0 = pop.graph_key(4, chunk, None)
    desc = pop.pairs[1].agent._desc
    old, fresh = desc.b3, torch.zeros(1, dtype=torch.float32, device=env.device)
    desc.b3 = fresh.data_ptr()
    pop.sync_actor_items()
    assert pop.graph_key(4, chunk, None) != key0
    desc.b3 = old
    pop.sync_actor_items()
    assert pop.graph_key(4, chunk, None) == key0
    with pytest.raises(NotImplementedError):
        ssc.VecSmartStartPopulation(env, [types.SimpleNamespace(ret_rms=object())] * 3, [None] * 3, counts)


def _loop_setup(ssc, own_pair=None, seed=9, max_steps=17):
    """2 pairs x 64 MountainCar envs with TRAINING agents (pair 0 normalises its observations, pair 1 carries parameter
    noise) -- the population, or pair ``own_pair`` alone on its own VecEnv; every object is built afresh from the same seeds"""
    from smartstartcontinuous_amd import navigator as nav
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent, DDPGPopulation
    name, counts, etas = "MountainCarContinuous-v0", [64, 64], [0.7, 1.0]
    agents, models = [], []
    for p in range(2):
        extra = dict(normalize_observations=True) if p == 0 else dict(param_noise_stddev=0.1)
        agents.append(DDPG_Baselines_agent(ssc.make(name), None, batch_size=64, num_train_iterations=3, actor_h1=64, actor_h2=32,
                                           critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=21 + p, ou_mu=0.4,
                                           ou_sigma=0.3 + 0.2 * p, ou_epsilon=0.9, ou_epsilon_decay_factor=0.5, precision="f32", **extra))
        rng = np.random.default_rng(200 + p)
        Ws, bs = make_mlp(rng, (3, 32, 2))
        models.append(nav.DynamicsModel(Ws, bs, make_norm(rng, 2, 1), state_dim=2, act_dim=1, precision="f32"))
    kw = dict(n_plans=2, n_ss=50, eta_decay_factor=0.9, chunk_steps=16, seed=seed + 1, w_max=max_steps + 1, **NAV)
    if own_pair is None:
        env = ssc.VecEnv(name, sum(counts), seed=seed, max_episode_steps=max_steps, env_id0=ID0)
        env.reset()
        return env, ssc.VecSmartStartPopulation(env, agents, models, counts, eta=etas, **kw), agents, DDPGPopulation._arrays
    p = own_pair
    env = ssc.VecEnv(name, counts[p], seed=seed, max_episode_steps=max_steps, env_id0=ID0 + sum(counts[:p]))
    env.reset()
    return env, ssc.VecSmartStart(env, agents[p], models[p], eta=etas[p], **kw), agents[p], DDPGPopulation._arrays


def test_population_loop_equals_each_pairs_own_loop(ssc):
    """rl_train_vec_smartstart_population: 2 pairs x 64 envs, 4 chunks of 16 steps, train_iters = 3 -- each pair's Summary,
    losses, replay ring contents, agent parameters and final eta / epsilon equal its own rl_train_vec_smartstart run bit for bit"""
    kw = dict(chunk_steps=16, train_iters=3, replay_capacity=1 << 13, ring_capacity=4096, seed=[5, 6])
    env, pop, agents, arrays = _loop_setup(ssc)
    got = ssc.rl_train_vec_smartstart_population(env, pop, 4, **kw)
    torch.cuda.synchronize()
    assert sum(pr.selections for pr in pop.pairs) > 0 and int(pop.mode_log.any()) == 1     # selections ran and envs navigated
    for p in range(2):
        e, smart, agent, _ = _loop_setup(ssc, own_pair=p)
        summary, losses, replay = ssc.rl_train_vec_smartstart(e, smart, 4, **dict(kw, seed=kw["seed"][p]))
        torch.cuda.synchronize()
        g_sum, g_losses, g_replay = got[p]
        assert len(summary.episodes) > 0 and g_sum.episodes == summary.episodes, p
        assert len(losses) > 0 and len(g_losses) == len(losses) and all(torch.equal(a, b) for a, b in zip(g_losses, losses)), p
        assert g_replay.count == replay.count and len(g_replay) == len(replay)
        for name in ("s", "a", "r", "t", "s2"):
            assert torch.equal(getattr(g_replay, name), getattr(replay, name)), (p, name)
        for k, (x, y) in enumerate(zip(arrays(agents[p]), arrays(agent))):
            assert torch.equal(x, y), (p, "agent array", k)
        if agent.obs_rms is not None:
            assert torch.equal(agents[p].obs_rms.block, agent.obs_rms.block)
        if agent.param_noise is not None:
            assert torch.equal(agents[p].perturbed_actor_flat, agent.perturbed_actor_flat)
        assert pop.pairs[p].eta == smart.eta and smart.eta < (0.7, 1.0)[p]                 # the decay ran
        assert agents[p].decaying_ou_action_noise.epsilon == agent.decaying_ou_action_noise.epsilon < 0.9
        assert pop.pairs[p].selections == smart.selections


def test_the_population_loop_refuses_overlapped_selection(ssc):
    env, pop, _agents, _ = _loop_setup(ssc)
    with pytest.raises(NotImplementedError):
        ssc.rl_train_vec_smartstart_population(env, pop, 1, chunk_steps=16, overlap_selection=True)
