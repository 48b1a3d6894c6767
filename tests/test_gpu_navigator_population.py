"""navigator.NavigatorPopulation: the navigators of several dynamics models in ONE VecEnv, stepped by one captured graph whose
forward simulation is one ssc_mpc_forward_sim_many launch.  Three models (1 x 32, 1 x 30, 1 x 64) with 5 MountainCar envs
each: the graph path, the eager path, both again with NAV_POPULATION_GROUPED = False (every model through its own call and a
strided copy) and three separate (VecEnv, NavigatorBatch) runs give every env the same bits -- transition log, waypoint
bookkeeping, env state.  The f64 chunk statistics sum over 15 envs in another order than over 3 x 5: only their integer
entries are compared."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import sim_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEPTHS, E, N, H, K = (32, 30, 64), 5, 16, 4, 6
COLS = ("obs", "act", "rew", "done", "obs2")


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


@pytest.fixture(scope="module")
def setting():
    rng = np.random.default_rng(31)
    nets = [SC.make_mlp(rng, (3, depth, 2)) + (SC.make_norm(rng, 2, 1),) for depth in DEPTHS]
    paths = [np.cumsum(rng.normal(scale=[0.02, 0.004], size=(12, 2)), axis=0) + [-0.5, 0.0] for _ in range(len(DEPTHS) * E)]
    plans = []
    for pth in paths:
        stds, means = O.path_deltas_stds_and_means_per_dim(pth)
        r = O.radii_calc(means, stds, 1, 1, 1) + 1e-3
        plans.append((pth, O.distances_left(pth, O.distance_func(r)), r))
    return nets, plans


def models_of(nav, nets):
    return [nav.DynamicsModel(Ws, bs, norm, state_dim=2, act_dim=1, precision="f32") for Ws, bs, norm in nets]


def problems_of(nav, plans):
    return nav.MpcProblemSet([p[0] for p in plans], [p[1] for p in plans], [p[2] for p in plans], [0] * len(plans))


def snapshot(env, ps, batch, chunks):
    torch.cuda.synchronize()
    return dict(log=[{k: getattr(ch, k).clone() for k in COLS} for ch in chunks], cur_idx=ps.cur_idx.clone(),
                actions_done=batch.actions_done.clone(), at_goal=batch.at_goal.clone(), s0=env.s0.clone(), s1=env.s1.clone(),
                steps=env.steps.clone(), ep_ret=env.ep_ret.clone(), stats=env.stats.cpu().numpy().copy(), t=env.t)


def run_population(nav, setting, graph):
    import smartstartcontinuous_amd as ssc
    nets, plans = setting
    env = ssc.VecEnv("MountainCarContinuous-v0", len(plans), seed=21, max_episode_steps=4)
    env.reset()
    ps = problems_of(nav, plans)
    batch = nav.NavigatorPopulation(models_of(nav, nets), ps, E, num_control_samples=N, horizon=H, seed=4,
                                    steps_before_giving_up_on_waypoint=2)
    pol = ssc.MpcPolicy(batch, graph=graph)
    chunks = []
    for _ in range(2):                              # the second chunk replays the first one's graph
        ch = env.rollout(K, pol)
        torch.cuda.synchronize()
        chunks.append({k: getattr(ch, k).clone() for k in COLS})
    snap = snapshot(env, ps, batch, [])
    snap["log"] = chunks
    return snap, batch, env


def run_separate(nav, setting, p):
    import smartstartcontinuous_amd as ssc
    nets, plans = setting
    env = ssc.VecEnv("MountainCarContinuous-v0", E, seed=21, max_episode_steps=4, env_id0=E * p)
    env.reset()
    ps = problems_of(nav, plans[E * p:E * (p + 1)])
    batch = nav.NavigatorBatch(models_of(nav, nets)[p], ps, num_control_samples=N, horizon=H, seed=4,
                               steps_before_giving_up_on_waypoint=2, problem_id0=E * p)
    pol = ssc.MpcPolicy(batch, graph=True)
    chunks = []
    for _ in range(2):
        ch = env.rollout(K, pol)
        torch.cuda.synchronize()
        chunks.append({k: getattr(ch, k).clone() for k in COLS})
    snap = snapshot(env, ps, batch, [])
    snap["log"] = chunks
    return snap


def assert_same(a, b, what):
    for c in range(2):
        for k in COLS:
            assert torch.equal(a["log"][c][k], b["log"][c][k]), (what, c, k)
    for k in ("cur_idx", "actions_done", "at_goal", "s0", "s1", "steps", "ep_ret"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert a["t"] == b["t"] == 2 * K
    assert a["stats"][2] == b["stats"][2] and a["stats"][3] == b["stats"][3], what      # steps and episodes: integers


def test_one_graph_steps_every_models_navigators(nav, setting, monkeypatch):
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 2)
    graph, batch, _ = run_population(nav, setting, True)
    assert batch.sim_ways == ["many"] * 3
    eager, _, _ = run_population(nav, setting, False)
    assert_same(graph, eager, "grouped: graph / eager")
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", False)
    alone_graph, batch, _ = run_population(nav, setting, True)
    assert batch.sim_ways == ["alone"] * 3
    alone_eager, _, _ = run_population(nav, setting, False)
    assert_same(graph, alone_graph, "grouped / alone, graph")
    assert_same(graph, alone_eager, "grouped / alone, eager")
    # three runs of their own: env_id0 = problem_id0 = 5 p
    steps = episodes = 0
    for p in range(len(DEPTHS)):
        own = run_separate(nav, setting, p)
        sl = slice(E * p, E * (p + 1))
        for c in range(2):
            for k in COLS:                      # [K, n] columns ([d, K, n] for the observations): envs are the last axis
                assert torch.equal(graph["log"][c][k][..., sl], own["log"][c][k]), (p, c, k)
        for k in ("cur_idx", "actions_done", "at_goal", "s0", "s1", "steps", "ep_ret"):
            assert torch.equal(graph[k][sl], own[k]), (p, k)
        steps += own["stats"][2]
        episodes += own["stats"][3]
    assert graph["stats"][2] == steps == 2 * K * E * len(DEPTHS) and graph["stats"][3] == episodes > 0
    # the models differ: a population that used one network for everyone would not pass the comparison above
    assert not torch.equal(graph["log"][0]["act"][:, :E], graph["log"][0]["act"][:, E:2 * E])


def test_graph_key_follows_every_models_weights_and_statistics(nav, setting, monkeypatch):
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    _, batch, env = run_population(nav, setting, True)
    nets, _ = setting
    key = batch.graph_key(env, None, None)
    assert batch.graph_key(env, None, None) == key
    for p, model in enumerate(batch.models.models):
        Ws, bs, norm = nets[p]
        old = (model.W, model.b)
        model.set_weights([w.copy() for w in Ws], [b.copy() for b in bs])            # new tensors: another pointer
        assert batch.graph_key(env, None, None) != key, p
        model.W, model.b = old
        model.set_weights(*old)                                                      # (the old tensors back: no copy)
        assert batch.graph_key(env, None, None) == key, p
        model.set_norm(dict(norm, std_z=np.asarray(norm["std_z"]) * 2))
        assert batch.graph_key(env, None, None) != key, p
        model.set_norm(norm)
        assert batch.graph_key(env, None, None) == key, p
    # the item table's addresses belong to the key too
    di = batch.models._items["sim"]
    assert any(x == (di.h_ptr, di.d_ptr) for x in _flat(key))


def _flat(key):
    for x in key:
        yield x
        if isinstance(x, tuple):
            yield from _flat(x)
