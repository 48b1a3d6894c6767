"""navigator.NavigatorPopulation with bf16-MFMA dynamics models: the class-default 1 x 500 networks of several seeds in ONE
VecEnv, stepped by one captured graph whose forward simulation is one ssc_mpc_forward_sim_many_mfma launch.  The graph path,
the eager path, both again with NAV_POPULATION_GROUPED = False (every model through its own call and a strided copy) and
separate (VecEnv, NavigatorBatch) runs give every env the same bits -- transition log, waypoint bookkeeping, env state.  The
f64 chunk statistics sum over all envs in another order than per model: only their integer entries are compared."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import sim_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E, N, H, K = 3, 16, 4, 5
COLS = ("obs", "act", "rew", "done", "obs2")
STATE = ("cur_idx", "actions_done", "at_goal", "s0", "s1", "steps", "ep_ret")
SAME_CLASS = [((3, 500, 2), "bf16_mfma")] * 3
MIXED = [((3, 32, 2), "f32"), ((3, 32, 2), "f32"), ((3, 500, 2), "bf16_mfma"), ((3, 500, 2), "bf16_mfma"),
         ((3, 500, 500, 2), "bf16_mfma")]


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


def make_setting(spec, seed):
    rng = np.random.default_rng(seed)
    nets = [SC.make_mlp(rng, dims) + (SC.make_norm(rng, 2, 1), prec) for dims, prec in spec]
    paths = [np.cumsum(rng.normal(scale=[0.02, 0.004], size=(12, 2)), axis=0) + [-0.5, 0.0] for _ in range(len(spec) * E)]
    plans = []
    for pth in paths:
        stds, means = O.path_deltas_stds_and_means_per_dim(pth)
        r = O.radii_calc(means, stds, 1, 1, 1) + 1e-3
        plans.append((pth, O.distances_left(pth, O.distance_func(r)), r))
    return nets, plans


def models_of(nav, nets):
    return [nav.DynamicsModel(Ws, bs, norm, state_dim=2, act_dim=1, precision=prec) for Ws, bs, norm, prec in nets]


def problems_of(nav, plans):
    return nav.MpcProblemSet([p[0] for p in plans], [p[1] for p in plans], [p[2] for p in plans], [0] * len(plans))


def training_set(model, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((64, model.in_dim), generator=g).cuda()
    Z = torch.randn((64, model.out_dim), generator=g).cuda()
    idx = torch.randint(0, 64, (3, 16), generator=g, dtype=torch.int32).cuda()
    return X, Z, idx


def rollout_chunks(env, pol, n=2):
    chunks = []
    for _ in range(n):
        ch = env.rollout(K, pol)
        torch.cuda.synchronize()
        chunks.append({k: getattr(ch, k).clone() for k in COLS})
    return chunks


def snapshot(env, ps, batch, chunks):
    torch.cuda.synchronize()
    return dict(log=chunks, cur_idx=ps.cur_idx.clone(), actions_done=batch.actions_done.clone(), at_goal=batch.at_goal.clone(),
                s0=env.s0.clone(), s1=env.s1.clone(), steps=env.steps.clone(), ep_ret=env.ep_ret.clone(),
                stats=env.stats.cpu().numpy().copy(), t=env.t)


def run_population(nav, setting, graph, retrain=None):
    """two chunks; `retrain` = the model that takes three Adam steps before the first chunk (so that its optimiser state and
    workspace exist) and three more between the chunks"""
    import smartstartcontinuous_amd as ssc
    nets, plans = setting
    env = ssc.VecEnv("MountainCarContinuous-v0", len(plans), seed=21, max_episode_steps=4)
    env.reset()
    ps = problems_of(nav, plans)
    models = models_of(nav, nets)
    batch = nav.NavigatorPopulation(models, ps, E, num_control_samples=N, horizon=H, seed=4, steps_before_giving_up_on_waypoint=2)
    pol = ssc.MpcPolicy(batch, graph=graph)
    keys = []
    if retrain is None:
        chunks = rollout_chunks(env, pol)
    else:
        data = training_set(models[retrain], 7)
        models[retrain].train_steps(*data, lr=0.05)
        chunks = rollout_chunks(env, pol, 1)
        keys.append(batch.graph_key(env, None, None))
        models[retrain].train_steps(*data, lr=0.05)
        chunks += rollout_chunks(env, pol, 1)
        keys.append(batch.graph_key(env, None, None))
    return snapshot(env, ps, batch, chunks), batch, keys


def run_separate(nav, setting, p):
    import smartstartcontinuous_amd as ssc
    nets, plans = setting
    env = ssc.VecEnv("MountainCarContinuous-v0", E, seed=21, max_episode_steps=4, env_id0=E * p)
    env.reset()
    ps = problems_of(nav, plans[E * p:E * (p + 1)])
    batch = nav.NavigatorBatch(models_of(nav, nets)[p], ps, num_control_samples=N, horizon=H, seed=4,
                               steps_before_giving_up_on_waypoint=2, problem_id0=E * p)
    return snapshot(env, ps, batch, rollout_chunks(env, ssc.MpcPolicy(batch, graph=True)))


def assert_same(a, b, what):
    for c in range(2):
        for k in COLS:
            assert torch.equal(a["log"][c][k], b["log"][c][k]), (what, c, k)
    for k in STATE:
        assert torch.equal(a[k], b[k]), (what, k)
    assert a["t"] == b["t"] == 2 * K
    assert a["stats"][2] == b["stats"][2] and a["stats"][3] == b["stats"][3], what      # steps and episodes: integers


def assert_equals_separate_runs(nav, setting, pop):
    steps = episodes = 0
    n_models = len(setting[0])
    for p in range(n_models):
        own = run_separate(nav, setting, p)
        sl = slice(E * p, E * (p + 1))
        for c in range(2):
            for k in COLS:                      # [K, n] columns ([d, K, n] for the observations): envs are the last axis
                assert torch.equal(pop["log"][c][k][..., sl], own["log"][c][k]), (p, c, k)
        for k in STATE:
            assert torch.equal(pop[k][sl], own[k]), (p, k)
        steps += own["stats"][2]
        episodes += own["stats"][3]
    assert pop["stats"][2] == steps == 2 * K * E * n_models and pop["stats"][3] == episodes > 0


def test_one_graph_steps_a_population_of_class_default_models(nav, monkeypatch):
    setting = make_setting(SAME_CLASS, 41)
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "NAV_POPULATION_MFMA_MIN_GROUP", 2)
    graph, batch, _ = run_population(nav, setting, True)
    assert batch.sim_ways == ["mfma<16,1>"] * 3
    assert sorted(batch.models._sim_mfma) == ["mfma<16,1>"] and batch.models._sim_mfma["mfma<16,1>"].n == 3
    eager, batch, _ = run_population(nav, setting, False)
    assert batch.sim_ways == ["mfma<16,1>"] * 3
    assert_same(graph, eager, "grouped: graph / eager")
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", False)
    alone_graph, batch, _ = run_population(nav, setting, True)
    assert batch.sim_ways == ["alone"] * 3 and not batch.models._sim_mfma
    alone_eager, batch, _ = run_population(nav, setting, False)
    assert batch.sim_ways == ["alone"] * 3
    assert_same(graph, alone_graph, "grouped / alone, graph")
    assert_same(graph, alone_eager, "grouped / alone, eager")
    assert_equals_separate_runs(nav, setting, graph)
    # the models differ: a population that used one network for everyone would not pass the comparisons above
    assert not torch.equal(graph["log"][0]["act"][:, :E], graph["log"][0]["act"][:, E:2 * E])


def test_a_mixed_population_equals_per_model_runs(nav, monkeypatch):
    setting = make_setting(MIXED, 43)
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 2)
    monkeypatch.setattr(nav, "NAV_POPULATION_MFMA_MIN_GROUP", 2)
    graph, batch, _ = run_population(nav, setting, True)
    assert batch.sim_ways == ["many", "many", "mfma<16,1>", "mfma<16,1>", "alone"]
    assert_equals_separate_runs(nav, setting, graph)


def test_retraining_changes_the_next_chunk_under_the_same_graph_key(nav, monkeypatch):
    setting = make_setting(SAME_CLASS, 47)
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "NAV_POPULATION_MFMA_MIN_GROUP", 2)
    trained, batch, keys = run_population(nav, setting, True, retrain=1)
    assert batch.sim_ways == ["mfma<16,1>"] * 3
    assert keys[0] == keys[1]                    # same weights tensors, same image buffer, same table: the graph is replayed
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", False)
    yardstick, _, _ = run_population(nav, setting, True, retrain=1)
    assert_same(trained, yardstick, "retrained: grouped / alone")
    # the second chunk saw the re-packed image: a run whose model stops learning after the first three steps differs there,
    # in model 1's envs and nowhere else
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    import smartstartcontinuous_amd as ssc
    nets, plans = setting
    env = ssc.VecEnv("MountainCarContinuous-v0", len(plans), seed=21, max_episode_steps=4)
    env.reset()
    models = models_of(nav, nets)
    batch = nav.NavigatorPopulation(models, problems_of(nav, plans), E, num_control_samples=N, horizon=H, seed=4,
                                    steps_before_giving_up_on_waypoint=2)
    models[1].train_steps(*training_set(models[1], 7), lr=0.05)
    stale = rollout_chunks(env, ssc.MpcPolicy(batch, graph=True))
    sl = slice(E, 2 * E)
    assert torch.equal(stale[0]["act"], trained["log"][0]["act"])
    assert not torch.equal(stale[1]["act"][:, sl], trained["log"][1]["act"][:, sl])
    others = [e for e in range(3 * E) if not E <= e < 2 * E]
    assert torch.equal(stale[1]["act"][:, others], trained["log"][1]["act"][:, others])
