"""``DDPG_Baselines_agent.evaluate_device`` / ``evaluate`` and ``rl_train_vec_ddpg(eval_env=, eval_every=, eval_steps=)``: the
evaluations logged on the device change nothing the loop computes, land in the rows they belong to, and use the plain
actor.  MountainCar, 256 envs, chunks of 16 steps, 6 chunks, batch 64, 3 iterations, ``max_episode_steps=60`` so that
episodes finish and epsilon decays inside the run; 32 eval envs x 24 steps with a time limit of 20, so every evaluation
finishes episodes."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import eval_cases as E

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_ENVS, K, CHUNKS, BATCH, ITERS = 256, 16, 6, 64, 3
EVAL_ENVS, EVAL_STEPS, EVAL_LIMIT = 32, 24, 20
ENV = "MountainCarContinuous-v0"
KINDS = {"plain": {}, "param_noise": dict(param_noise_stddev=0.2), "normalize": dict(normalize_observations=True)}
RING = ("s", "a", "r", "t", "s2")
ENV_STATE = ("s0", "s1", "steps", "ep_ret", "ou_x", "stats")
TOL_ACT = 2e-5                  # fp32 actor rollouts on unit action bounds


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def make_agent(ssc, kind="plain"):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    return DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=BATCH, num_train_iterations=ITERS, actor_h1=64,
                                actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7, **KINDS[kind])


def eval_env(ssc):
    return ssc.VecEnv(ENV, EVAL_ENVS, seed=17, env_id0=1000, max_episode_steps=EVAL_LIMIT)


_RUNS = {}


def run(ssc, overlap, kind, eval_every, chunks=CHUNKS):
    """one loop per variant, computed once and shared by the tests below"""
    key = (overlap, kind, eval_every, chunks)
    if key not in _RUNS:
        agent = make_agent(ssc, kind)
        env = ssc.VecEnv(ENV, N_ENVS, seed=5, max_episode_steps=60)
        kw = {} if eval_every is None else dict(eval_env=eval_env(ssc), eval_every=eval_every, eval_steps=EVAL_STEPS)
        summary, losses, replay = ssc.rl_train_vec_ddpg(env, agent, chunks, chunk_steps=K, train_iters=ITERS, seed=3,
                                                        overlap=overlap, replay_capacity=1 << 16, drain_every=2, **kw)
        torch.cuda.synchronize()
        _RUNS[key] = dict(agent=agent, env=env, summary=summary, losses=losses, replay=replay, eval_env=kw.get("eval_env"))
    return _RUNS[key]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("overlap", [False, True])
def test_results_are_bit_identical_with_and_without_evaluation(ssc, overlap, kind):
    base, other = run(ssc, overlap, kind, None), run(ssc, overlap, kind, 2)
    assert not hasattr(base["summary"], "eval_stats")
    assert len(base["losses"]) == CHUNKS and len(base["summary"]) > 0
    names = ["actor_flat", "critic_flat", "target_actor_flat", "target_critic_flat", "d_epsilon", "_adam_t"]
    if kind == "param_noise":
        names += ["perturbed_actor_flat", "adaptive_actor_flat", "d_param_noise_stddev"]
    for name in names:
        assert np.array_equal(bits(getattr(base["agent"], name)), bits(getattr(other["agent"], name))), name
    for which in ("_adam_actor", "_adam_critic"):
        for a, b in zip(getattr(base["agent"], which), getattr(other["agent"], which)):
            assert np.array_equal(bits(a), bits(b)), which
    if kind == "normalize":
        assert np.array_equal(bits(base["agent"].obs_rms.block), bits(other["agent"].obs_rms.block))
    assert base["agent"].decaying_ou_action_noise.epsilon == other["agent"].decaying_ou_action_noise.epsilon
    assert len(base["losses"]) == len(other["losses"])
    for la, lb in zip(base["losses"], other["losses"]):
        assert np.array_equal(bits(la), bits(lb))
    assert len(base["replay"]) == len(other["replay"]) and base["replay"]._batches_drawn == other["replay"]._batches_drawn
    for col in RING:
        assert np.array_equal(bits(getattr(base["replay"], col)), bits(getattr(other["replay"], col))), col
    for col in ENV_STATE:
        assert np.array_equal(bits(getattr(base["env"], col)), bits(getattr(other["env"], col))), col
    # (the episode ring hands out its slots atomically: the records are the same, their order inside a drain is not)
    assert sorted(base["summary"].episodes) == sorted(other["summary"].episodes)
    # ... and the evaluations are there: three rows, every one finished episodes of EVAL_LIMIT steps
    stats, chunks = other["summary"].eval_stats, other["summary"].eval_chunks
    assert list(stats) == list(other["agent"].EVAL_NAMES) and chunks == [1, 3, 5]
    assert all(v.shape == (3,) and v.dtype == np.float64 and np.all(np.isfinite(v)) for v in stats.values())
    assert np.all(stats["eval/steps"] == EVAL_ENVS * EVAL_STEPS) and np.all(stats["eval/episodes"] >= EVAL_ENVS)
    assert other["eval_env"].t == 3 * EVAL_STEPS
    assert len(set(stats["eval/Q"].tolist())) == 3                   # the learner moves Q between the evaluations


@pytest.mark.parametrize("kind", ["plain", "normalize", "param_noise"])
@pytest.mark.parametrize("overlap", [False, True])
def test_last_row_is_what_the_agent_reports_after_the_loop(ssc, overlap, kind):
    """eval_every == num_chunks: one row, behind the last train; a second eval env with the same seed gives it again"""
    r = run(ssc, overlap, kind, CHUNKS)
    stats = r["summary"].eval_stats
    assert r["summary"].eval_chunks == [CHUNKS - 1] and all(v.shape == (1,) for v in stats.values())
    row = np.array([stats[name][0] for name in r["agent"].EVAL_NAMES])
    after = r["agent"].evaluate_device(eval_env(ssc), EVAL_STEPS).cpu().numpy()
    assert np.all(np.isfinite(row)) and np.array_equal(after.view(np.uint64), row.view(np.uint64))


@pytest.mark.parametrize("overlap", [False, True])
def test_unreached_rows_stay_nan(ssc, overlap):
    r = run(ssc, overlap, "plain", 2, chunks=5)
    stats = r["summary"].eval_stats
    assert r["summary"].eval_chunks == [1, 3, 5]
    for name, v in stats.items():
        assert v.shape == (3,) and np.all(np.isfinite(v[:2])) and np.isnan(v[2]), name


def oracle_actions(weights, obs):
    w = {k: v.cpu().numpy() for k, v in weights.items()}
    a = O.actor_forward(obs.astype(np.float64), *(w[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")), last_layer_tanh=True,
                        obs_clip=5.0)[:, 0]
    return O.ddpg_action(a, 0.0, 0.0, -1.0, 1.0)


def test_parameter_noise_agent_evaluates_its_plain_actor(ssc):
    agent = make_agent(ssc, "param_noise")
    env = eval_env(ssc)
    chunk = ssc.TransitionChunk(env.obs_dim, EVAL_STEPS, EVAL_ENVS, env.device)
    agent.evaluate_device(env, EVAL_STEPS, log=chunk)
    torch.cuda.synchronize()
    obs = np.moveaxis(chunk.obs.cpu().numpy(), 0, -1).reshape(-1, 2)
    got = chunk.act.cpu().numpy().reshape(-1).astype(np.float64)
    plain, perturbed = oracle_actions(agent.weights, obs), oracle_actions(agent.perturbed_weights, obs)
    assert np.abs(plain - perturbed).max() > 101 * TOL_ACT           # the oracle alone: the two actors can be told apart
    assert np.abs(got - plain).max() <= TOL_ACT
    assert np.abs(got - perturbed).max() > 100 * TOL_ACT


def test_evaluate_returns_the_named_dict_and_carry_returns_switches_the_return(ssc):
    agent = make_agent(ssc)
    reports = {}
    for carry in (False, True):
        env = eval_env(ssc)
        env.reset()
        env.rollout(5, ssc.RandomPolicy(), log=False)                # mid-episode, with a running return
        steps0, ret0 = env.steps.cpu().numpy(), env.ep_ret.cpu().numpy()
        assert np.all(ret0 < 0) and env.t == 5
        chunk = ssc.TransitionChunk(env.obs_dim, EVAL_STEPS, EVAL_ENVS, env.device)
        q = torch.empty((EVAL_STEPS, EVAL_ENVS), dtype=torch.float32, device="cuda")
        d = agent.evaluate(env, EVAL_STEPS, log=chunk, q=q, carry_returns=carry)
        assert list(d) == list(agent.EVAL_NAMES) and env.t == 5 + EVAL_STEPS and (chunk.step0, chunk.env_id0) == (5, 1000)
        assert all(isinstance(d[k], int) for k in ("eval/episodes", "eval/steps", "eval/goals"))
        assert all(isinstance(d[k], float) for k in agent.EVAL_NAMES if k not in ("eval/episodes", "eval/steps", "eval/goals"))
        goal = chunk.obs2[0].cpu().numpy().astype(np.float64) >= np.float64(np.float32(O.MC_GOAL_POSITION))
        want, run_ret, el = E.eval_block(chunk.rew.cpu().numpy(), chunk.done.cpu().numpy(), goal, q.cpu().numpy(), steps0, ret0,
                                         zero_returns=not carry)
        E.assert_block([d[k] for k in agent.EVAL_NAMES], want)
        assert np.array_equal(env.ep_ret.cpu().numpy().view(np.uint32), run_ret.view(np.uint32))
        assert d["eval/episodes"] == EVAL_ENVS and d["eval/steps"] == EVAL_ENVS * EVAL_STEPS
        reports[carry] = d
    assert reports[True]["eval/return"] < reports[False]["eval/return"]          # the carried part is negative
    assert reports[True]["eval/Q"] == reports[False]["eval/Q"]


def test_evaluate_device_resets_a_fresh_env_and_checks_its_arguments(ssc):
    agent = make_agent(ssc)
    env = eval_env(ssc)
    assert env._needs_reset
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    assert agent.evaluate_device(env, 3, out=out) is out and not env._needs_reset and env.t == 3
    assert not torch.any(out == 7.0)
    with pytest.raises(ValueError):
        agent.evaluate_device(env, 0)
    with pytest.raises(ValueError):
        agent.evaluate_device(env, 3, out=torch.zeros(8, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        agent.evaluate_device(ssc.VecEnv("Pendulum-v0", 4), 3)
    with pytest.raises(ValueError):
        agent.evaluate_device(env, 3, q=torch.zeros((4, EVAL_ENVS), dtype=torch.float32, device="cuda"))
    assert env.t == 3
