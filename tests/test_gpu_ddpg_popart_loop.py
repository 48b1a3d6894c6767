"""A Pop-Art agent on the vectorised actor-learner loop: ``rl_train_vec_ddpg`` with 64 envs, 4 chunks of 16 steps, batch
64, 2 iterations per chunk and ``stats_every=1`` -- synchronous and ``overlap=True`` -- and the loops that refuse it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ENV = "MountainCarContinuous-v0"
N_ENVS, K, CHUNKS, BATCH, ITERS = 64, 16, 4, 64, 2


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def make_agent(ssc, **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    kw = dict(dict(normalize_returns=True, enable_popart=True), **kw)
    return DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=BATCH, num_train_iterations=ITERS, actor_h1=64, actor_h2=32,
                                critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7, **kw)


_RUNS = {}


def run(ssc, overlap, tag=0):
    key = (overlap, tag)
    if key not in _RUNS:
        agent = make_agent(ssc)
        env = ssc.VecEnv(ENV, N_ENVS, seed=5, max_episode_steps=60)
        history = []

        def on_chunk(i, chunk, env):
            history.append(agent.ret_rms.block.clone())          # stream-ordered behind the chunk's iterations
        summary, losses, replay = ssc.rl_train_vec_ddpg(env, agent, CHUNKS, chunk_steps=K, train_iters=ITERS, seed=3, overlap=overlap,
                                                        replay_capacity=1 << 14, stats_every=1, on_chunk=on_chunk)
        torch.cuda.synchronize()
        _RUNS[key] = dict(agent=agent, summary=summary, losses=losses, history=[h.cpu().numpy() for h in history])
    return _RUNS[key]


@pytest.mark.parametrize("overlap", [False, True])
def test_loop_runs_and_counts(ssc, overlap):
    from smartstartcontinuous_amd.obs_rms import mean_std_f32
    r = run(ssc, overlap)
    assert len(r["losses"]) == CHUNKS and all(np.all(np.isfinite(l.cpu().numpy())) for l in r["losses"])
    count = 1e-2
    for _ in range(CHUNKS * ITERS):
        count += float(BATCH)
    block = r["agent"].ret_rms.block.cpu().numpy()
    assert block[2] == count and block[1] > 1e-2
    # summary.ret_rms: one row per chunk, the fp32 (mean, std) of the block as it stood behind that chunk's iterations
    ret = r["summary"].ret_rms
    assert sorted(ret) == ["mean", "std"] and ret["mean"].shape == ret["std"].shape == (CHUNKS,)
    assert ret["mean"].dtype == np.float32 and ret["std"].dtype == np.float32
    for row, b in enumerate(r["history"]):
        mean, std = mean_std_f32(b, 1)
        assert ret["mean"][row:row + 1].tobytes() == mean.tobytes() and ret["std"][row:row + 1].tobytes() == std.tobytes()
    assert np.all(np.isfinite(r["summary"].agent_stats["reference_Q_mean"]))


def test_second_run_gives_the_same_bits(ssc):
    a, b = run(ssc, False), run(ssc, False, tag=1)
    for name in ("actor_flat", "critic_flat", "target_actor_flat", "target_critic_flat"):
        assert getattr(a["agent"], name).cpu().numpy().tobytes() == getattr(b["agent"], name).cpu().numpy().tobytes(), name
    assert a["agent"].ret_rms.block.cpu().numpy().tobytes() == b["agent"].ret_rms.block.cpu().numpy().tobytes()
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a["losses"], b["losses"]))
    assert a["summary"].ret_rms["std"].tobytes() == b["summary"].ret_rms["std"].tobytes()


def test_overlap_advances_count_by_the_same_amount(ssc):
    assert run(ssc, True)["agent"].ret_rms.block[2].item() == run(ssc, False)["agent"].ret_rms.block[2].item()


def test_agents_without_return_statistics_get_no_ret_rms_log(ssc):
    agent = make_agent(ssc, normalize_returns=False, enable_popart=False)
    env = ssc.VecEnv(ENV, N_ENVS, seed=5, max_episode_steps=60)
    summary, losses, _ = ssc.rl_train_vec_ddpg(env, agent, 2, chunk_steps=K, train_iters=ITERS, seed=3, replay_capacity=1 << 14,
                                               stats_every=1)
    assert not hasattr(summary, "ret_rms") and agent.ret_rms is None and len(losses) == 2


def test_sharded_and_smartstart_loops_refuse(ssc):
    agent = make_agent(ssc)
    env = ssc.VecEnv(ENV, N_ENVS, seed=5)
    from smartstartcontinuous_amd.sharding import rl_train_sharded_ddpg
    with pytest.raises(NotImplementedError, match="Pop-Art"):
        rl_train_sharded_ddpg(env, agent, 1, K, 0, 1)
    with pytest.raises(NotImplementedError, match="Pop-Art"):
        ssc.VecSmartStart(env, agent, None)

    class Smart:
        pass
    smart = Smart()
    smart.agent = agent
    with pytest.raises(NotImplementedError, match="Pop-Art"):
        ssc.rl_train_vec_smartstart(env, smart, 1)
