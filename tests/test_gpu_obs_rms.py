"""normalize_observations on the GPU: the RunningMeanStd update kernel, the *_rms network kernels against the plain
kernels fed x_hat, the normalising rollout, and the loops that keep the statistics."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _numpy_update(block, x):
    """RunningMeanStd.update restated: f64 sums of x and x^2, and the row count."""
    d = x.shape[1]
    x = x.astype(np.float64)
    block[:d] += x.sum(0)
    block[d:2 * d] += np.square(x).sum(0)
    block[2 * d] += len(x)


def _fill_chunk(chunk, rng):
    for c in range(chunk.obs_dim):
        chunk.obs[c].copy_(torch.as_tensor(rng.normal(0.3 * c - 0.5, 0.7, size=(chunk.K, chunk.N)).astype(np.float32)))


@pytest.mark.parametrize("packed", [False, True])
def test_update_chunk_matches_f64_numpy(ssc, packed):
    from smartstartcontinuous_amd.obs_rms import ObsRms, rms_initial
    from smartstartcontinuous_amd.vec_env import TransitionChunk
    rng = np.random.default_rng(3)
    for obs_dim, K, n, k0 in ((2, 9, 1000, 3), (3, 5, 70001, 0), (2, 64, 4099, 63)):
        chunk = TransitionChunk(obs_dim, K, n, "cuda", packed=packed)
        _fill_chunk(chunk, rng)
        a, b = ObsRms(obs_dim), ObsRms(obs_dim)
        for r in (a, b):
            r.update_chunk(chunk, k0, K)
            r.update_chunk(chunk, 0, K)
        ref = rms_initial(obs_dim)
        obs = chunk.obs.cpu().numpy()                                   # [obs_dim, K, n]
        for lo in (k0, 0):
            _numpy_update(ref, obs[:, lo:K].reshape(obs_dim, -1).T)
        got = a.block.cpu().numpy()
        scale = np.concatenate([np.abs(obs[:, k0:]).sum((1, 2)) + np.abs(obs).sum((1, 2)),
                                np.square(obs[:, k0:].astype(np.float64)).sum((1, 2)) + np.square(obs.astype(np.float64)).sum((1, 2))])
        assert np.all(np.abs(got[:-1] - ref[:-1]) <= 1e-12 * scale + 1e-12), (obs_dim, K, n, k0)
        assert got[-1] == ref[-1] and got[-1] == pytest.approx(1e-2 + (K - k0) * n + K * n, rel=0, abs=1e-9)
        assert torch.equal(a.block, b.block)                            # run to run: the same bits


def test_update_rows_one_at_a_time(ssc):
    from smartstartcontinuous_amd.obs_rms import ObsRms, rms_initial
    rng = np.random.default_rng(4)
    for d in (2, 3, 8):
        r = ObsRms(d)
        ref = rms_initial(d)
        for _ in range(25):
            x = rng.normal(1.0, 2.0, size=(1, d)).astype(np.float32)
            r.update_rows(x)
            _numpy_update(ref, x)                                       # sequential: exactly the same additions
        assert np.array_equal(r.block.cpu().numpy(), ref)
        x = rng.normal(size=(300, d)).astype(np.float32)
        r.update_rows(torch.as_tensor(x, device="cuda"))
        _numpy_update(ref, x)
        assert abs(r.block[-1].item() - ref[-1]) == 0


def _tight_stats(ssc, obs_dim, seed):
    """Statistics whose std sits at its 0.1 floor: observations a few tenths from the mean hit the +-5 clip."""
    from smartstartcontinuous_amd.obs_rms import ObsRms
    r = ObsRms(obs_dim)
    rng = np.random.default_rng(seed)
    r.update_rows(rng.normal(np.linspace(-0.5, 0.3, obs_dim), 0.02, size=(500, obs_dim)).astype(np.float32))
    return r


def _fma_stats(ssc, obs_dim, seed):
    """Statistics ABOVE the floor, with a nonzero mean, chosen so that contracting sq - mean * mean into one fused
    multiply-add would change the last bit of std in every component: the device derivation must be the plain one."""
    from smartstartcontinuous_amd.obs_rms import ObsRms, mean_std_f32
    rng = np.random.default_rng(seed)
    means, sqs = [], []
    while len(means) < obs_dim:
        m = np.float32(rng.uniform(0.2, 1.0))
        sq = np.float32(np.float64(m) * np.float64(m) + rng.uniform(0.02, 0.3))
        fused = np.float32(np.float64(sq) - np.float64(m) * np.float64(m))
        plain = np.float32(sq - np.float32(m * m))
        if np.float32(np.sqrt(fused)) != np.float32(np.sqrt(plain)):
            means.append(m)
            sqs.append(sq)
    block = np.array(means + sqs + [1.0], np.float64)          # count 1: both f32 casts are exact
    r = ObsRms(obs_dim)
    r.block.copy_(torch.as_tensor(block))
    mean, std = mean_std_f32(block)
    assert np.all(std > np.float32(0.1)) and np.all(mean != 0)
    return r


STATS = {"tight": _tight_stats, "fma": _fma_stats}


def _x_hat(x, rms, clip=5.0):
    """clip((x - mean) / std) in fp32 on the host (IEEE, one rounding per operation)."""
    mean, std = rms.mean_std()
    xh = (torch.as_tensor(x, dtype=torch.float32).cpu() - torch.as_tensor(mean)) / torch.as_tensor(std)
    return xh.clamp(-clip, clip)


def _agent(ssc, obs_dim=2, h=(64, 32), precision="f32", layer_norm=False, seed=7, batch=64):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    env = ssc.make("MountainCarContinuous-v0" if obs_dim == 2 else "Pendulum-v0")
    return DDPG_Baselines_agent(env, None, actor_h1=h[0], actor_h2=h[1], critic_h1=h[0], critic_h2=h[1], lastLayerTanh=True,
                                precision=precision, layer_norm=layer_norm, seed=seed, batch_size=batch, training=False)


@pytest.mark.parametrize("stats", ["tight", "fma"])
@pytest.mark.parametrize("obs_dim", [2, 3])
@pytest.mark.parametrize("kind,h", [("f32", (64, 32)), ("f32", (128, 64)), ("layer_norm", (64, 32)), ("mfma", (64, 32)),
                                    ("mfma", (128, 64)), ("mfma", (200, 100))])
def test_forward_rms_equals_plain_forward_on_x_hat(ssc, kind, h, obs_dim, stats):
    """Every forward kernel family (fp32 64-32 / row / generic, LayerNorm, MFMA 64-32 / 128-64 / LDS-staged 200-100) for
    MountainCar and Pendulum observation sizes: actor_forward_rms(x) == actor_forward(x_hat) bit for bit, same for the
    critic."""
    agent = _agent(ssc, obs_dim, h=h, precision="bf16_mfma" if kind == "mfma" else "f32", layer_norm=kind == "layer_norm")
    rms = STATS[stats](ssc, obs_dim, 1)
    rng = np.random.default_rng(2)
    for m in (1, 7, 1000):
        x = rng.uniform(-1.2, 0.8, size=(m, obs_dim)).astype(np.float32)
        xh = _x_hat(x, rms)
        if m > 1:
            assert float(xh.abs().max()) == 5.0                         # the clip acts
        a_rms = agent.actor(x, obs_rms=rms)
        a_ref = agent.actor(xh)
        assert torch.equal(a_rms, a_ref), (kind, m)
        act = torch.as_tensor(rng.uniform(-1, 1, size=(m, 1)).astype(np.float32))
        assert torch.equal(agent.critic(x, act, obs_rms=rms), agent.critic(xh, act)), (kind, m)


@pytest.mark.parametrize("stats", ["tight", "fma"])
@pytest.mark.parametrize("shape", [((64, 32), 64), ((64, 32), 128), ((128, 64), 64), ((64, 32), 96)])
def test_train_on_rms_equals_train_on_x_hat(ssc, shape, stats):
    """One-workgroup 64-32, tiled 64-32 (batch 128), wide (128-64, and 64-32 at batch 96): raw replay + statistics == the
    replay with s, s2 replaced by x_hat, in weights and losses."""
    h, batch = shape
    a1, a2 = _agent(ssc, 2, h, batch=batch), _agent(ssc, 2, h, batch=batch)
    rms = STATS[stats](ssc, 2, 5)
    rng = np.random.default_rng(6)
    cap, iters = 3000, 4
    s = rng.uniform(-1.2, 0.6, size=(cap, 2)).astype(np.float32)
    s2 = (s + rng.normal(0, 0.05, size=s.shape)).astype(np.float32)
    dev = lambda v, dt=torch.float32: torch.as_tensor(v, dtype=dt).cuda().contiguous()
    a = dev(rng.uniform(-1, 1, size=(cap, 1)))
    r = dev(rng.normal(size=cap))
    t = dev(rng.random(cap) < 0.05, torch.uint8)
    idx = dev(rng.integers(0, cap, size=(iters, batch)), torch.int32)
    l1 = a1.train_on(dev(s), a, r, t, dev(s2), idx, iters, obs_rms=rms)
    l2 = a2.train_on(_x_hat(s, rms).cuda(), a, r, t, _x_hat(s2, rms).cuda(), idx, iters)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2)
    assert torch.equal(a1.actor_flat, a2.actor_flat) and torch.equal(a1.critic_flat, a2.critic_flat)
    assert torch.equal(a1.target_actor_flat, a2.target_actor_flat) and torch.equal(a1.target_critic_flat, a2.target_critic_flat)


@pytest.mark.parametrize("precision", ["bf16_mfma", "f32"])
def test_rollout_rms(ssc, precision):
    """The normalising rollout: identity statistics (mean 0, std 1) reproduce the plain rollout bit for bit; tight
    statistics give the actions of the normalising forward kernel (noise off: sigma = mu = 0).  The oracle checks of the
    normalising rollouts are in test_gpu_obs_rms_oracle.py."""
    from smartstartcontinuous_amd.obs_rms import ObsRms
    agent = _agent(ssc, 2, precision=precision)
    agent.ou = dict(mu=0.0, sigma=0.0, theta=0.15)
    n, K = 3000, 40

    def run(rms):
        env = ssc.VecEnv("MountainCarContinuous-v0", n, seed=9)
        env.reset()
        return env.rollout(K, agent.as_policy(precision=precision, obs_rms=rms))
    ident = ObsRms(2)
    ident.block.copy_(torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0], dtype=torch.float64))
    plain, same = run(None), run(ident)
    assert torch.equal(plain.act, same.act) and torch.equal(plain.obs, same.obs)
    rms = _tight_stats(ssc, 2, 8)
    ch = run(rms)
    obs = ch.obs.permute(1, 2, 0).reshape(-1, 2).contiguous()
    want = agent.actor(obs, obs_rms=rms).reshape(K, n)
    err = float((ch.act - want.clamp(-1, 1)).abs().max())
    # f32: the same device code; MFMA: the fused bf16 policy vs the forward kernel (and a corrected reciprocal)
    assert err <= (1e-6 if precision == "f32" else 2e-2), err
    assert not torch.equal(ch.act, plain.act)


def _vec_ddpg(ssc, overlap, n=512, K=16, chunks=3, last=4):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    env = ssc.VecEnv("MountainCarContinuous-v0", n, seed=11)
    agent = DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, actor_h1=64, actor_h2=32, critic_h1=64,
                                 critic_h2=32, lastLayerTanh=True, normalize_observations=True, seed=3, num_train_iterations=5)
    ssc.rl_train_vec_ddpg(env, agent, chunks, chunk_steps=K, replay_capacity=1 << 16, train_iters=5, replay_last_steps=last,
                          seed=2, overlap=overlap)
    torch.cuda.synchronize()
    return agent


def test_vec_ddpg_replay_last_steps_zero(ssc):
    """replay_last_steps=0 appends nothing, so the statistics do not move either."""
    agent = _vec_ddpg(ssc, False, chunks=2, last=0)
    assert agent.obs_rms.block[-1].item() == 1e-2


@pytest.mark.parametrize("overlap", [False, True])
def test_vec_ddpg_keeps_statistics(ssc, overlap):
    a, b = _vec_ddpg(ssc, overlap), _vec_ddpg(ssc, overlap)
    assert a.obs_rms.block[-1].item() == pytest.approx(1e-2 + 3 * 4 * 512, rel=0, abs=1e-9)
    assert torch.equal(a.obs_rms.block, b.obs_rms.block)
    assert torch.equal(a.actor_flat, b.actor_flat) and torch.equal(a.critic_flat, b.critic_flat)
    mean, std = a.obs_rms.mean_std()
    assert -1.2 <= mean[0] <= 0.6 and np.all(std > 0)


def test_scalar_rltrain_counts_every_observe(ssc):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    env = ssc.Continuous_MountainCarEnv_Editted.make_timed_env(1.0, max_episode_steps=30)
    agent = DDPG_Baselines_agent(env, None, batch_size=16, num_train_iterations=2, num_steps_before_train=8, actor_h1=64,
                                 actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True, normalize_observations=True,
                                 seed=1)
    np.random.seed(0)
    ssc.rlTrain(agent, env, print_results=False, print_steps=False, num_episodes=2, max_steps=1000)
    assert agent.obs_rms.block[-1].item() == pytest.approx(1e-2 + 60, rel=0, abs=1e-9)
    s = agent.replay_buffer.all_batch()[0]
    assert np.allclose(agent.obs_rms.block[:2].cpu().numpy(), s.astype(np.float64).sum(0), rtol=1e-12, atol=1e-12)


def test_constructor_flags(ssc):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    env = ssc.make("MountainCarContinuous-v0")
    assert DDPG_Baselines_agent(env, None, normalize_observations=True, seed=1).obs_rms is not None
    for kw in (dict(normalize_returns=True), dict(enable_popart=True)):
        with pytest.raises(NotImplementedError, match="return normalisation / popart"):
            DDPG_Baselines_agent(env, None, **kw)


def test_vec_smartstart_with_normalisation(ssc):
    """The vectorised SmartStart step (HIP-graph replayed) with a normalising agent: the base agent's actions are
    clip(Actor(x_hat)) of the statistics, bit for bit (OU epsilon 0, every env in agent mode before any plan exists), and
    the loop keeps the statistics."""
    from smartstartcontinuous_amd import navigator as nav
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.vec_env import TransitionChunk
    from tests.gpu_util import actor_weights
    from tests.test_gpu_navigator import make_mlp, make_norm
    n, K, seed = 256, 16, 2
    rng = np.random.default_rng(seed)
    env = ssc.VecEnv("MountainCarContinuous-v0", n, seed=seed, max_episode_steps=24, env_id0=40)
    env.reset()
    agent = DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32,
                                 lastLayerTanh=True, seed=5, training=False, ou_mu=0.4, ou_sigma=0.6, precision="f32",
                                 normalize_observations=True)
    agent.set_weights({k: torch.as_tensor(v) for k, v in actor_weights(2, 64, 32, seed=77, w3_scale=0.5).items()})
    agent.obs_rms.update_rows(rng.normal([-0.5, 0.0], [0.3, 0.05], size=(200, 2)).astype(np.float32))
    Ws, bs = make_mlp(rng, (3, 32, 2))
    model = nav.DynamicsModel(Ws, bs, make_norm(rng, 2, 1), state_dim=2, act_dim=1, precision="f32")
    smart = ssc.VecSmartStart(env, agent, model, eta=0.9, n_plans=2, num_control_samples=32, horizon=3,
                              steps_before_giving_up_on_waypoint=2, final_steps=4, chunk_steps=K, seed=seed + 1, log_modes=True,
                              w_max=25)
    agent.decaying_ou_action_noise.epsilon = 0.0
    chunk = TransitionChunk(2, K, n, env.device)
    smart.rollout(K, chunk)
    torch.cuda.synchronize()
    assert int(smart.mode_log.sum()) == 0                               # no plans yet: the base agent acted everywhere
    obs = chunk.obs.permute(1, 2, 0).reshape(-1, 2).contiguous()
    want = agent.actor(obs).reshape(K, n).clamp(-1, 1)
    assert torch.equal(chunk.act, want)
    rms, agent.obs_rms = agent.obs_rms, None
    plain = agent.actor(obs).reshape(K, n).clamp(-1, 1)
    agent.obs_rms = rms
    assert not torch.equal(chunk.act, plain)
    # Q(s, pi(s)) of the SmartStart selection goes through the same statistics
    v = agent.state_value_device(obs[:100])
    assert torch.equal(v, agent.critic(obs[:100], agent.actor(obs[:100], obs_rms=rms), obs_rms=rms))
    # the loop: one statistics update per appended chunk
    agent.training_enabled = True
    agent.batch_size, agent.num_train_iterations = 64, 3
    before = agent.obs_rms.block[-1].item()
    summary, losses, replay = ssc.rl_train_vec_smartstart(env, smart, 3, chunk_steps=K, replay_capacity=1 << 15, train_iters=3)
    torch.cuda.synchronize()
    assert agent.obs_rms.block[-1].item() == pytest.approx(before + 3 * K * n, rel=0, abs=1e-9)
    assert len(losses) >= 2 and all(bool(torch.isfinite(l).all()) for l in losses)
