"""Adaptive parameter-space noise on the GPU: the perturb kernel against the oracle's Philox / Box-Muller stream, the adapt
kernel against f64 numpy, the perturbed actor in the fused rollout, the vectorised loop and the scalar agent."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TAG_PARAM_NOISE = 9
SEED = 0x5EED0000BEEF
N_ACTOR = 2 * 64 + 64 + 64 * 32 + 32 + 32 + 1            # 2305: the 64-32 actor on 2 observations
# the same actor with LayerNorm: [W1|b1|beta1|gamma1|W2|b2|beta2|gamma2|W3|b3]
N_LN, LN_SKIP = N_ACTOR + 2 * 64 + 2 * 32, (192, 320, 2400, 2464)
# the bound the Box-Muller routine is already held to (tests/test_gpu_agents.py: 1e-6 on 0.005 * g)
GAUSS_BOUND = 2e-4


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def oracle_gaussians(n, seed, generation):
    """g_i of ssc_param_noise_perturb in fp64: Philox(seed; q, generation, TAG_PARAM_NOISE) serves elements 4q .. 4q+3,
    words (0, 1) -> (cos, sin) for 4q, 4q+1, words (2, 3) -> (cos, sin) for 4q+2, 4q+3."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = O.rng_words(seed, q, np.full(len(q), generation, np.uint64), TAG_PARAM_NOISE)
    c0, s0 = O.gaussian_pair(w[0], w[1])
    c1, s1 = O.gaussian_pair(w[2], w[3])
    return np.stack([c0, s0, c1, s1], axis=1).reshape(-1)[:n]


def perturb(ssc, src, stddev, generation, skip=(0, 0, 0, 0), seed=SEED, in_place=False):
    f = ssc._ffi
    dst = src if in_place else torch.full_like(src, float("nan"))
    sd = torch.tensor([stddev], dtype=torch.float32, device="cuda")
    f.check(f.lib().ssc_param_noise_perturb(src.numel(), f.ptr(src), f.ptr(dst), f.ptr(sd), *skip, seed, generation,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return dst


@pytest.fixture(scope="module")
def gauss_err(ssc):
    """The largest |g_device - g_oracle| over the 2305 elements of the 64-32 actor: with src = 0 and stddev = 1 the
    kernel's output IS its gaussian (fma(1, g, 0) = g)."""
    g = perturb(ssc, torch.zeros(N_ACTOR, device="cuda"), 1.0, 0).cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(g - oracle_gaussians(N_ACTOR, SEED, 0))))
    print(f"param-noise gaussian: max |g_device - g_oracle| over {N_ACTOR} elements = {err:.3e}")
    assert err <= GAUSS_BOUND, err
    return err


def assert_close_to_stream(dst, src, stddev, seed, generation, skip, err):
    """|dst - (src + stddev * g_oracle)| <= 4 * err * stddev + one fp32 ulp of the sum, outside the skip ranges"""
    n = len(src)
    want = src.astype(np.float64) + float(np.float32(stddev)) * oracle_gaussians(n, seed, generation)
    tol = 4.0 * err * stddev + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    keep = perturbed_mask(n, skip)
    diff = np.abs(dst.astype(np.float64) - want)
    assert np.all(diff[keep] <= tol[keep]), (float(np.max(diff[keep] - tol[keep])), int(np.argmax(diff[keep] - tol[keep])))


def perturbed_mask(n, skip):
    keep = np.ones(n, bool)
    keep[skip[0]:skip[1]] = False
    keep[skip[2]:skip[3]] = False
    return keep


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("generation", [0, (1 << 33) + 1])
@pytest.mark.parametrize("n,skip", [(1, (0, 0, 0, 0)), (3, (0, 0, 0, 0)), (4, (0, 0, 0, 0)), (5, (0, 0, 0, 0)),
                                    (257, (0, 0, 0, 0)), (N_ACTOR, (0, 0, 0, 0)), (N_LN, LN_SKIP)])
def test_perturb_matches_oracle_stream(ssc, gauss_err, n, skip, generation):
    rng = np.random.default_rng(n)
    host = (0.1 * rng.normal(size=n)).astype(np.float32)
    host[0] = -0.0                                              # a bit copy keeps the sign of zero
    src = torch.from_numpy(host).cuda()
    out = perturb(ssc, src, 0.2, generation, skip)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got))                             # every element was written
    assert_close_to_stream(got, host, 0.2, SEED, generation, skip, gauss_err)
    keep = perturbed_mask(n, skip)
    assert np.array_equal(bits(out)[~keep], host.view(np.uint32)[~keep])          # LayerNorm segments: bit copies
    assert np.array_equal(bits(src), host.view(np.uint32))                        # the source is untouched
    assert np.array_equal(bits(perturb(ssc, src, 0.0, generation, skip)), host.view(np.uint32))   # stddev 0: a bit copy
    assert np.array_equal(bits(perturb(ssc, src, 0.2, generation, skip)), bits(out))              # same key, same bits
    other = perturb(ssc, src, 0.2, generation + 1, skip).cpu().numpy()
    pad = (-n) % 4
    differs = np.pad((other != got) & keep, (0, pad)).reshape(-1, 4).any(axis=1)
    has_perturbed = np.pad(keep, (0, pad)).reshape(-1, 4).any(axis=1)
    assert np.array_equal(differs, has_perturbed)               # another generation: every group of four draws anew
    # a different seed is a different stream as well
    assert not np.array_equal(perturb(ssc, src, 0.2, generation, skip, seed=SEED + 1).cpu().numpy()[keep], got[keep])
    inplace = src.clone()
    perturb(ssc, inplace, 0.2, generation, skip, in_place=True)
    assert np.array_equal(bits(inplace), bits(out))             # in place == out of place


def adapt(ssc, a, b, desired, coefficient, sd):
    f = ssc._ffi
    dist = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    f.check(f.lib().ssc_param_noise_adapt(a.numel(), f.ptr(a), f.ptr(b), desired, coefficient, f.ptr(sd), f.ptr(dist),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return float(dist.item())


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4096, 4096 * 4])
def test_adapt_matches_numpy(ssc, count):
    from smartstartcontinuous_amd.agents import AdaptiveParamNoiseSpec
    rng = np.random.default_rng(count)
    ha, hb = rng.uniform(-1, 1, count).astype(np.float32), rng.uniform(-1, 1, count).astype(np.float32)
    ref = float(np.sqrt(np.mean((ha.astype(np.float64) - hb.astype(np.float64)) ** 2)))
    assert ref > 1e-3
    a, b = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
    sd = torch.tensor([0.2], dtype=torch.float32, device="cuda")
    host = AdaptiveParamNoiseSpec(0.2, 0.0, 1.01)
    # desired 50 % above the distance: too close -> more noise; then 33 % below: too far -> less; compounding
    for desired in (1.5 * ref, 1.5 * ref, ref / 1.5, 1.5 * ref, ref / 1.5, ref / 1.5):
        d = adapt(ssc, a, b, desired, 1.01, sd)
        assert abs(d - ref) <= 1e-6 * ref, (d, ref)
        host.desired_action_stddev = desired
        before = host.current_stddev
        host.adapt(d)
        assert (host.current_stddev > before) == (desired > ref)
        assert float(sd.item()) == host.current_stddev, (desired, ref)


def test_adapt_tie_multiplies(ssc):
    """a - b = 0.25 everywhere: distance is exactly 0.25 = desired, and AdaptiveParamNoiseSpec.adapt multiplies on a tie"""
    hb = (np.arange(-64, 64) / 64.0).astype(np.float32)
    ha = (hb + np.float32(0.25)).astype(np.float32)
    assert np.all(ha.astype(np.float64) - hb.astype(np.float64) == 0.25)
    sd = torch.tensor([0.2], dtype=torch.float32, device="cuda")
    c = np.float32(1.01)
    a, b = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
    assert adapt(ssc, a, b, 0.25, 1.01, sd) == 0.25
    assert float(sd.item()) == float(np.float32(0.2) * c)
    assert adapt(ssc, a, b, 0.25, 1.01, sd) == 0.25            # two calls compound
    assert float(sd.item()) == float(np.float32(0.2) * c * c)
    assert adapt(ssc, a, b, float(np.nextafter(np.float32(0.25), np.float32(0))), 1.01, sd) == 0.25   # just above desired
    assert float(sd.item()) == float(np.float32(0.2) * c * c / c)


def make_agent(ssc, env_seed=1, **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    args = dict(batch_size=64, num_train_iterations=2, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32,
                lastLayerTanh=True, seed=7)
    args.update(kw)
    return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0", seed=env_seed), None, **args)


def chunk_bits(chunk):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (chunk.obs, chunk.act, chunk.rew, chunk.done, chunk.obs2)]


@pytest.mark.parametrize("precision,layer_norm", [("f32", False), ("bf16_mfma", False), ("f32", True)])
def test_perturbed_rollout_equals_plain_agent_with_the_perturbed_weights(ssc, precision, layer_norm):
    noisy = make_agent(ssc, layer_norm=layer_norm, param_noise_stddev=0.2)
    plain = make_agent(ssc, layer_norm=layer_norm)
    plain.set_weights({k: v.cpu() for k, v in noisy.perturbed_weights.items()})
    assert not torch.equal(noisy.perturbed_actor_flat, noisy.actor_flat)
    if layer_norm:                                              # beta / gamma travel unperturbed
        for k in ("ln1_b", "ln1_g", "ln2_b", "ln2_g"):
            assert torch.equal(noisy.perturbed_weights[k], noisy.weights[k])
        assert not torch.equal(noisy.perturbed_weights["b2"], noisy.weights["b2"])
    runs = []
    for policy in (noisy.as_policy(precision=precision, perturbed=True), plain.as_policy(precision=precision),
                   noisy.as_policy(precision=precision)):
        env = ssc.VecEnv("MountainCarContinuous-v0", 256, seed=11)
        runs.append(chunk_bits(env.rollout(8, policy)))
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not np.array_equal(runs[0][1], runs[2][1])           # ... and not what the unperturbed actor does


@pytest.mark.parametrize("normalize", [False, True])
def test_vec_loop_adapts_and_perturbs_on_device(ssc, gauss_err, normalize):
    from smartstartcontinuous_amd.agents import AdaptiveParamNoiseSpec
    CHUNKS = 3

    def run():
        agent = make_agent(ssc, param_noise_stddev=0.2, normalize_observations=normalize)
        assert agent.perturbed_generation == 0                  # set_weights perturbed the fresh copy
        env = ssc.VecEnv("MountainCarContinuous-v0", 256, seed=5)
        seen = []
        ssc.rl_train_vec_ddpg(env, agent, CHUNKS, chunk_steps=8, train_iters=2, seed=3,
                              on_chunk=lambda i, chunk, e: seen.append((agent.d_param_noise_distance.clone(),
                                                                        agent.d_param_noise_stddev.clone())))
        torch.cuda.synchronize()
        return agent, [(float(d.item()), float(s.item())) for d, s in seen]

    agent, seen = run()
    again, seen2 = run()
    assert seen == seen2 and len(seen) == CHUNKS
    for name in ("actor_flat", "perturbed_actor_flat", "d_param_noise_stddev"):
        assert np.array_equal(bits(getattr(agent, name)), bits(getattr(again, name))), name
    host = AdaptiveParamNoiseSpec(0.2, 0.2, 1.01)               # the host rule replayed on the recorded distances
    for distance, stddev in seen:
        assert np.isfinite(distance) and distance > 0
        host.adapt(distance)
        assert stddev == host.current_stddev
    assert agent.param_noise.current_stddev == seen[-1][1]
    # generation 0 at construction, 1 before chunk 0, then (adaptive, acting) = (2 + 2i, 3 + 2i) behind chunk i
    assert agent.perturbed_generation == 2 * CHUNKS + 1 and agent.param_noise_generation == 2 * CHUNKS + 2
    flat, pert = agent.actor_flat.cpu().numpy(), agent.perturbed_actor_flat.cpu().numpy()
    assert not np.array_equal(flat, pert)
    assert not np.array_equal(flat, make_agent(ssc, param_noise_stddev=0.2).actor_flat.cpu().numpy())   # the learner trained it
    assert_close_to_stream(pert, flat, seen[-1][1], agent.param_noise_seed, agent.perturbed_generation, (0, 0, 0, 0), gauss_err)
    # the adaptive copy drew the generation before
    assert_close_to_stream(agent.adaptive_actor_flat.cpu().numpy(), flat, seen[-2][1], agent.param_noise_seed,
                           agent.perturbed_generation - 1, (0, 0, 0, 0), gauss_err)


def test_scalar_agent_acts_with_the_perturbed_actor(ssc):
    agent = make_agent(ssc, param_noise_stddev=0.2, batch_size=16, num_train_iterations=1, num_steps_before_train=1)
    agent.decaying_ou_action_noise.epsilon = 0.0               # OU noise off: the action is the actor's
    obs = np.array([-0.5, 0.01])
    plain = np.clip(agent.actor(obs.astype(np.float32)[None, :])[0].cpu().numpy(), -1, 1)
    w = {k: v.cpu().numpy() for k, v in agent.perturbed_weights.items()}
    a0 = agent.get_action(obs)
    assert np.max(np.abs(a0 - np.clip(O.actor_forward(obs[None, :].astype(np.float32), **w)[0], -1, 1))) <= 1e-5
    assert abs(float(a0[0]) - float(plain[0])) > 1e-4
    assert np.array_equal(agent.get_action(obs), a0)           # the perturbation holds for the episode
    g = agent.perturbed_generation
    agent.start_new_episode(obs)                               # DDPG_editted.reset: a new perturbation
    assert agent.perturbed_generation == g + 1
    a1 = agent.get_action(obs)
    assert abs(float(a1[0]) - float(a0[0])) > 1e-6 and abs(float(a1[0]) - float(plain[0])) > 1e-6
    # train() adapts once per call as soon as the buffer holds a batch
    env = agent.env
    state = env.reset()
    assert agent.param_noise.current_stddev == float(np.float32(0.2))
    from smartstartcontinuous_amd.agents import AdaptiveParamNoiseSpec
    host, adaptions = AdaptiveParamNoiseSpec(0.2, 0.2, 1.01), 0
    for step in range(18):
        action = agent.get_action(state)
        new_state, reward, done, _info = env.step(action)
        before = agent.param_noise.current_stddev
        agent.observe(state, action, reward, new_state, done)
        state = new_state
        if step + 1 < 16:                                      # fewer records than a batch: train() returns early
            assert agent.param_noise.current_stddev == before == float(np.float32(0.2))
            continue
        host.adapt(float(agent.d_param_noise_distance.item()))  # the host rule on the distance train() just measured
        adaptions += 1
        assert agent.param_noise.current_stddev == host.current_stddev != before
    assert adaptions == 3                                       # 16, 17, 18 records: one adaption per train()
    agent.training_enabled = False                             # pi(apply_noise=False): the plain actor acts
    plain = np.clip(agent.actor(obs.astype(np.float32)[None, :])[0].cpu().numpy(), -1, 1)      # (the learner moved it)
    assert np.array_equal(agent.get_action(obs), agent.scale(agent.scale(plain)))
