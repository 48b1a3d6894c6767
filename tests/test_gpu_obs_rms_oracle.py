"""normalize_observations against the oracle: the normalising forward kernels and learners against O.actor_forward /
O.critic_forward / O.ddpg_train_step fed x_hat in fp64, and teacher-forced normalising rollouts (the fused 64-32 policy,
ActorPolicy<ActorMfma> / <ActorMfmaLds> / <ActorF32>, MountainCar and Pendulum) through O.replay_rollout with an action
function that normalises first -- the tolerances of test_gpu_actor_pendulum.py / test_gpu_agents.py."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests.gpu_util import actor_weights, x_hat64 as _x_hat64

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL_ACT_F32 = 1e-5
TOL_ACT_BF16 = 2e-2
TOL_ACT_BF16_EMU = 1.5e-3
CLIP = 5.0


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _stats(obs_dim, seed):
    """Statistics with nonzero means, one component on the 0.1 std floor and the others above it."""
    from smartstartcontinuous_amd.obs_rms import ObsRms
    r = ObsRms(obs_dim)
    rng = np.random.default_rng(seed)
    mu, sd = ([-0.5, 0.0], [0.3, 0.05]) if obs_dim == 2 else ([0.2, -0.1, 0.5], [0.5, 0.5, 2.0])
    r.update_rows(rng.normal(mu, sd, size=(400, obs_dim)).astype(np.float32))
    return r


def _x_hat32(x, rms):
    mean, std = rms.mean_std()
    return np.clip((np.asarray(x, np.float32) - mean) / std, np.float32(-CLIP), np.float32(CLIP)).astype(np.float32)


def _agent(ssc, obs_dim, h, precision="f32", batch=64):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    env = ssc.make("MountainCarContinuous-v0" if obs_dim == 2 else "Pendulum-v0")
    return DDPG_Baselines_agent(env, None, actor_h1=h[0], actor_h2=h[1], critic_h1=h[0], critic_h2=h[1], lastLayerTanh=True,
                                precision=precision, seed=11, batch_size=batch, actor_lr=1e-3, critic_lr=1e-3, training=False)


def _np(d):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in d.items()}


@pytest.mark.parametrize("obs_dim,h,precision", [(2, (64, 32), "f32"), (3, (128, 64), "f32"), (2, (64, 32), "bf16_mfma"),
                                                 (3, (200, 100), "bf16_mfma")])
def test_forward_rms_vs_oracle(ssc, obs_dim, h, precision):
    agent = _agent(ssc, obs_dim, h, precision)
    rms = _stats(obs_dim, 3)
    rng = np.random.default_rng(4)
    aw, cw = _np(agent.weights), _np(agent.critic_weights)
    for m in (1, 7, 1000):
        x = rng.uniform(-1.5, 1.5, size=(m, obs_dim)).astype(np.float32)
        got = agent.actor(x, obs_rms=rms).cpu().numpy()
        ref = O.actor_forward(_x_hat64(x, rms), **aw, last_layer_tanh=True, obs_clip=CLIP)
        if precision == "f32":
            assert np.max(np.abs(got - ref)) <= TOL_ACT_F32, m
        else:
            assert np.max(np.abs(got - ref)) <= TOL_ACT_BF16, m
            emu = O.actor_forward_bf16emu(_x_hat32(x, rms), **aw, last_layer_tanh=True, obs_clip=CLIP)
            assert np.max(np.abs(got - emu)) <= TOL_ACT_BF16_EMU, m
        act = rng.uniform(-1, 1, size=(m, 1)).astype(np.float32)
        q = agent.critic(x, act, obs_rms=rms).cpu().numpy()
        ref_q = O.critic_forward(_x_hat64(x, rms), act, **cw, last_layer_tanh=True, obs_clip=CLIP)[:, 0]
        assert np.max(np.abs(q - ref_q)) <= 1e-5 * max(1.0, np.abs(ref_q).max()), m


@pytest.mark.parametrize("h,batch", [((64, 32), 64), ((64, 32), 128), ((128, 64), 64)])
def test_train_on_rms_vs_oracle(ssc, h, batch):
    """One-workgroup 64-32, tiled 64-32 and multi-workgroup 128-64 learners on RAW replay rows with the statistics, against
    the fp64 train step on x_hat."""
    agent = _agent(ssc, 2, h, batch=batch)
    rms = _stats(2, 5)
    rng = np.random.default_rng(8)
    cap, n_iters = 2000, 6
    s = rng.uniform(-1.2, 0.6, (cap, 2)).astype(np.float32)
    s[:, 1] = rng.uniform(-0.07, 0.07, cap)
    a = rng.uniform(-1, 1, (cap, 1)).astype(np.float32)
    r = (rng.normal(size=cap) * 0.5).astype(np.float32)
    t = rng.random(cap) < 0.1
    s2 = (s + rng.normal(size=(cap, 2)) * 0.01).astype(np.float32)
    idx = np.stack([rng.permutation(cap)[:batch] for _ in range(n_iters)]).astype(np.int32)
    o_a, o_c = _np(agent.weights), _np(agent.critic_weights)
    o_ta = O.unflatten_params(agent.target_actor_flat.cpu().numpy().astype(np.float64), o_a)
    o_tc = O.unflatten_params(agent.target_critic_flat.cpu().numpy().astype(np.float64), o_c)
    na, nc = agent.actor_flat.numel(), agent.critic_flat.numel()
    adam = dict(m_actor=np.zeros(na), v_actor=np.zeros(na), t_actor=0, m_critic=np.zeros(nc), v_critic=np.zeros(nc), t_critic=0)
    sh, s2h = _x_hat64(s, rms), _x_hat64(s2, rms)
    ref_losses = []
    for it in range(n_iters):
        bi = idx[it]
        o_a, o_c, o_ta, o_tc, adam, cl, al = O.ddpg_train_step(
            o_a, o_c, o_ta, o_tc, adam, (sh[bi], a[bi], r[bi], t[bi], s2h[bi]), gamma=0.99, tau=0.001,
            actor_lr=1e-3, critic_lr=1e-3, last_layer_tanh=True, obs_clip=CLIP)
        ref_losses.append((cl, al))
    dev = lambda x, dt: torch.as_tensor(x, dtype=dt, device="cuda").contiguous()
    losses = agent.train_on(dev(s, torch.float32), dev(a, torch.float32), dev(r, torch.float32), dev(t, torch.uint8),
                            dev(s2, torch.float32), dev(idx, torch.int32), n_iters, obs_rms=rms)
    torch.cuda.synchronize()
    assert np.allclose(losses.cpu().numpy(), np.asarray(ref_losses), rtol=2e-4, atol=1e-6)
    tol = 5e-6
    assert np.max(np.abs(agent.actor_flat.cpu().numpy() - O.flatten_params(o_a))) <= tol
    assert np.max(np.abs(agent.critic_flat.cpu().numpy() - O.flatten_params(o_c))) <= tol
    assert np.max(np.abs(agent.target_actor_flat.cpu().numpy() - O.flatten_params(o_ta))) <= tol
    assert np.max(np.abs(agent.target_critic_flat.cpu().numpy() - O.flatten_params(o_tc))) <= tol


class NormalisingPolicy:
    """action_fn for O.replay_rollout: the oracle DDPG policy on x_hat (fp32, as the kernels form it)."""

    def __init__(self, inner, rms):
        self.inner, self.rms = inner, rms

    def __call__(self, k, t, obs, prev_done):
        return self.inner(k, t, _x_hat32(obs, self.rms), prev_done)


def _log(chunk):
    return dict(obs=chunk.obs.cpu().numpy(), act=chunk.act.cpu().numpy(), rew=chunk.rew.cpu().numpy(),
                done=chunk.done.cpu().numpy(), obs2=chunk.obs2.cpu().numpy())


@pytest.mark.parametrize("env_id,h,precision,eps", [
    ("MountainCarContinuous-v0", (64, 32), "bf16_mfma", 1.0),    # ActorPolicyFused<true, NORM>: the corrected reciprocal
    ("MountainCarContinuous-v0", (64, 32), "bf16_mfma", 0.0),    # no noise: ActorPolicy<ActorMfma<2, 2, 1>>
    ("MountainCarContinuous-v0", (128, 64), "bf16_mfma", 1.0),   # ActorPolicy<ActorMfma<2, 4, 2>>
    ("MountainCarContinuous-v0", (64, 32), "f32", 1.0),          # ActorPolicy<ActorF32<2, 64, 32>>
    ("Pendulum-v0", (64, 32), "bf16_mfma", 1.0),                 # ActorPolicy<ActorMfma<3, 2, 1>> (bounds +-2)
    ("Pendulum-v0", (200, 100), "bf16_mfma", 1.0),               # ActorPolicy<ActorMfmaLds<3, 7, 4>>
])
def test_rollout_rms_teacher_forced(ssc, env_id, h, precision, eps):
    n, K, seed, id0 = 700, 24, 31, 5
    pend = env_id.startswith("Pendulum")
    obs_dim = 3 if pend else 2
    w = actor_weights(obs_dim, h[0], h[1], seed=h[0] + obs_dim, w3_scale=0.5)
    rms = _stats(obs_dim, 9)
    env = ssc.VecEnv(env_id, n, seed=seed, env_id0=id0)
    obs0 = env.reset().cpu().numpy()
    start = 190 if pend else 990
    env.steps.fill_(start)         # time-limit reset (and OU reset) inside the window
    env.t = 5
    pol = ssc.ActorPolicy({k: torch.as_tensor(v) for k, v in w.items()}, precision=precision, obs_clip=CLIP, ou_epsilon=eps,
                          d_obs_rms=rms.block)
    chunk = env.rollout(K, pol)
    torch.cuda.synchronize()
    low, high = (-2.0, 2.0) if pend else (-1.0, 1.0)
    kind, tmax = ("pend", 200) if pend else ("mc", 999)
    mk = lambda bf16: NormalisingPolicy(O.OracleDDPGPolicy(w, seed, id0, n, epsilon=eps, bf16=bf16, low=low, high=high,
                                                           obs_clip=CLIP), rms)
    res = O.replay_rollout(kind, _log(chunk), seed, id0, 5, tmax, obs0, np.full(n, start), mk(False))
    assert res["start_max_err"] == 0 and res["continuity_mismatch"] == 0 and res["done_mismatch"] == 0, res
    scale = (high - low) / 2
    if precision == "f32":
        assert res["max_dact"] <= 2e-5 * scale, res
        return
    assert res["max_dact"] <= TOL_ACT_BF16 * scale, res
    res = O.replay_rollout(kind, _log(chunk), seed, id0, 5, tmax, obs0, np.full(n, start), mk(True))
    fused = not pend and h == (64, 32) and eps > 0
    if fused:   # the corrected reciprocal at the emulation tolerance of the plain fused policy
        assert res["max_dact"] <= TOL_ACT_BF16_EMU, res
        return
    # the other MFMA policies as in test_rollout_actor_wide_shapes_teacher_forced -- or as close as the PLAIN bf16 forward
    # kernel of the same network comes to the emulation on the same inputs: normalised Pendulum inputs reach the +-5 clip
    # in every component (the raw ones stay within |cos|, |sin| <= 1), and larger layer-1 sums put more hidden activations
    # on bf16 rounding boundaries
    from tests.test_gpu_actor_pendulum import _actor_forward_gpu
    xh = _x_hat32(chunk.obs.cpu().numpy().reshape(obs_dim, -1).T, rms)
    plain = _actor_forward_gpu(ssc, w, xh, ssc._ffi.SSC_PREC_BF16_MFMA)
    plain_err = float(np.max(np.abs(plain - O.actor_forward_bf16emu(xh, **w, last_layer_tanh=True, obs_clip=CLIP))))
    assert res["max_dact"] <= max(TOL_ACT_BF16_EMU, plain_err) * scale * 2 + 1e-6, (res["max_dact"], plain_err)
