"""Five kernels restate the index-order fp32 network forward: ``actor_generic_kernel`` / ``actor_row_kernel``
(``ssc_actor_forward``, m > 32 / m <= 32), ``critic_kernel`` (``ssc_critic_forward``), and ``net_rows`` in
``ddpg_stats_rows_kernel`` (``ssc_ddpg_stats``) and ``ddpg_eval_kernel`` (``ssc_ddpg_eval_rollout``).  DESIGN 4.7c / 4.7d promise that
every unit is the same chain of fused multiply-adds whatever the tiling, so the entry points agree TO THE BIT: every comparison
below is equality, none carries a tolerance."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests.test_gpu_ddpg_stats import CLIP, Device, launch, make_net, oracle_kw
from tests.test_gpu_ddpg_eval import MC, nets, run, stats_block

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def actor_fwd(actor, obs, rms=None):
    """``ssc_actor_forward[_rms]`` of a ``Device`` actor on a [m, obs_dim] cuda tensor -> [m, act_dim] cuda tensor"""
    from smartstartcontinuous_amd import _ffi
    out = torch.empty((obs.shape[0], actor.desc.act_dim), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().ssc_actor_forward_rms(ctypes.byref(actor.desc), obs.shape[0], _ffi.ptr(obs), _ffi.ptr(out), _stream(),
                                                _ffi.ptr(rms)))
    return out


def critic_fwd(critic, obs, act, rms=None):
    from smartstartcontinuous_amd import _ffi
    q = torch.empty(obs.shape[0], dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().ssc_critic_forward_rms(ctypes.byref(critic.desc), obs.shape[0], _ffi.ptr(obs), _ffi.ptr(act), _ffi.ptr(q),
                                                 _stream(), _ffi.ptr(rms)))
    return q


def sample(rng, m, od, block):
    """[m, od] observations with components beyond the +-5 clip (after the normalisation when ``block`` is given)"""
    from smartstartcontinuous_amd import obs_rms as R
    if block is None:
        obs = rng.uniform(-1.5, 1.5, size=(m, od)).astype(np.float32)
        obs[::5] *= 5.0
        x = obs
    else:
        mean, std = R.mean_std_f32(block)
        obs = (mean + std * rng.uniform(-7.5, 7.5, size=(m, od))).astype(np.float32)
        obs[0, 0] = mean[0] + 7.0 * std[0]
        x = R.normalize_f32(obs, block, CLIP)
    assert np.abs(x[0]).max() >= CLIP       # row 0 (the m = 1 sample) meets the clip
    return torch.as_tensor(obs).cuda()


# (h1, h2), LayerNorm, lastLayerTanh, statistics block, obs_dim, act_dim
ROW_GENERIC_CASES = [((24, 12), True, False, True, 3, 3),
                     ((24, 12), True, True, False, 2, 1),
                     ((400, 300), False, True, False, 2, 1)]      # 400 * 256 B = 100 KB: the > 64 KB dynamic-LDS launch


def row_and_generic_agree(case):
    """rows 0..19 of an m = 20 call (one 256-thread block per row) against the same rows of an m = 100 call (one lane per row)"""
    (h1, h2), ln, tanh, with_rms, od, ad = case
    rng = np.random.default_rng(7 + h1)
    actor = Device(make_net(rng, od, h1, 0, h2, ad, ln, 0.25, 0.0), "actor", od, ad, tanh)
    block = stats_block(rng, od) if with_rms else None
    rms = torch.as_tensor(block).cuda() if with_rms else None
    obs = sample(rng, 100, od, block)
    many, few = actor_fwd(actor, obs, rms), actor_fwd(actor, obs[:20].contiguous(), rms)
    torch.cuda.synchronize()
    assert torch.isfinite(many).all() and many.std() > 1e-3
    assert torch.equal(few.view(torch.int32), many[:20].view(torch.int32)), case


def test_critic_forward_wide_network(ssc):
    """400-300 without LayerNorm: (400 + 1) * 256 B of dynamic LDS, beyond the 64 KB a launch gets unasked.  Its output
    against the fp64 oracle on the same weights and the clipped observations, to the tolerance
    tests/test_gpu_agents.py::test_critic_kde_ucb_kernels holds its 64-32 and 200-100 critics to."""
    from smartstartcontinuous_amd import _ffi
    rng = np.random.default_rng(3)
    w = make_net(rng, 2, 400, 1, 300, 1, False, 1.5, 20.0)
    critic = Device(w, "critic", 2, 1, True)
    obs = sample(rng, 100, 2, None)
    act = torch.as_tensor(rng.uniform(-1, 1, size=(100, 1)).astype(np.float32)).cuda()
    q = torch.full((100,), float("nan"), dtype=torch.float32, device="cuda")
    rc = _ffi.lib().ssc_critic_forward(ctypes.byref(critic.desc), 100, _ffi.ptr(obs), _ffi.ptr(act), _ffi.ptr(q), _stream())
    torch.cuda.synchronize()
    assert rc == _ffi.SSC_OK and torch.isfinite(q).all() and q.std() > 1e-3
    o = obs.cpu().numpy()
    assert np.abs(o).max() > CLIP                  # the clip is part of what is compared
    ref = O.critic_forward(o, act.cpu().numpy(), **oracle_kw(w), last_layer_tanh=True, obs_clip=CLIP)[:, 0]
    err = float(np.max(np.abs(q.cpu().numpy() - ref)))
    print("critic 400-300: max |q - ref| = %.2e, |ref|max = %.2f" % (err, np.abs(ref).max()))
    assert err <= 1e-5 * max(1.0, np.abs(ref).max())


STATS_NETS = {"64-32": ((64, 32), False, False), "24-12-ln-rms": ((24, 12), True, True)}


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("net", list(STATS_NETS))
def test_stats_are_the_forward_kernels_values(ssc, net, m):
    """m = 1: each mean slot IS the forward kernels' float, each std slot exactly 0.  m = 5 (one tile): each mean slot is the
    left-to-right f64 sum of the forward kernels' floats over the count, as ddpg_stats_rows_kernel forms it."""
    (h1, h2), ln, with_rms = STATS_NETS[net]
    od, ad = 2, 1
    rng = np.random.default_rng(40 + h1)
    aw = make_net(rng, od, h1, 0, h2, ad, ln, 0.25, 0.0)
    pw = {k: (v + (0.2 * rng.normal(size=v.shape)).astype(np.float32) if not k.startswith("ln") else v) for k, v in aw.items()}
    actor, pert = Device(aw, "actor", od, ad, True), Device(pw, "actor", od, ad, True)
    critic = Device(make_net(rng, od, h1, ad, h2, 1, ln, 1.5, 20.0), "critic", od, ad, True)
    block = stats_block(rng, od) if with_rms else None
    rms = torch.as_tensor(block).cuda() if with_rms else None
    obs = sample(rng, 5, od, block)[:m].contiguous()
    act = torch.as_tensor(rng.uniform(-1, 1, size=(m, ad)).astype(np.float32)).cuda()
    out = launch(ssc, actor, critic, pert, obs, act, rms=rms)
    pi, pp = actor_fwd(actor, obs, rms), actor_fwd(pert, obs, rms)
    streams = [critic_fwd(critic, obs, act, rms), critic_fwd(critic, obs, pi, rms), pi, pp]
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert not torch.equal(pi, pp)
    for s, values in enumerate(streams):
        total = 0.0
        for v in values.cpu().numpy().reshape(-1):
            total += float(v)
        assert out[2 + 2 * s] == total / m, (s, out[2 + 2 * s], total / m)
        if m == 1:
            assert out[3 + 2 * s] == 0.0, (s, out[3 + 2 * s])


@pytest.mark.parametrize("global_weights", [False, True])
@pytest.mark.parametrize("with_rms", [False, True])
@pytest.mark.parametrize("hidden", [(64, 32), (24, 12)])      # ssc_actor_forward: actor_f32_kernel / actor_generic_kernel
def test_eval_rollout_steps_are_the_forward_kernels_values(ssc, monkeypatch, hidden, with_rms, global_weights):
    """MountainCar's action range is [-1, 1]: where |pi| < 1 the logged action is the raw actor output.  17 envs (the second
    workgroup holds one), 5 steps: log.act = ssc_actor_forward(log.obs) and q = ssc_critic_forward(log.obs, log.act).
    With 24-12 the 85 logged rows run actor_generic_kernel: the 16 x 16 tiling against the 64 x 1 one for both networks."""
    n, K = 17, 5
    rng = np.random.default_rng(9)
    _, _, actor, critic = nets(12, 2, hidden, hidden)
    rms = torch.as_tensor(stats_block(rng, 2)).cuda() if with_rms else None
    if global_weights:
        monkeypatch.setenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", "1")
    else:
        monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)
    env = ssc.VecEnv(MC, n, seed=5)
    env.reset()
    assert float(env.action_space.low[0]) == -1.0 and float(env.action_space.high[0]) == 1.0
    _, chunk, q = run(ssc, env, actor, critic, K, rms=rms)
    monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)
    obs = chunk.obs.permute(1, 2, 0).reshape(K * n, 2).contiguous()
    pi = actor_fwd(actor, obs, rms)
    q_fwd = critic_fwd(critic, obs, pi, rms)
    torch.cuda.synchronize()
    assert pi.abs().max() < 1.0 and pi.std() > 1e-3     # W3 is small: no output reaches the action bound
    assert torch.equal(chunk.act.reshape(K * n).view(torch.int32), pi.reshape(K * n).view(torch.int32))
    assert torch.equal(q.reshape(K * n).view(torch.int32), q_fwd.view(torch.int32))
