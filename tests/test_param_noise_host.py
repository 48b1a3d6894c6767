"""Adaptive parameter-space noise without a GPU: the two entry points exist and check their arguments on the host, the
host restatement of AdaptiveParamNoiseSpec.adapt, an agent built without the keyword carries nothing new, and the loops
that do not support parameter noise refuse it before any device work."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from smartstartcontinuous_amd import _ffi
    return _ffi.lib()


def fake(n=1 << 20):
    """A non-NULL address that is never dereferenced: every call below fails its host-side checks first."""
    return ctypes.c_void_p(n)


def test_perturb_argument_checks(lib):
    from smartstartcontinuous_amd import _ffi
    E = _ffi.SSC_EINVAL
    ok = dict(n=100, src=fake(), dst=fake(2 << 20), sd=fake(3 << 20), s0=(0, 0), s1=(0, 0), seed=1, gen=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ssc_param_noise_perturb(a["n"], a["src"], a["dst"], a["sd"], a["s0"][0], a["s0"][1], a["s1"][0], a["s1"][1],
                                           a["seed"], a["gen"], None)
    for bad in (dict(n=-1), dict(src=None), dict(dst=None), dict(sd=None),
                dict(s0=(-1, 4)), dict(s0=(8, 4)), dict(s0=(90, 101)), dict(s1=(-2, -1)), dict(s1=(50, 40)), dict(s1=(0, 101)),
                dict(s0=(10, 20), s1=(19, 30)), dict(s0=(10, 20), s1=(0, 11)), dict(s0=(10, 20), s1=(12, 14)),
                dict(s0=(12, 14), s1=(10, 20)), dict(s0=(10, 20), s1=(10, 20)),
                dict(gen=1 << 56), dict(gen=(1 << 64) - 1)):
        assert call(**bad) == E, bad
        assert b"ssc_param_noise_perturb" in lib.ssc_last_error(), bad
    assert call(gen=1 << 56) == E and b"generation" in lib.ssc_last_error()
    assert call(s0=(10, 20), s1=(19, 30)) == E and b"overlap" in lib.ssc_last_error()
    # nothing to do: no launch, whatever the data pointers are
    assert lib.ssc_param_noise_perturb(0, None, None, fake(), 0, 0, 0, 0, 1, 0, None) == _ffi.SSC_OK
    assert lib.ssc_param_noise_perturb(0, None, None, None, 0, 0, 0, 0, 1, 0, None) == E


def test_adapt_argument_checks(lib):
    from smartstartcontinuous_amd import _ffi
    E = _ffi.SSC_EINVAL
    ok = dict(count=64, a=fake(), b=fake(2 << 20), desired=0.2, coef=1.01, sd=fake(3 << 20), dist=fake(4 << 20))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ssc_param_noise_adapt(a["count"], a["a"], a["b"], a["desired"], a["coef"], a["sd"], a["dist"], None)
    for bad in (dict(count=0), dict(count=-1), dict(count=4096 * _ffi.SSC_MAX_ACT + 1), dict(a=None), dict(b=None),
                dict(sd=None), dict(dist=None), dict(coef=1.0), dict(coef=0.5), dict(coef=-1.01), dict(coef=float("nan"))):
        assert call(**bad) == E, bad
        assert b"ssc_param_noise_adapt" in lib.ssc_last_error(), bad


def test_host_adapt_rule():
    """baselines 0.1.5 AdaptiveParamNoiseSpec.adapt: distance > desired divides, anything else -- the tie included --
    multiplies; in fp32 like the device scalar."""
    from smartstartcontinuous_amd.agents import AdaptiveParamNoiseSpec
    f = np.float32
    s = AdaptiveParamNoiseSpec(initial_stddev=0.2, desired_action_stddev=0.25, adoption_coefficient=1.01)
    assert s.current_stddev == float(f(0.2)) and s.get_stats() == {"param_noise_stddev": float(f(0.2))}
    s.adapt(0.3)                                                  # too far: less noise
    assert s.current_stddev == float(f(0.2) / f(1.01))
    s.adapt(0.1)                                                  # too close: more noise
    assert s.current_stddev == float(f(0.2) / f(1.01) * f(1.01))
    s.adapt(0.25)                                                 # the tie multiplies
    assert s.current_stddev == float(f(0.2) / f(1.01) * f(1.01) * f(1.01))
    up = AdaptiveParamNoiseSpec(0.1, 0.1, 1.5)
    for _ in range(3):
        up.adapt(0.0)
    assert up.current_stddev == float(f(0.1) * f(1.5) * f(1.5) * f(1.5))
    with pytest.raises(ValueError):
        AdaptiveParamNoiseSpec(0.1, 0.1, 1.0)


class StubEnv:
    def __init__(self):
        from smartstartcontinuous_amd.spaces import Box
        self.observation_space = Box([-1.2, -0.07], [0.6, 0.07])
        self.action_space = Box([-1.0], [1.0])


NEW_ATTRIBUTES = ("perturbed_actor_flat", "perturbed_weights", "adaptive_actor_flat", "d_param_noise_stddev",
                  "d_param_noise_distance", "param_noise_generation", "param_noise_seed", "perturbed_generation")


def test_default_agent_has_nothing_new():
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    agent = DDPG_Baselines_agent(StubEnv(), None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, device="cpu", seed=1)
    assert agent.param_noise is None
    for name in NEW_ATTRIBUTES:
        assert not hasattr(agent, name), name
    with pytest.raises(ValueError, match="param_noise_stddev"):
        agent.as_policy(perturbed=True)
    with pytest.raises(RuntimeError, match="param_noise_stddev"):
        agent.perturb_policy()
    assert agent.adapt_param_noise(np.zeros((4, 2), np.float32)) == 0.      # ddpg_editted.py:361-362
    agent.set_weights({k: v.clone() for k, v in agent.weights.items()})
    for name in NEW_ATTRIBUTES:
        assert not hasattr(agent, name), name


def test_agent_with_param_noise_owns_the_copies():
    """The buffers and their layout (host tensors here: nothing is launched on a cpu agent)."""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    agent = DDPG_Baselines_agent(StubEnv(), None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, device="cpu", seed=1,
                                 layer_norm=True, param_noise_stddev=0.2)
    pn = agent.param_noise
    assert pn.current_stddev == float(np.float32(0.2)) and pn.desired_action_stddev == 0.2 and pn.adoption_coefficient == 1.01
    n = agent.actor_flat.numel()
    assert n == 2 * 64 + 64 + 2 * 64 + 64 * 32 + 32 + 2 * 32 + 32 + 1
    assert agent.perturbed_actor_flat.numel() == n and agent.adaptive_actor_flat.numel() == n
    assert agent.perturbed_actor_flat.data_ptr() not in (agent.actor_flat.data_ptr(), agent.adaptive_actor_flat.data_ptr())
    assert list(agent.perturbed_weights) == list(agent.weights)
    for k, v in agent.weights.items():
        p = agent.perturbed_weights[k]
        assert p.shape == v.shape
        assert p.data_ptr() - agent.perturbed_actor_flat.data_ptr() == v.data_ptr() - agent.actor_flat.data_ptr()
    # [beta1 | gamma1] and [beta2 | gamma2] of [W1|b1|beta1|gamma1|W2|b2|beta2|gamma2|W3|b3]
    assert agent._pn_skip == (192, 320, 320 + 64 * 32 + 32, 320 + 64 * 32 + 32 + 64)
    other = DDPG_Baselines_agent(StubEnv(), None, device="cpu", seed=1, param_noise_stddev=0.1,
                                 param_noise_desired_action_stddev=0.3, param_noise_adoption_coefficient=1.05)
    assert other.param_noise.desired_action_stddev == 0.3 and other.param_noise.adoption_coefficient == 1.05
    assert other._pn_skip == (0, 0, 0, 0)


class NoEnv:                                        # touched only if the refusal came too late
    def __getattr__(self, name):
        raise AssertionError(f"env.{name} used before the refusal")


class StubAgent:
    param_noise = object()
    obs_rms = None


def test_unsupported_loops_refuse_param_noise():
    from smartstartcontinuous_amd.rl_train import rl_train_vec_ddpg, rl_train_vec_smartstart
    from smartstartcontinuous_amd.sharding import rl_train_sharded_ddpg
    with pytest.raises(NotImplementedError, match="param_noise"):
        rl_train_vec_ddpg(NoEnv(), StubAgent(), 2, 4, overlap=True)
    with pytest.raises(NotImplementedError, match="param_noise"):
        rl_train_sharded_ddpg(NoEnv(), StubAgent(), 2, 4, 0, 1)
    with pytest.raises(NotImplementedError, match="param_noise"):
        rl_train_vec_smartstart(NoEnv(), SimpleNamespace(agent=StubAgent()), 2, 4)
