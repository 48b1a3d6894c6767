"""The training diagnostics (``ssc_ddpg_stats`` / ``DDPG_Baselines_agent.get_stats``) without a GPU: argument validation
before any device call, the order of the statistics, and what ``get_stats`` hands back."""
import ctypes

import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lib():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    return _ffi.lib()


def fake():
    return ctypes.c_void_p(0x1000)     # never dereferenced: every case below is rejected on the host


def descs(obs_dim=2, act_dim=1, h=(64, 32), ch=(64, 32)):
    from smartstartcontinuous_amd import _ffi
    a, c = _ffi.ActorDesc(), _ffi.CriticDesc()
    a.obs_dim, a.h1, a.h2, a.act_dim = obs_dim, h[0], h[1], act_dim
    c.obs_dim, c.h1, c.h2, c.act_dim = obs_dim, ch[0], ch[1], act_dim
    for d in (a, c):
        d.W1 = d.b1 = d.W2 = d.b2 = d.W3 = d.b3 = 0x1000
    return a, c


def call(lib, a, c, p=None, m=64, obs=True, act=True, out=True, ws=True, ws_bytes=None, rms=None, sd=None):
    ref = lambda d: None if d is None else ctypes.byref(d)
    need = lib.ssc_ddpg_stats_workspace_bytes(m)
    return lib.ssc_ddpg_stats(ref(a), ref(c), ref(p), m, fake() if obs else None, fake() if act else None, rms, sd,
                              fake() if out else None, fake() if ws else None, need if ws_bytes is None else ws_bytes, None)


def test_workspace_bytes(lib):
    from smartstartcontinuous_amd import _ffi
    assert _ffi.SSC_DDPG_N_STATS == 11
    # (count, mean, M2) in f64 for four statistics per 16-row tile
    assert lib.ssc_ddpg_stats_workspace_bytes(1) == 4 * 3 * 8
    assert lib.ssc_ddpg_stats_workspace_bytes(16) == 4 * 3 * 8
    assert lib.ssc_ddpg_stats_workspace_bytes(17) == 2 * 4 * 3 * 8
    assert lib.ssc_ddpg_stats_workspace_bytes(4096) == 256 * 4 * 3 * 8
    assert lib.ssc_ddpg_stats_workspace_bytes(0) == 0 and lib.ssc_ddpg_stats_workspace_bytes(4097) == 0


def test_argument_validation_before_any_device_call(lib):
    from smartstartcontinuous_amd import _ffi
    E = _ffi.SSC_EINVAL
    a, c = descs()

    def rejected(rc, word):
        msg = lib.ssc_last_error()
        assert rc == E and word in msg, (rc, msg)

    rejected(call(lib, None, c), b"NULL")
    rejected(call(lib, a, None), b"NULL")
    rejected(call(lib, a, c, out=False), b"output")
    rejected(call(lib, a, c, m=0), b"m 0")
    rejected(call(lib, a, c, m=-3), b"m -3")
    rejected(call(lib, a, c, m=4097), b"4097")
    rejected(call(lib, a, c, obs=False), b"sample")
    rejected(call(lib, a, c, act=False), b"sample")
    rejected(call(lib, a, c, ws=False), b"workspace")
    rejected(call(lib, a, c, m=64, ws_bytes=4 * 4 * 3 * 8 - 1), b"workspace")
    _, c3 = descs(obs_dim=3)
    rejected(call(lib, a, c3), b"differ")
    _, c_a2 = descs(act_dim=2)
    rejected(call(lib, a, c_a2), b"differ")
    a9, c9 = descs(obs_dim=9)
    rejected(call(lib, a9, c9), b"out of range")
    a0, c0 = descs(act_dim=0)
    rejected(call(lib, a0, c0), b"out of range")
    az, _ = descs(h=(0, 32))
    rejected(call(lib, az, c), b"hidden")
    p_wide, _ = descs(h=(128, 32))
    rejected(call(lib, a, c, p=p_wide), b"perturbed")
    a_null, _ = descs()
    a_null.W2 = None
    rejected(call(lib, a_null, c), b"actor")
    _, c_ln = descs()
    c_ln.ln1_g = 0x1000                 # one LayerNorm pointer without the other three
    rejected(call(lib, a, c_ln), b"critic")
    p_null, _ = descs()
    p_null.b3 = None
    rejected(call(lib, a, c, p=p_null), b"perturbed")
    # a 16-row tile of this width does not fit the LDS: refused with the byte count, still before any device call
    a_big, c_big = descs(h=(2000, 600), ch=(2000, 600))
    assert call(lib, a_big, c_big) == _ffi.SSC_EUNSUPPORTED and b"LDS" in lib.ssc_last_error()


def test_stats_names_are_the_reference_order():
    """setup_stats (ddpg_editted.py:219-253) with normalize_observations and parameter noise on, normalize_returns off:
    obs_rms mean / std, then reference_Q, reference_actor_Q, reference_action, reference_perturbed_action (mean, std
    each); get_stats appends param_noise.get_stats()."""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    assert DDPG_Baselines_agent.STATS_NAMES == (
        "obs_rms_mean", "obs_rms_std",
        "reference_Q_mean", "reference_Q_std",
        "reference_actor_Q_mean", "reference_actor_Q_std",
        "reference_action_mean", "reference_action_std",
        "reference_perturbed_action_mean", "reference_perturbed_action_std",
        "param_noise_stddev")
    from smartstartcontinuous_amd import _ffi
    assert len(DDPG_Baselines_agent.STATS_NAMES) == _ffi.SSC_DDPG_N_STATS


def _bare_agent(block, param_noise):
    """get_stats over a given block: no device, no library call"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    agent = object.__new__(DDPG_Baselines_agent)
    agent.param_noise = param_noise
    agent.get_stats_device = lambda replay=None, out=None: torch.tensor(block, dtype=torch.float64)
    return agent


def test_get_stats_drops_nan_slots_and_merges_param_noise():
    from smartstartcontinuous_amd.agents import AdaptiveParamNoiseSpec, DDPG_Baselines_agent
    names = DDPG_Baselines_agent.STATS_NAMES
    nan = float("nan")
    # plain agent: no observation statistics, no parameter noise
    got = _bare_agent([nan, nan, 1.5, 0.25, -2.0, 0.5, 0.125, 0.75, nan, nan, nan], None).get_stats()
    assert list(got) == list(names[2:8])
    assert got == dict(zip(names[2:8], (1.5, 0.25, -2.0, 0.5, 0.125, 0.75)))
    assert all(isinstance(v, float) for v in got.values())
    # everything on: the reference order, the noise spec's own entry merged over slot 10 (ddpg_editted.py:355-356)
    spec = AdaptiveParamNoiseSpec(initial_stddev=0.2)
    full = [0.1, 1.1, 1.5, 0.25, -2.0, 0.5, 0.125, 0.75, 0.0, 0.5, 0.3]
    got = _bare_agent(full, spec).get_stats()
    assert list(got) == list(names)
    assert got["param_noise_stddev"] == spec.get_stats()["param_noise_stddev"] == spec.current_stddev != full[10]
    assert [got[k] for k in names[:10]] == full[:10]
    # observation statistics without parameter noise
    got = _bare_agent([0.1, 1.1, 1.5, 0.25, -2.0, 0.5, 0.125, 0.75, nan, nan, nan], None).get_stats()
    assert list(got) == list(names[:8])
