"""normalize_observations without a GPU: the fp32 derivation of mean / std from the RunningMeanStd block, the argument
checks of the new entry points, and the sharded loop's refusal of a normalising agent."""
import ctypes

import numpy as np
import pytest


def restated_mean_std(sum_, sumsq, count):
    """baselines 0.1.5 common/mpi_running_mean_std.RunningMeanStd, as TF evaluates it:
        mean = to_float(sum / count)
        std = sqrt(maximum(to_float(sumsq / count) - square(mean), 1e-2))
    every fp32 operation rounded on its own."""
    mean = np.float32(np.float64(sum_) / np.float64(count))
    sq = np.float32(np.float64(sumsq) / np.float64(count))
    m2 = np.float32(mean * mean)
    var = np.float32(sq - m2)
    return mean, np.float32(np.sqrt(np.float32(max(var, np.float32(1e-2)))))


def test_mean_std_matches_restatement():
    from smartstartcontinuous_amd.obs_rms import mean_std_f32, rms_initial
    rng = np.random.default_rng(5)
    for d in (1, 2, 3, 8):
        b = rms_initial(d)
        m, s = mean_std_f32(b)
        assert np.all(m == 0) and np.all(s == np.float32(1.0))     # sumsq / count = 1: std 1 before any update
        for _ in range(50):
            x = rng.normal(rng.normal(size=d) * 3, rng.uniform(0.01, 5, size=d), size=(int(rng.integers(1, 500)), d))
            b[:d] += x.sum(0)
            b[d:2 * d] += (x * x).sum(0)
            b[2 * d] += len(x)
            m, s = mean_std_f32(b)
            for c in range(d):
                rm, rs = restated_mean_std(b[c], b[d + c], b[2 * d])
                assert m[c] == rm and s[c] == rs, (d, c)


def test_mean_std_no_fused_multiply_add():
    """Blocks where fma(-mean, mean, sq) rounds differently from sq - f32(mean * mean), down to the last bit of std: the
    helper must give the separately rounded result."""
    from smartstartcontinuous_amd.obs_rms import mean_std_f32
    rng = np.random.default_rng(11)
    found = 0
    for _ in range(20000):
        mean = np.float32(rng.uniform(0.5, 4.0))
        sq = np.float32(np.float64(mean) * np.float64(mean) + rng.uniform(0.02, 0.5))
        fused = np.float32(np.float64(sq) - np.float64(mean) * np.float64(mean))   # one rounding: what an FMA gives
        plain = np.float32(sq - np.float32(mean * mean))
        if np.float32(np.sqrt(fused)) == np.float32(np.sqrt(plain)):
            continue
        block = np.array([np.float64(mean), np.float64(sq), 1.0])                  # count 1: the f32 casts are exact
        m, s = mean_std_f32(block)
        assert m[0] == mean
        assert s[0] == np.float32(np.sqrt(plain)) and s[0] != np.float32(np.sqrt(fused))
        found += 1
        if found >= 5:
            break
    assert found >= 5


def test_normalize_clips():
    from smartstartcontinuous_amd.obs_rms import normalize_f32
    block = np.array([0.0, 0.0, 1e-2 * 1e-4, 1e-2 * 1e-4, 1e-2])          # std floored at 0.1
    x = np.array([[1.0, -0.2], [0.05, 0.0]], np.float32)
    xh = normalize_f32(x, block, 5.0)
    assert xh.dtype == np.float32
    assert np.array_equal(xh, np.array([[5.0, -2.0], [np.float32(0.05) / np.float32(0.1), 0.0]], np.float32))


@pytest.fixture(scope="module")
def lib():
    from smartstartcontinuous_amd import _ffi
    return _ffi.lib()


def fake(n=1 << 20):
    """A non-NULL address that is never dereferenced: every call below fails its host-side checks first."""
    return ctypes.c_void_p(n)


def test_update_argument_checks(lib):
    from smartstartcontinuous_amd import _ffi
    ws_bytes = lib.ssc_obs_rms_update_workspace_bytes(2)
    assert ws_bytes > 0 and lib.ssc_obs_rms_update_workspace_bytes(0) == 0 and lib.ssc_obs_rms_update_workspace_bytes(9) == 0
    log = _ffi.TransitionLog()
    log.obs[0], log.obs[1] = 1 << 20, 1 << 21
    ok = dict(obs_dim=2, k0=0, K=4, n=100, rms=fake(), ws=fake(), ws_bytes=ws_bytes)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ssc_obs_rms_update(a["obs_dim"], ctypes.byref(log), a["k0"], a["K"], a["n"], a["rms"], a["ws"],
                                      a["ws_bytes"], None)
    for bad in (dict(obs_dim=0), dict(obs_dim=4), dict(rms=None), dict(K=0), dict(k0=4), dict(k0=5), dict(k0=-1),
                dict(n=0), dict(ws=None), dict(ws_bytes=ws_bytes - 1)):
        assert call(**bad) == _ffi.SSC_EINVAL, bad
    assert lib.ssc_obs_rms_update(2, None, 0, 4, 100, fake(), fake(), ws_bytes, None) == _ffi.SSC_EINVAL
    log.obs[1] = None
    assert call() == _ffi.SSC_EINVAL
    log.obs[1] = 1 << 21
    log.row_stride = 50                                                        # < n
    assert call() == _ffi.SSC_EINVAL

    ws8 = lib.ssc_obs_rms_update_workspace_bytes(8)
    rows = lambda d, m, x, r, w, wb: lib.ssc_obs_rms_update_rows(d, m, x, r, w, wb, None)
    assert rows(0, 1, fake(), fake(), fake(), ws8) == _ffi.SSC_EINVAL
    assert rows(9, 1, fake(), fake(), fake(), ws8) == _ffi.SSC_EINVAL
    assert rows(8, -1, fake(), fake(), fake(), ws8) == _ffi.SSC_EINVAL
    assert rows(8, 1, fake(), None, fake(), ws8) == _ffi.SSC_EINVAL
    assert rows(8, 1, fake(), fake(), fake(), ws8 - 8) == _ffi.SSC_EINVAL
    assert rows(8, 1, None, fake(), fake(), ws8) == _ffi.SSC_EINVAL
    assert rows(8, 0, None, fake(), fake(), ws8) == _ffi.SSC_OK            # nothing to add


def test_rms_variants_keep_the_plain_checks(lib):
    """The *_rms entry points validate like their plain neighbours (NULL descriptors, dims out of range)."""
    from smartstartcontinuous_amd import _ffi
    assert lib.ssc_actor_forward_rms(None, 4, fake(), fake(), None, fake()) == _ffi.SSC_EINVAL
    a = _ffi.ActorDesc()
    a.obs_dim, a.h1, a.h2, a.act_dim = 9, 64, 32, 1
    assert lib.ssc_actor_forward_rms(ctypes.byref(a), 4, fake(), fake(), None, fake()) == _ffi.SSC_EINVAL
    assert lib.ssc_critic_forward_rms(None, 4, fake(), fake(), fake(), None, fake()) == _ffi.SSC_EINVAL
    c = _ffi.CriticDesc()
    c.obs_dim, c.h1, c.h2, c.act_dim = 0, 64, 32, 1
    assert lib.ssc_critic_forward_rms(ctypes.byref(c), 4, fake(), fake(), fake(), None, fake()) == _ffi.SSC_EINVAL
    st = _ffi.RolloutState()
    assert lib.ssc_rollout_rms(None, None, 4, 4, ctypes.byref(st), None, None, None, 0, 0, 0, None, fake()) == _ffi.SSC_EINVAL
    d = _ffi.DdpgDesc()
    d.obs_dim, d.act_dim, d.batch_size = 2, 1, 64
    d.actor_h1 = d.actor_h2 = d.critic_h1 = d.critic_h2 = 0
    rv = _ffi.ReplayView()
    assert lib.ssc_ddpg_train_ws_rms(ctypes.byref(d), ctypes.byref(rv), fake(), 1, fake(), fake(), 1 << 20, None,
                                     fake()) == _ffi.SSC_EINVAL
    assert lib.ssc_ddpg_train_ws_rms(None, ctypes.byref(rv), fake(), 1, fake(), fake(), 1 << 20, None, fake()) == _ffi.SSC_EINVAL


def test_sharded_loop_refuses_a_normalising_agent():
    from smartstartcontinuous_amd.sharding import rl_train_sharded_ddpg

    class StubAgent:
        obs_rms = object()

    class NoEnv:                                    # touched only if the refusal came too late
        def __getattr__(self, name):
            raise AssertionError(f"env.{name} used before the refusal")
    with pytest.raises(NotImplementedError, match="normalize_observations"):
        rl_train_sharded_ddpg(NoEnv(), StubAgent(), 2, 4, 0, 1)
