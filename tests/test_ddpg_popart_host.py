"""Return normalisation / Pop-Art of the DDPG agent without a GPU: the constructor's four keyword combinations, the
return statistics and their fp32 derivation, the foreign-function table and the argument validation of
``ssc_ddpg_train_ws_popart`` before any device call."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lib():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    return _ffi.lib()


class StubEnv:
    def __init__(self):
        from smartstartcontinuous_amd.spaces import Box
        self.observation_space = Box([-1.2, -0.07], [0.6, 0.07])
        self.action_space = Box([-1.0], [1.0])


@pytest.mark.parametrize("normalize_returns,enable_popart", [(False, False), (True, False), (False, True), (True, True)])
def test_constructor_keyword_combinations(lib, normalize_returns, enable_popart):
    """both switches (Pop-Art: the conjunction of ddpg_editted.py:140, 291) give the agent ret_rms; one switch without the
    other stays refused, with the message tests/test_gpu_obs_rms.py::test_constructor_flags pins"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.obs_rms import ObsRms
    kw = dict(actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, device="cpu", seed=1,
              normalize_returns=normalize_returns, enable_popart=enable_popart)
    if normalize_returns != enable_popart:
        with pytest.raises(NotImplementedError, match="return normalisation / popart"):
            DDPG_Baselines_agent(StubEnv(), None, **kw)
        return
    agent = DDPG_Baselines_agent(StubEnv(), None, **kw)
    assert (agent.ret_rms is not None) == normalize_returns
    assert agent.popart == (normalize_returns and enable_popart)
    assert agent.get_param_dict()["normalize_returns"] == normalize_returns
    assert agent.get_param_dict()["enable_popart"] == enable_popart
    if normalize_returns:
        assert isinstance(agent.ret_rms, ObsRms) and agent.ret_rms.obs_dim == 1
        block = agent.ret_rms.block
        assert block.dtype == torch.float64 and block.tolist() == [0.0, 1e-2, 1e-2]
        mean, std = agent.ret_rms.mean_std()
        assert mean.tolist() == [0.0] and std.tolist() == [1.0]
        dm, ds = agent.ret_rms.mean_std_device()
        assert dm.dtype == ds.dtype == torch.float32 and dm.tolist() == [0.0] and ds.tolist() == [1.0]


def _f32_mean_std(block):
    """the derivation spelled out with numpy float32 scalars: one rounding per operation"""
    f = np.float32
    mean = f(block[0] / block[2])
    sq = f(block[1] / block[2])
    var = f(sq - f(mean * mean))
    return mean, f(np.sqrt(max(var, f(1e-2))))


@pytest.mark.parametrize("block,on_floor", [
    ([3.2, 0.66, 64.01], True),                   # variance 7.8e-3: under the floor
    ([-1.0, 0.5, 100.01], True),
    ([186.3, 2412.7, 64.01], False),              # mean 2.9, std 5.4
    ([57301.9, 3012345.6, 4096.01], False),       # a cancelling difference of two large fp32 numbers
    ([0.0, 1e-2, 1e-2], False),                   # the initial block: variance exactly 1
])
def test_mean_std_arithmetic(lib, block, on_floor):
    from smartstartcontinuous_amd.obs_rms import ObsRms
    rms = ObsRms(1, "cpu")
    rms.block.copy_(torch.tensor(block, dtype=torch.float64))
    want_mean, want_std = _f32_mean_std(np.asarray(block, np.float64))
    assert (want_std == np.float32(0.1)) == on_floor
    for mean, std in (rms.mean_std(), tuple(x.numpy() for x in rms.mean_std_device())):
        assert mean.dtype == np.float32 and std.dtype == np.float32
        assert mean.tobytes() == want_mean.tobytes() and std.tobytes() == want_std.tobytes()


def test_ffi_entry(lib):
    from smartstartcontinuous_amd import _ffi
    assert "ssc_ddpg_train_ws_popart" in _ffi._SIGNATURES and "ssc_ddpg_train_popart_workspace_bytes" in _ffi._SIGNATURES
    res, args = lib.ssc_ddpg_train_ws_popart.restype, lib.ssc_ddpg_train_ws_popart.argtypes
    assert res is ctypes.c_int and len(args) == 10
    assert args[6] is ctypes.c_size_t and args[8] is ctypes.c_void_p and args[9] is ctypes.c_void_p
    assert lib.ssc_ddpg_train_popart_workspace_bytes.restype is ctypes.c_size_t
    assert lib.ssc_version() == 108                        # additive: the ABI version does not move


def _desc(B=64, h=(64, 32), obs_dim=2):
    from smartstartcontinuous_amd import _ffi
    d = _ffi.DdpgDesc()
    d.obs_dim, d.act_dim, d.actor_h1, d.actor_h2, d.critic_h1, d.critic_h2 = obs_dim, 1, h[0], h[1], h[0], h[1]
    d.last_layer_tanh, d.batch_size = 1, B
    d.actor = d.critic = d.target_actor = d.target_critic = 0x1000
    d.adam_m_actor = d.adam_v_actor = d.adam_m_critic = d.adam_v_critic = d.adam_t = 0x1000
    d.gamma, d.tau, d.actor_lr, d.critic_lr, d.beta1, d.beta2, d.epsilon = 0.99, 0.001, 1e-3, 1e-3, 0.9, 0.999, 1e-8
    return d


def test_workspace_layout(lib):
    """[the plain step's workspace | y | partials | scalars], each part rounded up to 256 bytes"""
    up = lambda x: (x + 255) // 256 * 256
    for B, h in ((64, (64, 32)), (50, (64, 32)), (4096, (64, 32)), (256, (200, 100)), (1, (37, 19))):
        d = _desc(B, h)
        plain = lib.ssc_ddpg_train_workspace_bytes(ctypes.byref(d))
        want = up(plain) + up(4 * B) + up(16 * ((B + 15) // 16)) + 256
        assert lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d)) == want
    assert lib.ssc_ddpg_train_popart_workspace_bytes(None) == 256
    assert lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(_desc(0))) == 256
    assert lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(_desc(4097))) == 256


def test_argument_validation_before_any_device_call(lib):
    from smartstartcontinuous_amd import _ffi
    fake = lambda: ctypes.c_void_p(0x1000)     # never dereferenced: every case below is rejected on the host
    rv = _ffi.ReplayView(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 100)

    def call(d, ws_bytes=None, ws=True, ret=True, n_iters=1, replay=rv, idx=True):
        need = lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d))
        return lib.ssc_ddpg_train_ws_popart(ctypes.byref(d), None if replay is None else ctypes.byref(replay),
                                            fake() if idx else None, n_iters, None, fake() if ws else None,
                                            need if ws_bytes is None else ws_bytes, None, None, fake() if ret else None)

    def rejected(rc, word, code=_ffi.SSC_EINVAL):
        msg = lib.ssc_last_error()
        assert rc == code and word in msg, (rc, msg)

    d = _desc()
    need = lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d))
    rejected(call(d, ws_bytes=need - 1), b"ssc_ddpg_train_popart_workspace_bytes")
    rejected(call(d, ws=False), b"workspace")
    # the plain step's size is not enough
    rejected(call(d, ws_bytes=lib.ssc_ddpg_train_workspace_bytes(ctypes.byref(d))), b"workspace")
    rejected(call(d, replay=None), b"NULL")
    rejected(call(d, idx=False), b"replay")
    rejected(call(d, n_iters=-1), b"n_iters")
    assert call(d, n_iters=0) == _ffi.SSC_OK
    rejected(call(_desc(obs_dim=9)), b"out of range")
    rejected(call(_desc(h=(0, 32))), b"hidden")
    rejected(call(_desc(B=4097)), b"4097", _ffi.SSC_EUNSUPPORTED)
    d_null = _desc()
    d_null.target_critic = None
    rejected(call(d_null), b"parameter")
    # a NULL block is ssc_ddpg_train_ws_rms: its own checks and messages (here its workspace check)
    rejected(call(_desc(B=128, h=(200, 100)), ret=False, ws_bytes=16), b"ssc_ddpg_train_workspace_bytes")
    assert call(_desc(B=128, h=(200, 100)), ret=False, n_iters=0) == _ffi.SSC_OK
    # ... and a NULL block with the shipped shape takes the one-workgroup route, which a Pop-Art agent never does:
    # with a block, a 64-32 network at batch 64 needs the Pop-Art workspace
    rejected(call(_desc(), ws_bytes=0), b"workspace")


def test_loops_without_the_read_out_refuse(lib):
    """the sharded and the SmartStart loops read the raw critic: they refuse an agent with return statistics"""
    from smartstartcontinuous_amd import rl_train, sharding
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    agent = DDPG_Baselines_agent(StubEnv(), None, device="cpu", seed=1, normalize_returns=True, enable_popart=True)
    with pytest.raises(NotImplementedError, match="Pop-Art"):
        sharding.rl_train_sharded_ddpg(None, agent, 1, 1, 0, 1)

    class Smart:
        pass
    smart = Smart()
    smart.agent = agent
    with pytest.raises(NotImplementedError, match="Pop-Art"):
        rl_train.rl_train_vec_smartstart(None, smart, 1)
