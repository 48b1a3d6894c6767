"""``ssc_ddpg_eval_rollout`` on the GPU: teacher-forced against the fp64 oracle of a noise-free policy (``O.replay_rollout``
with ``O.OracleDDPGPolicy(epsilon=0)``, Q from ``O.critic_forward(x, O.actor_forward(x))`` on the logged observations), the
f64 block against a numpy restatement of the kernel's own trace (tests/eval_cases.py), the reduction on its own,
composition over chunks and shards, and the argument checks.

Tolerances: the project's own for fp32 actor rollouts -- action 2e-5 * (high - low) / 2, MountainCar
obs2 [2.4e-7, 1e-8], Pendulum 3e-6, reward 1e-6 relative (Pendulum 2e-5), resets exact (Pendulum 2e-6); Q per element
1e-5 * max(1, max |Q|) plus twice what the actor's own 1e-5 can move Q by, measured on the oracle alone as
tests/test_gpu_ddpg_stats.py::build_case does."""
import ctypes
import re

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import eval_cases as E
from tests.test_gpu_ddpg_stats import CLIP, TOL_ACT, Device, make_net, oracle_kw

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MC, PEND = "MountainCarContinuous-v0", "Pendulum-v0"


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def nets(seed, obs_dim, actor_h, critic_h, ln=False, tanh=True):
    """(actor weights, critic weights, Device actor, Device critic); the critic with w3_scale = 1.5, b3 = 20: Q of O(10)"""
    rng = np.random.default_rng(seed)
    aw = make_net(rng, obs_dim, actor_h[0], 0, actor_h[1], 1, ln, 0.25, 0.0)
    cw = make_net(rng, obs_dim, critic_h[0], 1, critic_h[1], 1, ln, 1.5, 20.0)
    return aw, cw, Device(aw, "actor", obs_dim, 1, tanh), Device(cw, "critic", obs_dim, 1, tanh)


def state_of(env):
    return {k: getattr(env, k).clone() for k in ("s0", "s1", "steps", "ep_ret")}


def set_state(env, st):
    for k, v in st.items():
        getattr(env, k).copy_(v)


def call(env, actor, critic, K, rms=None, chunk=None, q=None, zero_returns=1, out=None, raw=False, over=None):
    """the C entry point on ``env``'s state; ``over`` replaces single arguments (the error tests); -> return code"""
    from smartstartcontinuous_amd import _ffi
    lib = _ffi.lib()
    n = env.n
    st = _ffi.RolloutState(env.s0.data_ptr(), env.s1.data_ptr(), env.steps.data_ptr(), env.ep_ret.data_ptr(), None)
    log_s = chunk.as_struct() if chunk is not None else None
    ws = torch.empty(int(lib.ssc_ddpg_eval_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    a = dict(p=ctypes.byref(env.params), actor=ctypes.byref(actor.desc), critic=ctypes.byref(critic.desc),
             low=float(env.action_space.low[0]), high=float(env.action_space.high[0]), n=n, K=K, state=ctypes.byref(st),
             rms=_ffi.ptr(rms), log=ctypes.byref(log_s) if log_s is not None else None, q=_ffi.ptr(q), zero=zero_returns,
             out=_ffi.ptr(out), ws=_ffi.ptr(ws), ws_bytes=ws.numel(), seed=env._seed, id0=env.env_id0, step0=env.t,
             stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    a.update(over or {})
    rc = lib.ssc_ddpg_eval_rollout(*a.values())
    if raw:
        return rc
    _ffi.check(rc)
    env.t += K
    return rc


def run(ssc, env, actor, critic, K, rms=None, log=True, want_q=True, zero_returns=1, prefill=0.0):
    """-> (block [8] float64 numpy, chunk or None, q [K, n] or None)"""
    chunk = ssc.TransitionChunk(env.obs_dim, K, env.n, env.device) if log else None
    q = torch.empty((K, env.n), dtype=torch.float32, device="cuda") if want_q else None
    out = torch.full((8,), prefill, dtype=torch.float64, device="cuda")
    if chunk is not None:
        chunk.step0, chunk.env_id0 = env.t, env.env_id0
    call(env, actor, critic, K, rms=rms, chunk=chunk, q=q, zero_returns=zero_returns, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), chunk, q


def log_of(chunk):
    return dict(obs=chunk.obs.cpu().numpy(), act=chunk.act.cpu().numpy(), rew=chunk.rew.cpu().numpy(),
                done=chunk.done.cpu().numpy(), obs2=chunk.obs2.cpu().numpy())


class NoiseFreePolicy(O.OracleDDPGPolicy):
    """``O.OracleDDPGPolicy(epsilon=0)`` for a network with LayerNorm (the base class has no argument for it)"""

    def __init__(self, weights, *args, **kw):
        super().__init__(weights, *args, **kw)
        assert self.eps == 0.0

    def __call__(self, k, t, obs, prev_done):
        a = O.actor_forward(obs, **oracle_kw(self.w), last_layer_tanh=self.llt, obs_clip=self.obs_clip)[:, 0]
        return O.ddpg_action(a, 0.0, 0.0, self.low, self.high)


def stats_block(rng, od):
    """a statistics block well away from (0, 1), as tests/test_gpu_ddpg_stats.py::build_case builds it"""
    from smartstartcontinuous_amd import obs_rms as R
    mean, std = np.array([0.3, -0.6, 1.5])[:od], np.array([0.4, 2.0, 0.7])[:od]
    rows = rng.normal(mean, std, size=(4000, od)).astype(np.float32).astype(np.float64)
    block = R.rms_initial(od)
    block[:od] += rows.sum(0)
    block[od:2 * od] += (rows ** 2).sum(0)
    block[2 * od] += len(rows)
    got_mean, got_std = R.mean_std_f32(block)
    assert np.all(np.abs(got_mean) > 0.2) and np.all(np.abs(got_std - 1.0) > 0.2)
    return block


CASES = {   # env, actor h, critic h, LayerNorm, lastLayerTanh, statistics, n, K, t0, steps0
    "mc-64-32": (MC, (64, 32), (64, 32), False, True, False, 37, 41, 3, 970),       # two tiles + 5 ragged; every env meets the limit
    "mc-ln-relu": (MC, (64, 64), (64, 32), True, False, False, 16, 12, 0, 0),
    "pend-128-64-rms": (PEND, (128, 64), (128, 64), False, True, True, 33, 9, 0, 0),
    "mc-200-100": (MC, (200, 100), (200, 100), False, True, False, 17, 6, 0, 0),    # the weights-from-global path
}


@pytest.mark.parametrize("name", list(CASES))
def test_teacher_forced_parity(ssc, name):
    from smartstartcontinuous_amd import obs_rms as R
    from smartstartcontinuous_amd.obs_rms import ObsRms
    from tests.test_gpu_obs_rms_oracle import NormalisingPolicy
    env_id, ah, ch, ln, tanh, with_rms, n, K, t0, steps0 = CASES[name]
    pend = env_id == PEND
    od = 3 if pend else 2
    seed, id0 = 31, 5
    aw, cw, actor, critic = nets(50 + n, od, ah, ch, ln, tanh)
    env = ssc.VecEnv(env_id, n, seed=seed, env_id0=id0)
    env.reset()
    if pend:      # a spread of velocities: normalised, many of them lie beyond the +-5 clip
        env.s1.copy_(torch.linspace(-8.0, 8.0, n, device="cuda"))
    env.steps.fill_(steps0)
    env.t = t0
    obs0 = env.observe().cpu().numpy().copy()
    block = stats_block(np.random.default_rng(7), od) if with_rms else None
    rms = torch.as_tensor(block).cuda() if with_rms else None
    got, chunk, q = run(ssc, env, actor, critic, K, rms=rms)
    log = log_of(chunk)
    low, high = float(env.action_space.low[0]), float(env.action_space.high[0])
    mk = NoiseFreePolicy if ln else O.OracleDDPGPolicy
    pol = mk(aw, seed, id0, n, epsilon=0.0, low=low, high=high, last_layer_tanh=tanh, obs_clip=CLIP)
    if with_rms:
        holder = ObsRms(od)
        holder.block.copy_(rms)
        pol = NormalisingPolicy(pol, holder)
    kind, tmax = ("pend", 200) if pend else ("mc", 999)
    res = O.replay_rollout(kind, log, seed, id0, t0, tmax, obs0, np.full(n, steps0), pol)
    print(name, {k: v for k, v in res.items() if k != "final_elapsed"})
    assert res["start_max_err"] == 0 and res["continuity_mismatch"] == 0 and res["done_mismatch"] == 0, res
    assert res["max_dact"] <= 2e-5 * (high - low) / 2, res
    assert np.all(res["max_dobs2"] <= (3e-6 if pend else np.array([2.4e-7, 1e-8]))), res
    assert res["max_drew_rel"] <= (2e-5 if pend else 1e-6), res
    assert res["reset_max_err"] <= (2e-6 if pend else 0.0), res
    if steps0:
        assert log["done"].sum() == n                      # every env met the time limit inside the window
        assert np.array_equal(env.steps.cpu().numpy(), res["final_elapsed"])
    # ---- Q of the RAW actor output, per element, from the logged observations ----
    raw = np.moveaxis(log["obs"], 0, -1).reshape(K * n, od)
    if with_rms:
        x = R.normalize_f32(raw, block, CLIP).astype(np.float64)
        assert np.any(np.abs(x) == CLIP) and np.any(np.abs(x) < CLIP)          # some inputs sit on the clip (oracle side only)
    else:
        x = raw.astype(np.float64)
    a_ref = O.actor_forward(x, **oracle_kw(aw), last_layer_tanh=tanh, obs_clip=CLIP)
    critic_ref = lambda a: O.critic_forward(x, a, **oracle_kw(cw), last_layer_tanh=tanh, obs_clip=CLIP)[:, 0]
    q_ref = critic_ref(a_ref)
    moved = max(np.abs(critic_ref(a_ref + s * TOL_ACT) - q_ref).max() for s in (-1.0, 1.0))
    tol_q = 1e-5 * max(1.0, np.abs(q_ref).max()) + 2 * moved
    dq = np.abs(q.cpu().numpy().reshape(-1).astype(np.float64) - q_ref).max()
    print(name, "max |dQ|", dq, "tol", tol_q, "max |Q|", np.abs(q_ref).max())
    assert 1.0 <= np.abs(q_ref).max() <= 300.0
    assert dq <= tol_q, (dq, tol_q)
    assert abs(got[3] - q_ref.mean()) <= tol_q and abs(got[4] - q_ref.std()) <= tol_q and got[5] == n * K


def test_goal_terminations(ssc):
    n, K = 64, 4
    aw, cw, actor, critic = nets(3, 2, (64, 32), (64, 32))
    env = ssc.VecEnv(MC, n, seed=9)
    env.reset()
    env.s0.fill_(0.43)
    env.s1.fill_(0.06)
    got, chunk, q = run(ssc, env, actor, critic, K)
    done, rew = chunk.done.cpu().numpy(), chunk.rew.cpu().numpy()
    assert np.all(done[0] == 1) and np.all(rew[0] > 99.8)
    assert got[6] >= n and got[0] >= n and got[5] == n * K


def goal_flags(chunk):
    return chunk.obs2[0].cpu().numpy().astype(np.float64) >= np.float64(np.float32(O.MC_GOAL_POSITION))


def mid_episode_env(ssc, n, seed):
    """envs a few random steps into their episodes (non-zero running returns), every third one close to its time limit"""
    env = ssc.VecEnv(MC, n, seed=seed)
    env.reset()
    env.rollout(7, ssc.RandomPolicy(), log=False)
    env.steps[::3] = 985
    env.s0[1::7] = 0.44        # ... and some about to reach the goal
    env.s1[1::7] = 0.05
    return env


@pytest.mark.parametrize("zero_returns", [1, 0])
def test_block_against_the_kernels_own_trace(ssc, zero_returns):
    n, K = 45, 30
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))
    env = mid_episode_env(ssc, n, 21)
    start = state_of(env)
    assert np.all(start["ep_ret"].cpu().numpy() != 0.0)
    got, chunk, q = run(ssc, env, actor, critic, K, zero_returns=zero_returns)
    want, run_ret, el = E.eval_block(chunk.rew.cpu().numpy(), chunk.done.cpu().numpy(), goal_flags(chunk), q.cpu().numpy(),
                                     start["steps"].cpu().numpy(), start["ep_ret"].cpu().numpy(), bool(zero_returns))
    print("zero_returns", zero_returns, "got", got.tolist(), "want", want.tolist())
    # the emulation follows the kernel's bookkeeping bit for bit
    assert np.array_equal(env.ep_ret.cpu().numpy().view(np.uint32), run_ret.view(np.uint32))
    assert np.array_equal(env.steps.cpu().numpy(), el)
    assert want[0] >= n // 3 and want[6] >= 1 and want[0] > want[6]          # time limits and goals both occur
    E.assert_block(got, want)
    # the same launch again from the same state: the same 8 doubles
    env2 = mid_episode_env(ssc, n, 21)
    set_state(env2, start)
    again, _, _ = run(ssc, env2, actor, critic, K, zero_returns=zero_returns)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


def test_carried_return_differs_from_zeroed(ssc):
    """the two settings report different eval/return from the same state (the first episode's return carries the past or not)"""
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))
    blocks = []
    for zero in (1, 0):
        env = mid_episode_env(ssc, 45, 21)
        blocks.append(run(ssc, env, actor, critic, 30, zero_returns=zero)[0])
    assert blocks[0][0] == blocks[1][0] and blocks[0][1] != blocks[1][1]
    assert np.array_equal(blocks[0][3:].view(np.uint64), blocks[1][3:].view(np.uint64))


def test_no_episode_ends(ssc):
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))
    env = ssc.VecEnv(MC, 19, seed=4)
    env.reset()
    got, _, _ = run(ssc, env, actor, critic, 5, prefill=7.0)          # 7.0 everywhere: every slot is written
    assert got[0] == 0 and np.all(np.isnan(got[[1, 2, 7]])) and np.all(np.isfinite(got[[3, 4, 5, 6]]))
    assert got[5] == 19 * 5 and got[6] == 0 and not np.any(got == 7.0)


@pytest.mark.parametrize("c", [100.0, -3.25])
def test_reduction_in_isolation(ssc, c):
    """A critic of zero weights and b3 = c: Q = c at every step of every env, so the mean IS c and the std is 0 up to f64
    rounding -- the bounds of tests/test_gpu_ddpg_stats.py::test_reduction_in_isolation."""
    n, K = 1000, 50
    aw, _, actor, _ = nets(11, 2, (64, 32), (64, 32))
    zero = dict(W1=np.zeros((2, 64), np.float32), b1=np.zeros(64, np.float32), W2=np.zeros((65, 32), np.float32),
                b2=np.zeros(32, np.float32), W3=np.zeros((32, 1), np.float32), b3=np.full(1, c, np.float32))
    critic = Device(zero, "critic", 2, 1, True)
    env = ssc.VecEnv(MC, n, seed=4)
    env.reset()
    got, _, _ = run(ssc, env, actor, critic, K, log=False, want_q=False)
    eps = 2.0 ** -40
    print("c", c, "mean - c", got[3] - c, "std", got[4])
    assert abs(got[3] - c) <= eps * abs(c) and 0.0 <= got[4] <= eps * abs(c) and got[5] == n * K


def columns(chunk, q):
    return [chunk.obs, chunk.act, chunk.rew, chunk.done, chunk.obs2, q]


def test_chunks_compose(ssc):
    """K = 16 then K = 24 equals K = 40, column by column; time-limit resets fall into both parts"""
    n = 21
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))

    def make():
        env = ssc.VecEnv(MC, n, seed=13, env_id0=3)
        env.reset()
        env.steps[::2] = 990
        env.steps[1::2] = 970
        env.t = 6
        return env
    whole, split = make(), make()
    _, cw40, q40 = run(ssc, whole, actor, critic, 40, zero_returns=0)
    _, c16, q16 = run(ssc, split, actor, critic, 16, zero_returns=0)
    _, c24, q24 = run(ssc, split, actor, critic, 24, zero_returns=0)
    assert c16.done.sum() > 0 and c24.done.sum() > 0 and split.t == whole.t == 46
    for a, b, c in zip(columns(cw40, q40), columns(c16, q16), columns(c24, q24)):
        assert torch.equal(a, torch.cat([b, c], dim=-2))
    for k in ("s0", "s1", "steps", "ep_ret"):
        assert torch.equal(getattr(whole, k), getattr(split, k)), k


def test_id_space_shards(ssc):
    """two halves of the id range via env_id0 equal the whole"""
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))

    def make(n, id0):
        env = ssc.VecEnv(MC, n, seed=13, env_id0=id0)
        env.reset()
        env.steps.fill_(990)
        env.t = 2
        return env
    whole, lo, hi = make(40, 5), make(16, 5), make(24, 21)
    K = 20
    _, cw_, qw = run(ssc, whole, actor, critic, K)
    _, cl, ql = run(ssc, lo, actor, critic, K)
    _, ch, qh = run(ssc, hi, actor, critic, K)
    assert cw_.done.sum() == 40
    for a, b, c in zip(columns(cw_, qw), columns(cl, ql), columns(ch, qh)):
        assert torch.equal(a, torch.cat([b, c], dim=-1))
    for k in ("s0", "s1", "steps", "ep_ret"):
        assert torch.equal(getattr(whole, k), torch.cat([getattr(lo, k), getattr(hi, k)])), k


def test_weight_paths_and_log_switch_agree(ssc, monkeypatch):
    """weights staged in LDS or read from global memory, with the log or without: the same final state, the same block bits"""
    n, K = 37, 30
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))
    results = []
    for global_weights in (False, True):
        if global_weights:
            monkeypatch.setenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", "1")
        else:
            monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)
        for log in (True, False):
            env = mid_episode_env(ssc, n, 21)
            got, _, _ = run(ssc, env, actor, critic, K, log=log, want_q=log, zero_returns=0)
            results.append((got, state_of(env)))
    monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)
    assert results[0][0][0] > 0
    for got, st in results[1:]:
        assert np.array_equal(got.view(np.uint64), results[0][0].view(np.uint64))
        for k, v in st.items():
            assert torch.equal(v, results[0][1][k]), k


def test_argument_errors(ssc):
    from smartstartcontinuous_amd import _ffi
    aw, cw, actor, critic = nets(11, 2, (64, 32), (64, 32))
    _, _, actor3, critic3 = nets(11, 3, (64, 32), (64, 32))
    env = ssc.VecEnv(MC, 20, seed=4)
    env.reset()
    start = state_of(env)
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    small = torch.empty(8, dtype=torch.uint8, device="cuda")

    def variant(dev, **fields):
        d = type(dev.desc).from_buffer_copy(dev.desc)
        for k, v in fields.items():
            setattr(d, k, v)
        holder = type("D", (), {})()
        holder.desc = d
        return holder
    inval = [dict(p=None), dict(actor=None), dict(critic=None), dict(state=None), dict(ws=None), dict(n=0), dict(n=-3),
             dict(ws=_ffi.ptr(small), ws_bytes=8), dict(ws_bytes=0)]
    for over in inval:
        assert call(env, actor, critic, 4, out=out, raw=True, over=over) == _ffi.SSC_EINVAL, over
    assert call(env, actor, critic, 4, out=None, raw=True) == _ffi.SSC_EINVAL
    assert call(env, actor, critic, 0, out=out, raw=True) == call(env, actor, critic, -1, out=out, raw=True) == _ffi.SSC_EINVAL
    for a, c in ((actor3, critic3), (actor3, critic), (actor, critic3), (actor, variant(critic, act_dim=2))):
        assert call(env, a, c, 4, out=out, raw=True) == _ffi.SSC_EINVAL
    assert call(env, variant(actor, act_dim=2), variant(critic, act_dim=2), 4, out=out, raw=True) == _ffi.SSC_EUNSUPPORTED
    # a tile whose activations alone exceed LDS: 3001 rows of 16 floats for the critic's first layer alone; the byte count is reported
    assert call(env, actor, variant(critic, h1=3000), 4, out=out, raw=True) == _ffi.SSC_EUNSUPPORTED
    msg = _ffi.lib().ssc_last_error().decode()
    reported = re.search(r"(\d+) B of LDS", msg)
    assert reported is not None and int(reported.group(1)) > max(160 * 1024, 4 * 16 * 3001), msg
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)                                   # no call wrote the block ...
    for k, v in start.items():
        assert torch.equal(getattr(env, k), v), k                  # ... or moved the envs
    assert _ffi.lib().ssc_ddpg_eval_workspace_bytes(0) == 0 and _ffi.lib().ssc_ddpg_eval_workspace_bytes(17) > 0
