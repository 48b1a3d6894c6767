"""``ssc_ddpg_eval_rollout_many`` / ``DDPGPopulation.evaluate_device``: a population of (eval-env set, agent) pairs in one
fused launch plus one merge launch.  Every result is DEFINED as what ``ssc_ddpg_eval_rollout`` leaves pair by pair from the
same starting state, so every comparison here is bitwise: no tolerance.  The single call is held to the fp64 oracle by
tests/test_gpu_ddpg_eval.py; bit identity carries that bound over.

The sizes sit on the 16-env tile edges (1, 16, 17, 33); every output block and workspace of the population call lies
between NaN-filled guard bands."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_ddpg_eval import MC, PEND, call, nets, set_state, state_of, stats_block

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = 32                                      # guard doubles either side of every block and workspace
STATE = ("s0", "s1", "steps", "ep_ret")


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


@pytest.fixture(autouse=True)
def _weights_where_they_fit(monkeypatch):
    monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)


class Pair:
    """one (eval-env set, agent): the env, both networks on the device, a statistics block or None"""

    def __init__(self, ssc, p, env_id, n, shape=(64, 32), ln=False, tanh=True, rms=False, limit=None, t0=0):
        od = 3 if env_id == PEND else 2
        self.env = ssc.VecEnv(env_id, n, seed=50 + p, env_id0=1000 * p, max_episode_steps=limit)
        self.env.reset()
        self.env.t = t0
        _, _, self.actor, self.critic = nets(200 + p, od, shape, shape, ln, tanh)
        self.rms = torch.as_tensor(stats_block(np.random.default_rng(7 + p), od)).cuda() if rms else None

    def twin(self, ssc):
        """the same pair over a copy of the env's state (the networks are only read: shared)"""
        other = object.__new__(Pair)
        e = self.env
        other.env = ssc.VecEnv(e.spec.id, e.n, seed=e._seed, env_id0=e.env_id0, max_episode_steps=e.params.max_episode_steps)
        other.env.reset()
        set_state(other.env, state_of(e))
        other.env.t = e.t
        other.actor, other.critic, other.rms = self.actor, self.critic, self.rms
        return other


def singles(pairs, K, zero_returns):
    """the per-pair calls -> [P, 8] float64"""
    out = torch.full((len(pairs), 8), 7.0, dtype=torch.float64, device="cuda")
    for p, x in enumerate(pairs):
        call(x.env, x.actor, x.critic, K, rms=x.rms, zero_returns=zero_returns, out=out[p])
    return out


class Launch:
    """the population call on ``pairs``: items, cursors, and every block and workspace between guard bands"""

    def __init__(self, pairs):
        from smartstartcontinuous_amd import _ffi
        from smartstartcontinuous_amd.population import DeviceItems, PairCursors
        self.ffi, self.pairs, P = _ffi, pairs, len(pairs)
        lib = _ffi.lib()
        self.words = [int(lib.ssc_ddpg_eval_workspace_bytes(x.env.n)) // 8 for x in pairs]
        self.out = torch.full((P, G + 8 + G), float("nan"), dtype=torch.float64, device="cuda")
        self.ws = [torch.full((G + w + G,), float("nan"), dtype=torch.float64, device="cuda") for w in self.words]
        self.items = DeviceItems(_ffi.DdpgEvalManyItem, P, "cuda")
        for p, (it, x) in enumerate(zip(self.items.items, pairs)):
            e = x.env
            it.params, it.actor, it.critic = e.params, x.actor.desc, x.critic.desc
            it.act_low, it.act_high = float(e.action_space.low[0]), float(e.action_space.high[0])
            it.n, it.state = e.n, e.rollout_state(ou=False)
            it.d_rms = None if x.rms is None else x.rms.data_ptr()
            it.d_out, it.d_workspace = self.out[p, G:].data_ptr(), self.ws[p][G:].data_ptr()
            it.workspace_bytes, it.seed, it.env_id0 = 8 * self.words[p], e._seed, e.env_id0
        self.items.upload()
        self.cursors = PairCursors(P, "cuda")

    def __call__(self, K, zero_returns):
        envs = [x.env for x in self.pairs]
        self.cursors.stage(step0=[e.t for e in envs]).upload()
        self.ffi.check(self.ffi.lib().ssc_ddpg_eval_rollout_many(
            self.items.h_ptr, self.items.d_ptr, self.cursors.h_ptr, self.cursors.d_ptr, len(envs), K, zero_returns,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        for e in envs:
            e.t += K
        torch.cuda.synchronize()
        # the guard bands either side of every block and workspace are untouched, every word between them is written
        assert torch.isnan(self.out[:, :G]).all() and torch.isnan(self.out[:, G + 8:]).all()
        for w, ws in zip(self.words, self.ws):
            assert torch.isnan(ws[:G]).all() and torch.isnan(ws[G + w:]).all() and not torch.isnan(ws[G:G + w]).any()
        return self.out[:, G:G + 8].clone()


def assert_same(got, want, pairs, twins):
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (got, want)       # bits: NaN slots included
    for p, (x, y) in enumerate(zip(pairs, twins)):
        for k in STATE:
            assert torch.equal(getattr(x.env, k), getattr(y.env, k)), (p, k)
        assert x.env.t == y.env.t


def mountaincar_population(ssc):
    """n = 1, 16, 17, 33 with a 7-step time limit (every env resets several times in 23 steps); half of the last pair's envs
    start where the first step reaches the goal (tests/test_gpu_ddpg_eval.py::test_goal_terminations)"""
    pairs = [Pair(ssc, p, MC, n, limit=7, t0=3 * p) for p, n in enumerate((1, 16, 17, 33))]
    for p, x in enumerate(pairs):
        x.env.steps.copy_(torch.arange(x.env.n, device="cuda", dtype=torch.int32) % 7)
        x.env.ep_ret.copy_(-0.25 * torch.arange(1, x.env.n + 1, device="cuda", dtype=torch.float32))
    pairs[3].env.s0[::2] = 0.43
    pairs[3].env.s1[::2] = 0.06
    return pairs


@pytest.mark.parametrize("zero_returns", [1, 0])
def test_mountaincar_population_is_bitwise_the_single_calls(ssc, zero_returns):
    pairs = mountaincar_population(ssc)
    twins = [x.twin(ssc) for x in pairs]
    many = Launch(pairs)
    for K in (23, 5):                        # the second call continues with advanced cursors, as two single calls in a row
        got, want = many(K, zero_returns), singles(twins, K, zero_returns)
        assert_same(got, want, pairs, twins)
        if K == 23:
            block = got.cpu().numpy()
            assert np.all(block[:, 0] >= 3 * np.array([1, 16, 17, 33]))          # every env met the limit several times
            assert block[3, 6] >= 17 and np.all(block[:3, 6] == 0)               # goals where they were set up, only there
            assert np.array_equal(block[:, 5], 23.0 * np.array([1, 16, 17, 33]))


def mixed_population(ssc, wide):
    """64-32, 7-5 with LayerNorm, 128-64 with a ReLU last layer, 64-32 ReLU -- statistics on pairs 1 and 2 only; ``wide``
    adds a 200-100 pair whose weights do not fit LDS, which takes the staging away from the whole launch"""
    spec = [dict(n=17, shape=(64, 32)), dict(n=16, shape=(7, 5), ln=True, rms=True), dict(n=33, shape=(128, 64), tanh=False, rms=True),
            dict(n=1, shape=(64, 32), tanh=False)]
    if wide:
        spec.append(dict(n=17, shape=(200, 100)))
    return [Pair(ssc, p, MC, limit=9, t0=p, **kw) for p, kw in enumerate(spec)]


@pytest.mark.parametrize("weights", ["lds", "forced-global", "too-wide-for-lds"])
def test_mixed_shapes_share_a_launch(ssc, weights, monkeypatch):
    pairs = mixed_population(ssc, weights == "too-wide-for-lds")
    twins = [x.twin(ssc) for x in pairs]
    want = singles(twins, 23, 1)             # the single calls stage what fits, whatever the population launch does
    if weights == "forced-global":
        monkeypatch.setenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", "1")
    got = Launch(pairs)(23, 1)
    assert_same(got, want, pairs, twins)
    block = got.cpu().numpy()
    assert np.all(block[:, 0] >= 2) and len({block[p, 3] for p in range(len(pairs))}) == len(pairs)


def test_pendulum_population(ssc):
    pairs = [Pair(ssc, p, PEND, n, rms=p == 1, limit=6, t0=2) for p, n in enumerate((5, 16, 40))]
    for x in pairs:
        x.env.s1.copy_(torch.linspace(-8.0, 8.0, x.env.n, device="cuda"))
    twins = [x.twin(ssc) for x in pairs]
    got, want = Launch(pairs)(14, 1), singles(twins, 14, 1)
    assert_same(got, want, pairs, twins)
    assert np.all(got.cpu().numpy()[:, 0] >= 2 * np.array([5, 16, 40]))


def test_more_pairs_than_compute_units(ssc):
    """260 pairs of one env each: more grid rows than the device has CUs"""
    P = 260
    _, _, actor, critic = nets(11, 2, (64, 32), (64, 32))
    pairs = []
    for p in range(P):                       # one network pair for all (weights may be shared), 260 env sets
        x = Pair.__new__(Pair)
        x.env = ssc.VecEnv(MC, 1, seed=300 + p, env_id0=p, max_episode_steps=5)
        x.env.reset()
        x.actor, x.critic, x.rms = actor, critic, None
        pairs.append(x)
    twins = [x.twin(ssc) for x in pairs]
    got, want = Launch(pairs)(12, 1), singles(twins, 12, 1)
    assert_same(got, want, pairs, twins)
    assert len(torch.unique(got[:, 3])) > P // 2                 # the pairs do differ


def test_a_refused_population_touches_nothing(ssc):
    from smartstartcontinuous_amd import _ffi
    pairs = [Pair(ssc, 0, MC, 4), Pair(ssc, 1, PEND, 4)]
    many = Launch(pairs)
    before = [state_of(x.env) for x in pairs]
    rc = _ffi.lib().ssc_ddpg_eval_rollout_many(many.items.h_ptr, many.items.d_ptr, many.cursors.h_ptr, many.cursors.d_ptr, 2, 3, 1, None)
    assert rc == _ffi.SSC_EINVAL and b"env kind" in _ffi.lib().ssc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(many.out).all()
    for x, st in zip(pairs, before):
        for k, v in st.items():
            assert torch.equal(getattr(x.env, k), v)


# ---- DDPGPopulation.evaluate_device ----------------------------------------------------------------------------------
def make_agents(ssc, kws):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    return [DDPG_Baselines_agent(ssc.make(MC), None, batch_size=64, lastLayerTanh=True, seed=40 + p, **kw) for p, kw in enumerate(kws)]


def eval_envs(ssc, sizes=(17, 16, 33)):
    envs = [ssc.VecEnv(MC, n, seed=70 + p, env_id0=100 * p, max_episode_steps=8) for p, n in enumerate(sizes)]
    for e in envs[1:]:                        # the first is reset by the call
        e.reset()
    return envs


def feed_statistics(agents):
    rows = np.random.default_rng(4).uniform(-1.2, 0.6, (300, 2)).astype(np.float32)
    for a in agents:
        if a.obs_rms is not None:
            a.obs_rms.update_rows(rows)


SHAPES = [dict(actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32), dict(actor_h1=128, actor_h2=64, critic_h1=128, critic_h2=64,
                                                                           normalize_observations=True),
          dict(actor_h1=64, actor_h2=64, critic_h1=64, critic_h2=32, layer_norm=True)]


def test_population_evaluate_is_bitwise_the_agents_own(ssc):
    agents, twins = make_agents(ssc, SHAPES), make_agents(ssc, SHAPES)
    feed_statistics(agents), feed_statistics(twins)
    envs, t_envs = eval_envs(ssc), eval_envs(ssc)
    pop = ssc.DDPGPopulation(agents)
    block = torch.full((3, 8), float("nan"), dtype=torch.float64, device="cuda")
    for call_no, carry in enumerate((False, False, True)):       # the later calls reuse the descriptors
        got = pop.evaluate_device(envs, 19, out=block, carry_returns=carry)
        assert got is block and pop.eval_fused is True
        items = pop._eval_items
        want = torch.stack([a.evaluate_device(e, 19, carry_returns=carry) for a, e in zip(twins, t_envs)])
        assert torch.equal(got.view(torch.int64), want.view(torch.int64))
        for e, t in zip(envs, t_envs):
            assert e.t == t.t == 19 * (call_no + 1)
            for k in STATE:
                assert torch.equal(getattr(e, k), getattr(t, k))
    assert pop._eval_items is items                              # built once
    dicts = pop.evaluate(envs, 5)
    assert [d["eval/steps"] for d in dicts] == [5 * e.n for e in envs] and all(isinstance(d["eval/episodes"], int) for d in dicts)
    with pytest.raises(ValueError):
        pop.evaluate_device(envs[:2], 5)
    with pytest.raises(ValueError):
        pop.evaluate_device(envs, 0)


def test_population_with_return_statistics_falls_back(ssc):
    kws = [SHAPES[0], dict(SHAPES[0], normalize_returns=True, enable_popart=True), SHAPES[0]]
    agents, twins = make_agents(ssc, kws), make_agents(ssc, kws)
    for a in (agents[1], twins[1]):                              # return statistics well away from (0, 1)
        a.ret_rms.update_rows(np.random.default_rng(3).normal(-20.0, 6.0, (200, 1)).astype(np.float32))
    envs, t_envs = eval_envs(ssc), eval_envs(ssc)
    pop = ssc.DDPGPopulation(agents)
    got = pop.evaluate_device(envs, 19)
    assert pop.eval_fused is False
    want = torch.stack([a.evaluate_device(e, 19) for a, e in zip(twins, t_envs)])
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert abs(float(got[1, 3]) + 20.0) < 15.0 and [e.t for e in envs] == [19] * 3     # the denormalised eval/Q
