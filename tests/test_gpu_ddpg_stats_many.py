"""``ssc_ddpg_stats_many`` / ``DDPGPopulation.get_stats_device``: the training diagnostics of a population of agents in two
launches.  Every result is DEFINED as what ``ssc_ddpg_stats`` writes agent by agent, so every comparison here is bitwise: no
tolerance.  The single call is held to the fp64 oracle by tests/test_gpu_ddpg_stats.py; bit identity carries that bound
over.  Every output block and workspace of the population call lies between NaN-filled guard bands."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_ddpg_eval import stats_block
from tests.test_gpu_ddpg_stats import Device, launch, make_net

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = 32                                      # guard doubles either side of every block and workspace
SENT = 7.0                                  # what a block holds before the call


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


# m, (obs_dim, act_dim), actor h, critic h, LayerNorm, lastLayerTanh, statistics block, perturbed copy
PAIRS = [(1, (2, 1), (64, 32), (64, 32), False, True, False, False),
         (16, (3, 1), (64, 64), (64, 64), True, False, True, True),
         (17, (2, 1), (64, 32), (128, 64), False, False, False, True),
         (0, (2, 1), (64, 32), (64, 32), False, True, True, True),          # no sample yet: skipped
         (64, (3, 2), (200, 100), (200, 100), False, True, True, False),
         (64, (2, 1), (7, 5), (7, 5), True, True, False, True)]


class Agent:
    def __init__(self, p, m, dims, ah, ch, ln, tanh, with_rms, with_pert):
        od, ad = dims
        rng = np.random.default_rng(500 + p)
        aw = make_net(rng, od, ah[0], 0, ah[1], ad, ln, 0.25, 0.0)
        cw = make_net(rng, od, ch[0], ad, ch[1], 1, ln, 1.5, 20.0)
        self.m = m
        self.actor, self.critic = Device(aw, "actor", od, ad, tanh), Device(cw, "critic", od, ad, tanh)
        self.pert = self.sd = self.rms = self.obs = self.act = None
        if with_pert:
            pw = {k: (v + (0.2 * rng.normal(size=v.shape)).astype(np.float32) if not k.startswith("ln") else v) for k, v in aw.items()}
            self.pert = Device(pw, "actor", od, ad, tanh)
            self.sd = torch.tensor([0.1 + 0.05 * p], dtype=torch.float32, device="cuda")
        if with_rms:
            self.rms = torch.as_tensor(stats_block(np.random.default_rng(7 + p), od)).cuda()
        if m:
            self.obs = torch.as_tensor(rng.uniform(-6.0, 6.0, size=(m, od)).astype(np.float32)).cuda()
            self.act = torch.as_tensor(rng.uniform(-1, 1, size=(m, ad)).astype(np.float32)).cuda()


def many(agents):
    """the population call -> [P, 11]; blocks pre-filled with SENT, guards and workspaces with NaN"""
    from smartstartcontinuous_amd import _ffi
    from smartstartcontinuous_amd.population import DeviceItems
    lib, P = _ffi.lib(), len(agents)
    words = [int(lib.ssc_ddpg_stats_workspace_bytes(a.m)) // 8 for a in agents]
    out = torch.full((P, G + 11 + G), float("nan"), dtype=torch.float64, device="cuda")
    out[:, G:G + 11] = SENT
    ws = [torch.full((G + w + G,), float("nan"), dtype=torch.float64, device="cuda") for w in words]
    items = DeviceItems(_ffi.DdpgStatsManyItem, P, "cuda")
    for p, (it, a) in enumerate(zip(items.items, agents)):
        it.actor, it.critic, it.m = a.actor.desc, a.critic.desc, a.m
        if a.pert is not None:
            it.perturbed, it.has_perturbed, it.d_param_noise_stddev = a.pert.desc, 1, a.sd.data_ptr()
        if a.m:
            it.d_obs, it.d_act = a.obs.data_ptr(), a.act.data_ptr()
        it.d_rms = None if a.rms is None else a.rms.data_ptr()
        it.d_out, it.d_workspace, it.workspace_bytes = out[p, G:].data_ptr(), ws[p][G:].data_ptr(), 8 * words[p]
    items.upload()
    _ffi.check(lib.ssc_ddpg_stats_many(items.h_ptr, items.d_ptr, P, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.isnan(out[:, :G]).all() and torch.isnan(out[:, G + 11:]).all()
    for a, w, x in zip(agents, words, ws):
        assert torch.isnan(x[:G]).all() and torch.isnan(x[G + w:]).all()
        if a.pert is not None:               # every word of the workspace is written (without a perturbed copy: three streams of four)
            assert not torch.isnan(x[G:G + w]).any()
    return out[:, G:G + 11].clone()


def test_population_is_bitwise_the_single_calls(ssc):
    agents = [Agent(p, *spec) for p, spec in enumerate(PAIRS)]
    got = many(agents)
    for p, a in enumerate(agents):
        if a.m == 0:
            assert torch.all(got[p] == SENT)                     # the skipped pair's block is untouched
            continue
        want = launch(ssc, a.actor, a.critic, a.pert, a.obs, a.act, a.rms, a.sd)
        assert torch.equal(got[p].view(torch.int64), want.view(torch.int64)), (p, got[p], want)
        nan = torch.isnan(got[p]).cpu().numpy()
        assert nan[[0, 1]].all() == (a.rms is None) and nan[[8, 9, 10]].all() == (a.pert is None) and not nan[2:8].any()
    assert len({float(x) for x in got[[0, 1, 2, 4, 5], 2]}) == 5      # the pairs do differ


def test_only_skipped_pairs_launch_nothing(ssc):
    agents = [Agent(p, 0, *spec[1:]) for p, spec in enumerate(PAIRS[:3])]
    assert torch.all(many(agents) == SENT)


# ---- DDPGPopulation.get_stats_device ---------------------------------------------------------------------------------
def make_agents(ssc):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    kws = [dict(actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32),
           dict(actor_h1=128, actor_h2=64, critic_h1=128, critic_h2=64, normalize_observations=True, param_noise_stddev=0.2),
           dict(actor_h1=64, actor_h2=64, critic_h1=64, critic_h2=32, layer_norm=True),
           dict(actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, param_noise_stddev=0.1)]
    agents = [DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, batch_size=64, lastLayerTanh=True, seed=40 + p, **kw)
              for p, kw in enumerate(kws)]
    agents[1].obs_rms.update_rows(np.random.default_rng(4).uniform(-1.2, 0.6, (300, 2)).astype(np.float32))
    return agents


def test_population_get_stats_is_bitwise_the_agents_own(ssc):
    from tests.test_gpu_ddpg_many import make_replay
    agents, twins = make_agents(ssc), make_agents(ssc)
    records = (256, 256, 40, 200)                                # the third ring holds fewer than batch_size records
    replays, t_replays = ([make_replay(ssc, p, n) for p, n in enumerate(records)] for _ in range(2))
    pop = ssc.DDPGPopulation(agents)
    got = pop.get_stats_device(replays)
    assert pop.stats_fused is True and getattr(agents[2], "stats_sample", None) is None and torch.isnan(got[2]).all()
    for p in (0, 1, 3):
        want = twins[p].get_stats_device(t_replays[p])
        assert torch.equal(got[p].view(torch.int64), want.view(torch.int64)), p
        assert torch.equal(agents[p].stats_sample[0], twins[p].stats_sample[0])      # the sample drawn and kept is the agent's own
    assert [r._batches_drawn for r in replays] == [0] * 4        # ... from a stream of its own
    # the ring fills up: the agent joins with its own sample, the others keep theirs; out= is written in place
    replays[2].count = t_replays[2].count = 64
    block = torch.full((4, 11), 7.0, dtype=torch.float64, device="cuda")
    assert pop.get_stats_device(replays, out=block) is block
    items = pop._stats_items
    for p in range(4):
        want = twins[p].get_stats_device(t_replays[p])
        assert torch.equal(block[p].view(torch.int64), want.view(torch.int64)), p
    pop.get_stats_device(replays, out=block)
    assert pop._stats_items is items                             # nothing changed: the descriptors are reused
    dicts = pop.get_stats(replays)
    assert dicts == [a.get_stats(r) for a, r in zip(twins, t_replays)]
    assert "param_noise_stddev" in dicts[1] and "obs_rms_mean" in dicts[1] and "obs_rms_mean" not in dicts[0]


def test_population_with_return_statistics_falls_back(ssc):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from tests.test_gpu_ddpg_many import make_replay
    mk = lambda: [DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, batch_size=64, actor_h1=64, actor_h2=32, critic_h1=64,
                                       critic_h2=32, lastLayerTanh=True, seed=40 + p, normalize_returns=p == 1, enable_popart=p == 1)
                  for p in range(2)]
    agents, twins = mk(), mk()
    for a in (agents[1], twins[1]):
        a.ret_rms.update_rows(np.random.default_rng(3).normal(-20.0, 6.0, (200, 1)).astype(np.float32))
    replays, t_replays = ([make_replay(ssc, p) for p in range(2)] for _ in range(2))
    pop = ssc.DDPGPopulation(agents)
    got = pop.get_stats_device(replays)
    assert pop.stats_fused is False
    for p in range(2):
        want = twins[p].get_stats_device(t_replays[p])
        assert torch.equal(got[p].view(torch.int64), want.view(torch.int64)), p
    assert "ret_rms_mean" in pop.get_stats(replays)[1]
