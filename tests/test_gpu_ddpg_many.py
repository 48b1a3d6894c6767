"""A population of DDPG agents in one learner launch (ssc_ddpg_train_many, ssc_replay_sample_many, DDPGPopulation,
rl_train_vec_ddpg_population).  Every result is DEFINED as what the single-agent path gives agent by agent, so every
comparison here is torch.equal: no tolerance.  The single-agent kernel is held to the fp64 oracle by the existing suite
(tests/test_gpu_agents.py, tests/test_gpu_ddpg_rms_matrix.py); bit identity carries that bound over.

The kernel tests drive the C entry points on arrays of their own: agent p's copy of an array is row p of a 2-d tensor with
a guard band either side, so the neighbours of every array are other agents' guards."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import rms_edge_stats

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = 64                    # guard floats either side of every array (arrays stay 16-byte aligned)
SENT = -12345.0
SENT_I = 0x5A5A5A5A
B = 64
ARRAYS = ("actor", "critic", "target_actor", "target_critic", "adam_m_actor", "adam_v_actor", "adam_m_critic", "adam_v_critic")


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


@pytest.fixture(autouse=True)
def _no_path_switches(monkeypatch):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)


def pad4(n):
    return (n + 3) // 4 * 4


class Pop:
    """P agents of the shipped shape as raw arrays: distinct parameters, non-zero Adam moments and step counters, distinct
    gamma / tau / learning rates, a ring of ``cap`` random records (one in ten terminal) and ``n_max`` index batches each."""

    def __init__(self, P, obs_dim, llt, cap=256, n_max=4, seed=0, obs_ranges=None):
        self.P, self.O, self.llt, self.cap, self.n_max = P, obs_dim, llt, cap, n_max
        rng = np.random.default_rng(1000 + seed)
        na = obs_dim * 64 + 64 + 64 * 32 + 32 + 32 + 1
        nc = obs_dim * 64 + 64 + 65 * 32 + 32 + 32 + 1
        self.n = dict(actor=na, target_actor=na, adam_m_actor=na, adam_v_actor=na, critic=nc, target_critic=nc, adam_m_critic=nc,
                      adam_v_critic=nc)
        self.T = {}
        for name in ARRAYS:
            n = self.n[name]
            if "adam_m" in name:
                x = 1e-3 * rng.normal(size=(P, n))
            elif "adam_v" in name:
                x = 1e-6 * rng.random((P, n))
            else:
                x = rng.uniform(-0.3, 0.3, (P, n))
            full = np.full((P, G + pad4(n) + G), SENT, np.float32)
            full[:, G:G + n] = x
            self.T[name] = torch.as_tensor(full, device="cuda")
        t = np.full((P, 12), SENT_I, np.int32)
        t[:, 4:6] = rng.integers(0, 40, (P, 2))
        self.T["adam_t"] = torch.as_tensor(t, device="cuda")
        losses = np.full((P, 2 * G + 2 * (n_max + 2)), SENT, np.float32)
        losses[:, G:G + 2 * (n_max + 2)] = np.nan
        self.T["losses"] = torch.as_tensor(losses, device="cuda")
        self.hyper = [dict(gamma=0.9 + 0.02 * (p % 5), tau=0.001 * (1 + p % 4), actor_lr=1e-4 * (1 + p % 3), critic_lr=1e-3 / (1 + p % 2))
                      for p in range(P)]
        s = np.empty((P, cap, obs_dim), np.float32)
        for p in range(P):
            lo, hi = (-1.2, 0.6) if obs_ranges is None else obs_ranges[p]
            s[p] = rng.uniform(lo, hi, (cap, obs_dim))
        dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
        self.s = dev(s, torch.float32)
        self.s2 = dev(s + 0.01 * rng.normal(size=s.shape), torch.float32)
        self.a = dev(rng.uniform(-1, 1, (P, cap, 1)), torch.float32)
        self.r = dev(0.5 * rng.normal(size=(P, cap)), torch.float32)
        self.t = dev(rng.random((P, cap)) < 0.1, torch.uint8)
        self.idx = dev(np.stack([[rng.permutation(cap)[:B] for _ in range(n_max)] for _ in range(P)]), torch.int32)

    def clone(self):
        import copy
        other = copy.copy(self)
        other.T = {k: v.clone() for k, v in self.T.items()}     # rings and indices are read-only: shared
        return other

    def view(self, name, p):
        if name == "adam_t":
            return self.T[name][p, 4:6]
        if name == "losses":
            return self.T[name][p, G:G + 2 * (self.n_max + 2)].view(-1, 2)
        return self.T[name][p, G:G + self.n[name]]

    def desc(self, ffi, p):
        d = ffi.DdpgDesc()
        d.obs_dim, d.act_dim, d.actor_h1, d.actor_h2, d.critic_h1, d.critic_h2 = self.O, 1, 64, 32, 64, 32
        d.last_layer_tanh, d.batch_size = int(self.llt), B
        for name in ARRAYS + ("adam_t",):
            setattr(d, name, self.view(name, p).data_ptr())
        for k, v in self.hyper[p].items():
            setattr(d, k, v)
        d.beta1, d.beta2, d.epsilon, d.obs_clip = 0.9, 0.999, 1e-8, 5.0
        return d

    def replay(self, ffi, p):
        return ffi.ReplayView(self.s[p].data_ptr(), self.a[p].data_ptr(), self.r[p].data_ptr(), self.t[p].data_ptr(),
                              self.s2[p].data_ptr(), self.cap)

    def train_single(self, ffi, p, n, rms=None, first=0):
        """the call agent.train_on makes today: ssc_ddpg_train_ws / ssc_ddpg_train_ws_rms with the agent's workspace"""
        if n == 0:
            return
        d, rv = self.desc(ffi, p), self.replay(ffi, p)
        lib = ffi.lib()
        ws = torch.empty(int(lib.ssc_ddpg_train_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8, device="cuda")
        idx, losses = self.idx[p, first:], self.view("losses", p)
        if rms is None:
            ffi.check(lib.ssc_ddpg_train_ws(ctypes.byref(d), ctypes.byref(rv), ffi.ptr(idx), n, ffi.ptr(losses), ffi.ptr(ws), ws.numel(),
                                            ffi.stream()))
        else:
            ffi.check(lib.ssc_ddpg_train_ws_rms(ctypes.byref(d), ctypes.byref(rv), ffi.ptr(idx), n, ffi.ptr(losses), ffi.ptr(ws),
                                                ws.numel(), ffi.stream(), ffi.ptr(rms)))

    def train_many(self, ffi, n, rms=None, first=0):
        items = (ffi.DdpgManyItem * self.P)()
        for p, it in enumerate(items):
            it.ddpg, it.replay = self.desc(ffi, p), self.replay(ffi, p)
            it.d_batch_idx, it.d_losses = self.idx[p, first:].data_ptr(), self.view("losses", p).data_ptr()
            it.d_rms = None if rms is None else rms[p].data_ptr()
            it.n_iters = n[p]
        d_items = torch.frombuffer(bytearray(items), dtype=torch.uint8).cuda()
        ffi.check(ffi.lib().ssc_ddpg_train_many(ctypes.addressof(items), d_items.data_ptr(), self.P, ffi.stream()))
        torch.cuda.synchronize()

    def assert_equal(self, other):
        for name in self.T:
            a, b = self.T[name], other.T[name]
            if name == "losses":                     # NaN where no iteration wrote
                assert torch.equal(torch.isnan(a), torch.isnan(b)), name
                a, b = torch.nan_to_num(a), torch.nan_to_num(b)
            rows = [p for p in range(self.P) if not torch.equal(a[p], b[p])]
            assert not rows, (name, rows)

    def assert_guards(self):
        for name, t in self.T.items():
            if name == "adam_t":
                assert bool((t[:, :4] == SENT_I).all()) and bool((t[:, 6:] == SENT_I).all()), name
                continue
            n = 2 * (self.n_max + 2) if name == "losses" else self.n[name]
            assert bool((t[:, :G] == SENT).all()) and bool((t[:, G + n:] == SENT).all()), name
        assert bool(torch.isfinite(torch.stack([self.view("actor", p).abs().max() for p in range(self.P)])).all())


_RMS = {}


def stats_for(obs_dim, P):
    """-> (statistics block per agent, raw observation range per agent): even agents on the std floor, odd ones above it"""
    if obs_dim not in _RMS:
        _RMS[obs_dim] = {kind: rms_edge_stats(obs_dim, kind) for kind in ("floor", "wide")}
    both = _RMS[obs_dim]
    kinds = ["floor" if p % 2 == 0 else "wide" for p in range(P)]
    return [both[k][0].block.clone() for k in kinds], [both[k][1] for k in kinds]


N_ITERS = (3, 0, 1, 4, 2)


@pytest.mark.parametrize("stats", ["none", "all"])
@pytest.mark.parametrize("llt", [False, True])
@pytest.mark.parametrize("obs_dim", [2, 3])
def test_many_launch_is_bitwise_the_single_launches(ssc, obs_dim, llt, stats):
    """P = 5, n_iters (3, 0, 1, 4, 2): parameters, targets, the four Adam moment arrays, adam_t and the losses of every
    agent equal those of its copy trained alone; with statistics, agents alternate a block on the std floor and one above."""
    ffi = ssc._ffi
    rms, ranges = stats_for(obs_dim, 5) if stats == "all" else (None, None)
    pop = Pop(5, obs_dim, llt, seed=obs_dim, obs_ranges=ranges)
    ref, before = pop.clone(), pop.clone()
    for p, n in enumerate(N_ITERS):
        ref.train_single(ffi, p, n, None if rms is None else rms[p])
    pop.train_many(ffi, N_ITERS, rms)
    pop.assert_equal(ref)
    pop.assert_guards()
    assert all(not torch.equal(pop.view(name, 3), before.view(name, 3)) for name in ARRAYS)      # it trained


def test_untouched_neighbours(ssc):
    """The n_iters = 0 agent's arrays, its step counters and its loss rows are exactly as they were; loss rows beyond each
    agent's n_iters stay NaN; every guard band is intact."""
    ffi = ssc._ffi
    pop = Pop(5, 3, True, seed=7)
    before = pop.clone()
    pop.train_many(ffi, N_ITERS)
    pop.assert_guards()
    for name in ARRAYS + ("adam_t",):
        assert torch.equal(pop.T[name][1], before.T[name][1]), name
    for p, n in enumerate(N_ITERS):
        rows = pop.view("losses", p)
        assert bool(torch.isfinite(rows[:n]).all()) and bool(torch.isnan(rows[n:]).all()), p
        assert [int(x) for x in pop.view("adam_t", p) - before.view("adam_t", p)] == [n, n]


def test_more_agents_than_compute_units(ssc):
    """P = 260 workgroups of a 154 KB LDS image on 256 CUs: the last ones queue.  One iteration each on 64-record rings
    (every batch is the whole ring), against 260 single launches of ssc_ddpg_train."""
    ffi = ssc._ffi
    lib = ffi.lib()
    pop = Pop(260, 2, True, cap=64, n_max=1, seed=3)
    ref = pop.clone()
    for p in range(260):
        d, rv = ref.desc(ffi, p), ref.replay(ffi, p)
        ffi.check(lib.ssc_ddpg_train(ctypes.byref(d), ctypes.byref(rv), ffi.ptr(ref.idx[p]), 1, ffi.ptr(ref.view("losses", p)), ffi.stream()))
    pop.train_many(ffi, [1] * 260)
    pop.assert_equal(ref)
    pop.assert_guards()


def test_second_launch_round_trips_the_optimiser_state(ssc):
    """Two consecutive many-launches == two consecutive single launches: the Adam moments and step counters go through HBM."""
    ffi = ssc._ffi
    pop = Pop(3, 2, False, n_max=6, seed=5)
    ref = pop.clone()
    for first, n in ((0, (2, 1, 1)), (2, (2, 3, 1))):          # index rows [0, 2) then [2, 5) of 6
        for p in range(3):
            ref.train_single(ffi, p, n[p], first=first)
        pop.train_many(ffi, n, first=first)
    pop.assert_equal(ref)
    pop.assert_guards()


@pytest.mark.parametrize("batch", [1, 17, 64])
def test_sample_many_equals_the_single_draws(ssc, batch):
    """P = 7 keys, distinct in seed, counter0 and size -- size == batch_size, sizes above 2^31 / 64 and the largest one --
    three batches each: the rows of ssc_replay_sample called once per key."""
    ffi = ssc._ffi
    lib = ffi.lib()
    sizes = [batch, batch + 1, 256, 4096, (1 << 31) // 64 + 12345, 1_000_000_007, 0x7fffffff]
    keys = (ffi.ReplaySampleKey * 7)()
    for p, k in enumerate(keys):
        k.seed, k.counter0, k.size = 17 + 1000 * p, 5 * p * p, sizes[p]
    keys[6].counter0 = (1 << 40) + 3
    n = 7 * 3 * batch
    got = torch.full((n + 2 * G,), SENT_I, dtype=torch.int32, device="cuda")
    d_keys = torch.frombuffer(bytearray(keys), dtype=torch.uint8).cuda()
    ffi.check(lib.ssc_replay_sample_many(ctypes.addressof(keys), d_keys.data_ptr(), 7, 3, batch, got[G:].data_ptr(), ffi.stream()))
    want = torch.empty((7, 3, batch), dtype=torch.int32, device="cuda")
    for p, k in enumerate(keys):
        ffi.check(lib.ssc_replay_sample(k.seed, k.counter0, k.size, 3, batch, want[p].data_ptr(), ffi.stream()))
    assert torch.equal(got[G:G + n].view(7, 3, batch), want)
    assert bool((got[:G] == SENT_I).all()) and bool((got[G + n:] == SENT_I).all())
    rows = want.cpu().numpy()
    assert all(len(set(r)) == batch for r in rows.reshape(-1, batch)) and rows.min() >= 0
    assert all(rows[p].max() < sizes[p] for p in range(7)) and rows[4].max() >= 1 << 24


# ---- DDPGPopulation on agent objects ---------------------------------------------------------------------------------
AGENT_STATE = ("actor_flat", "critic_flat", "target_actor_flat", "target_critic_flat", "_adam_t")


def make_agent(ssc, p, h=(64, 32), **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    kw.setdefault("num_train_iterations", 1 + p % 3)
    return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, batch_size=64, actor_h1=h[0], actor_h2=h[1], critic_h1=h[0],
                                critic_h2=h[1], lastLayerTanh=True, seed=40 + p, actor_lr=1e-4 * (1 + p), critic_lr=1e-3 / (1 + p),
                                gamma=0.99 - 0.01 * p, tau=0.001 * (1 + p), **kw)


def make_replay(ssc, p, records=256):
    rng = np.random.default_rng(90 + p)
    r = ssc.DeviceReplayBuffer(256, 2, seed=7 + p)
    dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
    s = rng.uniform(-1.2, 0.6, (256, 2))
    r.s.copy_(dev(s, torch.float32)); r.s2.copy_(dev(s + 0.01 * rng.normal(size=s.shape), torch.float32))
    r.a.copy_(dev(rng.uniform(-1, 1, (256, 1)), torch.float32)); r.r.copy_(dev(0.5 * rng.normal(size=256), torch.float32))
    r.t.copy_(dev(rng.random(256) < 0.1, torch.uint8))
    r.count = records
    return r


def agent_tensors(a):
    return [getattr(a, k) for k in AGENT_STATE] + list(a._adam_actor) + list(a._adam_critic)


def assert_agents_equal(got, want):
    for p, (a, b) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(agent_tensors(a), agent_tensors(b))):
            assert torch.equal(x, y), (p, k)


def assert_losses_equal(got, want):
    assert [l is None for l in got] == [l is None for l in want]
    assert all(torch.equal(x, y) for x, y in zip(got, want) if x is not None)


def _population_vs_agents(ssc, agents, twins, fused, records=(256, 256, 40, 200), kept=None):
    """three train_from calls against the twins' own; ``kept``: a list that gets, per call, every one-workgroup group's
    DeviceItems (items, sampling keys)"""
    replays, twin_replays = ([make_replay(ssc, p, n) for p, n in enumerate(records)] for _ in range(2))
    untouched = [t.clone() for t in agent_tensors(agents[2])]
    pop = ssc.DDPGPopulation(agents)
    for call in range(3):          # the second and third call reuse the descriptors
        got = pop.train_from(replays, copy=True)
        assert pop.fused is fused
        if kept is not None:
            kept.append([(g.items, g.draw.keys) for g in pop._groups])
        want = [a.train_from(r) for a, r in zip(twins, twin_replays)]
        assert_losses_equal(got, want)
        assert got[2] is None and [g.shape[0] for g in got if g is not None] == [a.num_train_iterations for a in agents[:2] + agents[3:]]
        assert_agents_equal(agents, twins)
        assert [r._batches_drawn for r in replays] == [r._batches_drawn for r in twin_replays]
    assert replays[0]._batches_drawn == 3 * agents[0].num_train_iterations and replays[2]._batches_drawn == 0
    assert all(torch.equal(x, y) for x, y in zip(agent_tensors(agents[2]), untouched))     # the ring below batch_size
    return pop, replays, twin_replays


def test_population_train_from_is_bitwise_the_agents_own(ssc):
    from smartstartcontinuous_amd.population import DeviceItems
    agents, twins = ([make_agent(ssc, p) for p in range(4)] for _ in range(2))
    kept = []
    pop, replays, twin_replays = _population_vs_agents(ssc, agents, twins, True, kept=kept)
    assert len(kept[0]) == 1 and all(isinstance(x, DeviceItems) for x in kept[0][0])
    for later in kept[1:]:                 # the second and third calls: the same descriptors, only the keys uploaded
        assert len(later) == 1 and all(x is y for x, y in zip(later[0], kept[0][0]))
    # a ring fills up: the descriptors are rebuilt and the third agent joins
    replays[2].count = twin_replays[2].count = 64
    got = pop.train_from(replays, n_iters=2)
    want = [a.train_from(r, 2) for a, r in zip(twins, twin_replays)]
    assert pop.fused is True and got[2] is not None
    assert_losses_equal(got, want)
    assert_agents_equal(agents, twins)
    # the index-explicit form
    idx = [r.sample_indices(k, 64) for r, k in zip(twin_replays, (1, 0, 2, 3))]
    views = [(r.s, r.a, r.r, r.t, r.s2) for r in replays]
    got = pop.train_on(views, idx, (1, 0, 2, 3))
    want = [a.train_on(r.s, r.a, r.r, r.t, r.s2, i, k) if k else None for a, r, i, k in zip(twins, twin_replays, idx, (1, 0, 2, 3))]
    assert pop.fused is True
    assert_losses_equal(got, want)
    assert_agents_equal(agents, twins)


def test_population_with_statistics_is_fused(ssc):
    agents, twins = ([make_agent(ssc, p, normalize_observations=True) for p in range(4)] for _ in range(2))
    rows = np.random.default_rng(4).uniform(-1.2, 0.6, (4, 300, 2)).astype(np.float32)
    for p in range(4):
        agents[p].obs_rms.update_rows(rows[p]); twins[p].obs_rms.update_rows(rows[p])
    _population_vs_agents(ssc, agents, twins, True)


def test_population_with_another_shape_falls_back(ssc):
    agents, twins = ([make_agent(ssc, p, h=(128, 64) if p == 1 else (64, 32)) for p in range(4)] for _ in range(2))
    _population_vs_agents(ssc, agents, twins, False)


def test_population_with_mixed_statistics_falls_back(ssc):
    agents, twins = ([make_agent(ssc, p, normalize_observations=p == 3) for p in range(4)] for _ in range(2))
    _population_vs_agents(ssc, agents, twins, False)


def test_population_respects_the_path_switch(ssc, monkeypatch):
    agents, twins = ([make_agent(ssc, p) for p in range(4)] for _ in range(2))
    monkeypatch.setenv("SSC_DDPG_WIDE", "1")
    pop, replays, twin_replays = _population_vs_agents(ssc, agents, twins, False)
    monkeypatch.delenv("SSC_DDPG_WIDE")
    pop.train_from(replays)
    assert pop.fused is True


# ---- the loop ----------------------------------------------------------------------------------------------------------
def _loop_pairs(ssc, mixed):
    envs = [ssc.VecEnv("MountainCarContinuous-v0", 64, seed=20 + p, max_episode_steps=20) for p in range(3)]
    for e in envs:
        e.reset()
    agents = [make_agent(ssc, p, normalize_observations=mixed and p == 1, reward_scale=0.5 + 0.25 * p, num_train_iterations=5) for p in range(3)]
    return envs, agents


@pytest.mark.parametrize("mixed", [True, False])
def test_population_loop_is_bitwise_the_single_loops(ssc, mixed, monkeypatch):
    """P = 3 pairs of 64 envs, 4 chunks of 16 steps, 3 iterations per chunk on rings of 4096: parameters, losses, Summary
    records and the final epsilon equal three separate rl_train_vec_ddpg runs.  ``mixed``: one agent normalises its
    observations, so the population trains agent by agent; otherwise in one launch."""
    from smartstartcontinuous_amd import agents as agents_mod
    ways = []
    inner = agents_mod.DDPGPopulation.train_from

    def spy(self, *a, **kw):
        out = inner(self, *a, **kw)
        ways.append(self.fused)
        return out
    monkeypatch.setattr(agents_mod.DDPGPopulation, "train_from", spy)
    kw = dict(num_chunks=4, chunk_steps=16, train_iters=3, replay_capacity=4096)
    envs, agents = _loop_pairs(ssc, mixed)
    got = ssc.rl_train_vec_ddpg_population(envs, agents, seed=[3, 4, 5], **kw)
    assert ways == [not mixed] * 4
    t_envs, twins = _loop_pairs(ssc, mixed)
    for p in range(3):
        summary, losses, replay = ssc.rl_train_vec_ddpg(t_envs[p], twins[p], seed=3 + p, **kw)
        g_summary, g_losses, g_replay = got[p]
        assert len(losses) == 4 and len(g_losses) == 4 and all(torch.equal(x, y) for x, y in zip(g_losses, losses))
        assert g_summary.episodes == summary.episodes and len(summary.episodes) == 3 * 64
        assert g_summary.dropped_episode_records == summary.dropped_episode_records == 0
        assert g_replay.count == replay.count and g_replay._batches_drawn == replay._batches_drawn == 12
        assert torch.equal(g_replay.s, replay.s) and torch.equal(g_replay.r, replay.r)
        assert agents[p].decaying_ou_action_noise.epsilon == twins[p].decaying_ou_action_noise.epsilon < 1.0
        if twins[p].obs_rms is not None:
            assert torch.equal(agents[p].obs_rms.block, twins[p].obs_rms.block)
    assert_agents_equal(agents, twins)


def test_population_loop_refuses_what_it_does_not_do(ssc):
    envs, agents = _loop_pairs(ssc, False)
    for kw in (dict(overlap=True), dict(stats_every=2), dict(eval_env=envs[0], eval_every=1)):
        with pytest.raises(NotImplementedError):
            ssc.rl_train_vec_ddpg_population(envs, agents, 1, chunk_steps=4, **kw)
    noisy = agents[:2] + [make_agent(ssc, 2, param_noise_stddev=0.1)]
    with pytest.raises(NotImplementedError):
        ssc.rl_train_vec_ddpg_population(envs, noisy, 1, chunk_steps=4)
    with pytest.raises(ValueError):
        ssc.rl_train_vec_ddpg_population(envs[:2], agents, 1)
