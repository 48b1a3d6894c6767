"""A population of ANY mix of shapes on the multi-workgroup learner in grouped launches (ssc_ddpg_train_many_wide, the
three-way routing of DDPGPopulation, rl_train_vec_ddpg_population on mixed layer sizes).  Every result is DEFINED as what
ssc_ddpg_train_ws / ssc_ddpg_train_ws_rms gives agent by agent, so the comparisons are torch.equal: no tolerance.  One
agent is also held to the fp64 oracle directly, through the existing learner helper and its tolerances, so that the file
does not rest on the twin alone.

The ABI tests drive the C entry points on arrays of their own, every array, workspace and loss block between guard bands."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import rms_edge_stats
from tests.test_gpu_ddpg_many import (_population_vs_agents, assert_agents_equal, make_agent, make_replay)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = 64                    # guard floats either side of every array
GB = 256                  # guard bytes either side of every workspace
SENT = -12345.0
SENT_I = 0x5A5A5A5A
SENT_B = 0x5A
CAP = 256
ARRAYS = ("actor", "critic", "target_actor", "target_critic", "adam_m_actor", "adam_v_actor", "adam_m_critic", "adam_v_critic")

# the issue's population: (actor, critic, batch, obs_dim, last_layer_tanh, layer_norm, critic_l2_reg, clip_norm, n_iters)
SPECS = [
    ((128, 64), (64, 32), 64, 2, 1, 0, 0.0, 0.0, 3),        # a
    ((200, 100), (200, 100), 17, 2, 1, 0, 0.0, 0.0, 1),     # b: two tiles, the second with one valid row; LDS above 64 KB
    ((7, 5), (9, 3), 16, 3, 0, 0, 0.0, 0.0, 2),             # c: sizes off every tile multiple
    ((64, 32), (64, 32), 48, 2, 1, 1, 0.0, 0.0, 2),         # d: LayerNorm
    ((64, 32), (64, 32), 64, 2, 1, 0, 1e-2, 0.5, 3),        # e: critic_l2_reg and clip_norm
    ((128, 64), (128, 64), 256, 2, 1, 0, 0.0, 0.5, 1),      # f: clip_norm only
    ((128, 64), (128, 64), 64, 2, 1, 0, 0.0, 0.0, 0),       # g: nothing to do; its arrays are sentinel and stay so
]
N_MAX = 3


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


def n_params(obs, h1, h2, out, extra, ln):
    return obs * h1 + h1 + (h1 + extra) * h2 + h2 + h2 * out + out + (2 * (h1 + h2) if ln else 0)


class WidePop:
    """The agents of SPECS as raw arrays: distinct parameters, non-zero Adam moments and step counters, distinct gamma /
    tau / learning rates, a ring of CAP random records (one in ten terminal), N_MAX index batches and a workspace each."""

    def __init__(self, ffi, seed=0, stats=()):
        self.specs, self.P = SPECS, len(SPECS)
        rng = np.random.default_rng(2000 + seed)
        lib = ffi.lib()
        dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
        self.T, self.n, self.ring, self.idx, self.rms = [], [], [], [], []
        for p, (A, C, B, O, llt, ln, l2, clip, n_it) in enumerate(SPECS):
            na, nc = n_params(O, A[0], A[1], 1, 0, ln), n_params(O, C[0], C[1], 1, 1, ln)
            n = dict(actor=na, target_actor=na, adam_m_actor=na, adam_v_actor=na, critic=nc, target_critic=nc, adam_m_critic=nc, adam_v_critic=nc)
            T = {}
            for name in ARRAYS:
                full = np.full(G + pad4(n[name]) + G, SENT, np.float32)
                if n_it > 0:
                    full[G:G + n[name]] = (1e-3 * rng.normal(size=n[name]) if "adam_m" in name else 1e-6 * rng.random(n[name]) if "adam_v" in name
                                           else rng.uniform(-0.3, 0.3, n[name]))
                T[name] = dev(full, torch.float32)
            t = np.full(12, SENT_I, np.int32)
            if n_it > 0:
                t[4:6] = rng.integers(0, 40, 2)
            T["adam_t"] = dev(t, torch.int32)
            losses = np.full(2 * G + 2 * (N_MAX + 2), SENT, np.float32)
            losses[G:G + 2 * (N_MAX + 2)] = np.nan
            T["losses"] = dev(losses, torch.float32)
            self.T.append(T)
            self.n.append(n)
            block, (lo, hi) = (None, (-1.2, 0.6))
            if p in stats:
                r, (lo, hi) = rms_edge_stats(O, "floor" if p == 2 else "wide")
                block = r.block.clone()
            self.rms.append(block)
            s = rng.uniform(lo, hi, (CAP, O))
            self.ring.append((dev(s, torch.float32), dev(rng.uniform(-1, 1, (CAP, 1)), torch.float32), dev(0.5 * rng.normal(size=CAP), torch.float32),
                              dev(rng.random(CAP) < 0.1, torch.uint8), dev(s + 0.01 * rng.normal(size=s.shape), torch.float32)))
            self.idx.append(dev(np.stack([rng.permutation(CAP)[:B] for _ in range(N_MAX)]), torch.int32))
        self.hyper = [dict(gamma=0.9 + 0.02 * (p % 5), tau=0.001 * (1 + p % 4), actor_lr=1e-4 * (1 + p % 3), critic_lr=1e-3 / (1 + p % 2))
                      for p in range(self.P)]
        self.ws = []
        for p in range(self.P):
            need = int(lib.ssc_ddpg_train_workspace_bytes(ctypes.byref(self.desc(ffi, p))))
            self.ws.append(torch.full((GB + need + GB,), SENT_B, dtype=torch.uint8, device="cuda"))

    def clone(self):
        import copy
        other = copy.copy(self)
        other.T = [{k: v.clone() for k, v in T.items()} for T in self.T]     # rings, indices, statistics: read-only, shared
        other.ws = [w.clone() for w in self.ws]
        return other

    def view(self, name, p):
        if name == "adam_t":
            return self.T[p][name][4:6]
        if name == "losses":
            return self.T[p][name][G:G + 2 * (N_MAX + 2)].view(-1, 2)
        return self.T[p][name][G:G + self.n[p][name]]

    def desc(self, ffi, p):
        A, C, B, O, llt, ln, l2, clip, _ = self.specs[p]
        d = ffi.DdpgDesc()
        d.obs_dim, d.act_dim, d.actor_h1, d.actor_h2, d.critic_h1, d.critic_h2 = O, 1, A[0], A[1], C[0], C[1]
        d.last_layer_tanh, d.batch_size, d.layer_norm, d.critic_l2_reg, d.clip_norm = llt, B, ln, l2, clip
        for name in ARRAYS + ("adam_t",):
            setattr(d, name, self.view(name, p).data_ptr())
        for k, v in self.hyper[p].items():
            setattr(d, k, v)
        d.beta1, d.beta2, d.epsilon, d.obs_clip = 0.9, 0.999, 1e-8, 5.0
        return d

    def replay(self, ffi, p):
        return ffi.ReplayView(*(x.data_ptr() for x in self.ring[p]), CAP)

    def workspace(self, p):
        return self.ws[p][GB:self.ws[p].numel() - GB]

    def train_single(self, ffi, p):
        """what agent.train_on calls today"""
        n = self.specs[p][8]
        if n == 0:
            return
        d, rv, ws, lib = self.desc(ffi, p), self.replay(ffi, p), self.workspace(p), ffi.lib()
        if self.rms[p] is None:
            ffi.check(lib.ssc_ddpg_train_ws(ctypes.byref(d), ctypes.byref(rv), ffi.ptr(self.idx[p]), n, ffi.ptr(self.view("losses", p)),
                                            ffi.ptr(ws), ws.numel(), ffi.stream()))
        else:
            ffi.check(lib.ssc_ddpg_train_ws_rms(ctypes.byref(d), ctypes.byref(rv), ffi.ptr(self.idx[p]), n, ffi.ptr(self.view("losses", p)),
                                                ffi.ptr(ws), ws.numel(), ffi.stream(), ffi.ptr(self.rms[p])))

    def plan(self, ffi):
        lib = ffi.lib()
        items = (ffi.DdpgManyWideItem * self.P)()
        for p, it in enumerate(items):
            it.ddpg, it.replay = self.desc(ffi, p), self.replay(ffi, p)
            it.d_batch_idx, it.d_losses = self.idx[p].data_ptr(), self.view("losses", p).data_ptr()
            it.d_rms = None if self.rms[p] is None else self.rms[p].data_ptr()
            it.n_iters = self.specs[p][8]
            it.d_workspace, it.workspace_bytes = self.workspace(p).data_ptr(), self.workspace(p).numel()
        nbytes = int(lib.ssc_ddpg_train_many_wide_plan_bytes(self.P))
        h_plan = torch.full((nbytes + 2 * GB,), SENT_B, dtype=torch.uint8)
        ffi.check(lib.ssc_ddpg_train_many_wide_plan(ctypes.addressof(items), self.P, h_plan[GB:].data_ptr(), nbytes))
        assert bool((h_plan[:GB] == SENT_B).all()) and bool((h_plan[GB + nbytes:] == SENT_B).all())      # the builder stays inside
        h_plan = h_plan[GB:GB + nbytes].clone()
        return items, h_plan, h_plan.cuda()

    def train_many(self, ffi, plan):
        items, h_plan, d_plan = plan
        ffi.check(ffi.lib().ssc_ddpg_train_many_wide(ctypes.addressof(items), h_plan.data_ptr(), d_plan.data_ptr(), self.P, ffi.stream()))
        torch.cuda.synchronize()

    def assert_equal(self, other):
        for p in range(self.P):
            for name in self.T[p]:
                a, b = self.T[p][name], other.T[p][name]
                if name == "losses":                     # NaN where no iteration wrote
                    assert torch.equal(torch.isnan(a), torch.isnan(b)), (p, name)
                    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
                assert torch.equal(a, b), (p, name)

    def assert_guards(self):
        for p in range(self.P):
            for name, t in self.T[p].items():
                if name == "adam_t":
                    assert bool((t[:4] == SENT_I).all()) and bool((t[6:] == SENT_I).all()), (p, name)
                    continue
                n = 2 * (N_MAX + 2) if name == "losses" else self.n[p][name]
                assert bool((t[:G] == SENT).all()) and bool((t[G + n:] == SENT).all()), (p, name)
            w = self.ws[p]
            assert bool((w[:GB] == SENT_B).all()) and bool((w[w.numel() - GB:] == SENT_B).all()), (p, "workspace")


@pytest.mark.parametrize("stats", [(), (0, 2, 4)], ids=["plain", "statistics_on_a_c_e"])
def test_grouped_launches_are_bitwise_the_single_launches(ssc, stats):
    """The seven agents of the issue, n_iters (3, 1, 2, 2, 3, 1, 0), in ONE ssc_ddpg_train_many_wide call: parameters,
    targets, the four Adam moment arrays, adam_t and the losses of every agent equal those of its copy trained alone by
    ssc_ddpg_train_ws (with statistics on a, c and e: ssc_ddpg_train_ws_rms, so both gradient groups run).  Guard bands
    around every array, workspace and loss block are intact; a second call on the same plan continues the chain."""
    ffi = ssc._ffi
    pop = WidePop(ffi, seed=len(stats), stats=stats)
    ref, before = pop.clone(), pop.clone()
    plan = pop.plan(ffi)
    for call in range(2):
        for p in range(pop.P):
            ref.train_single(ffi, p)
        pop.train_many(ffi, plan)
        pop.assert_equal(ref)
        pop.assert_guards()
        for p, spec in enumerate(SPECS):
            n = spec[8]
            assert [int(x) for x in pop.view("adam_t", p) - before.view("adam_t", p)] == [(call + 1) * n] * 2, p
            rows = pop.view("losses", p)
            assert bool(torch.isfinite(rows[:n]).all()) and bool(torch.isnan(rows[n:]).all()), p
    assert all(not torch.equal(pop.view(name, p), before.view(name, p)) for name in ARRAYS for p in range(6))      # they trained
    for name in ARRAYS + ("adam_t",):                                                                               # g did not
        assert torch.equal(pop.T[6][name], before.T[6][name]) and bool((pop.view(name, 6) == (SENT_I if name == "adam_t" else SENT)).all())
    assert [int(x) for x in pop.view("adam_t", 0) - before.view("adam_t", 0)] == [6, 6]                             # 3 + 3


def test_a_grouped_agent_against_the_fp64_oracle(ssc, monkeypatch):
    """Agent b's shape (200-100 / 200-100, batch 17: LDS above 64 KB, a tile with one valid row) after ONE iteration in a
    grouped launch, held to the fp64 learner oracle by the helper and at the tolerances the plain multi-workgroup learner is
    held to (tests/test_gpu_agents.py::_ddpg_kernel_vs_oracle): the helper's ``agent.train_on`` goes
    through a two-agent population whose other member is a 128-64 agent on a ring of its own."""
    from smartstartcontinuous_amd import agents as agents_mod
    from tests.test_gpu_agents import _ddpg_kernel_vs_oracle
    ways, seen = [], []
    mate, mate_replay = make_agent(ssc, 1, h=(128, 64)), make_replay(ssc, 1)
    mate_idx = mate_replay.sample_indices(1, 64)

    def through_a_population(self, s, a, r, t, s2, batch_idx, n_iters, obs_rms=None):
        assert obs_rms is None and n_iters == 1
        pop = agents_mod.DDPGPopulation([self, mate])
        m = mate_replay
        out = pop.train_on([(s, a, r, t, s2), (m.s, m.a, m.r, m.t, m.s2)], [batch_idx, mate_idx], [1, 1], copy=True)
        ways.append(pop.ways)
        seen.append((self.h1, self.h2, self.batch_size))
        return out[0]
    monkeypatch.setattr(agents_mod.DDPG_Baselines_agent, "train_on", through_a_population)
    _ddpg_kernel_vs_oracle(ssc, 2, 200, 100, B=17, n_iters=1, cap=256)
    assert ways == [("wide", "wide")] * 2 and seen == [(200, 100, 17)] * 2          # last_layer_tanh on and off


# ---- DDPGPopulation on agent objects ---------------------------------------------------------------------------------
def agent_of(ssc, p, actor=(64, 32), critic=None, batch_size=64, **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    critic = critic or actor
    kw.setdefault("num_train_iterations", 1 + p % 3)
    return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, batch_size=batch_size, actor_h1=actor[0], actor_h2=actor[1],
                                critic_h1=critic[0], critic_h2=critic[1], lastLayerTanh=True, seed=40 + p, actor_lr=1e-4 * (1 + p),
                                critic_lr=1e-3 / (1 + p), gamma=0.99 - 0.01 * p, tau=0.001 * (1 + p), **kw)


def with_statistics(agents, twins, which):
    rows = np.random.default_rng(4).uniform(-1.2, 0.6, (len(agents), 300, 2)).astype(np.float32)
    for p in which:
        agents[p].obs_rms.update_rows(rows[p]); twins[p].obs_rms.update_rows(rows[p])


MIXED = [((64, 32), None), ((128, 64), None), ((64, 32), None), ((200, 100), (128, 64))]


@pytest.fixture
def single_agent_calls(ssc, monkeypatch):
    """-> the names of the single-agent learner entry points called from INSIDE DDPGPopulation.train_from / train_on (the
    twins call them too, outside)"""
    from smartstartcontinuous_amd import agents as agents_mod
    lib, calls, inside = ssc._ffi.lib(), [], [0]
    for name in ("ssc_ddpg_train", "ssc_ddpg_train_ws", "ssc_ddpg_train_ws_rms", "ssc_ddpg_train_ws_popart"):
        def spy(*a, _fn=getattr(lib, name), _name=name):
            if inside[0]:
                calls.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, spy)
    for name in ("train_from", "train_on"):
        def wrapped(self, *a, _fn=getattr(agents_mod.DDPGPopulation, name), **kw):
            inside[0] += 1
            try:
                return _fn(self, *a, **kw)
            finally:
                inside[0] -= 1
        monkeypatch.setattr(agents_mod.DDPGPopulation, name, wrapped)
    return calls


def test_population_of_mixed_shapes_is_split_three_ways(ssc, single_agent_calls):
    """[64-32, 128-64, 64-32, 200-100 / 128-64]: the two wide agents in the grouped launches, the two of the shipped shape
    (one of them on a ring below batch_size) through ssc_ddpg_train_many, no single-agent call at all."""
    agents, twins = ([agent_of(ssc, p, *MIXED[p]) for p in range(4)] for _ in range(2))
    pop, replays, twin_replays = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("one_workgroup", "wide", "one_workgroup", "wide") and pop.fused is False
    assert single_agent_calls == []
    # the index-explicit form, on the same split (the third ring has filled up meanwhile)
    replays[2].count = twin_replays[2].count = 64
    idx = [r.sample_indices(k, 64) for r, k in zip(twin_replays, (1, 0, 2, 3))]
    views = [(r.s, r.a, r.r, r.t, r.s2) for r in replays]
    got = pop.train_on(views, idx, (1, 0, 2, 3))
    want = [a.train_on(r.s, r.a, r.r, r.t, r.s2, i, k) if k else None for a, r, i, k in zip(twins, twin_replays, idx, (1, 0, 2, 3))]
    assert pop.ways == ("one_workgroup", "wide", "one_workgroup", "wide") and single_agent_calls == []
    assert [g is None for g in got] == [w is None for w in want] and all(torch.equal(g, w) for g, w in zip(got, want) if g is not None)
    assert_agents_equal(agents, twins)


def test_population_under_the_wide_switch_is_all_wide(ssc, monkeypatch, single_agent_calls):
    monkeypatch.setenv("SSC_DDPG_WIDE", "1")
    agents, twins = ([make_agent(ssc, p) for p in range(4)] for _ in range(2))
    pop, replays, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("wide",) * 4 and single_agent_calls == []
    monkeypatch.delenv("SSC_DDPG_WIDE")
    pop.train_from(replays)
    assert pop.fused is True and pop.ways == ("one_workgroup",) * 4


@pytest.mark.parametrize("shape", [(128, 64), (64, 32)])
def test_population_with_mixed_statistics_is_grouped(ssc, shape, single_agent_calls):
    """Statistics on agent 3 only: among wide agents it runs in the statistics instantiation of the gradient launch, the
    others in the plain one; among agents of the shipped shape it is a one-workgroup group of its own.  Each equals its twin."""
    agents, twins = ([agent_of(ssc, p, shape, normalize_observations=p == 3) for p in range(4)] for _ in range(2))
    with_statistics(agents, twins, [3])
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == (("wide",) * 4 if shape == (128, 64) else ("one_workgroup",) * 4) and single_agent_calls == []
    if shape == (64, 32):
        assert sorted(g.ps for g in pop._groups if g.way == "one_workgroup") == [[0, 1, 2], [3]]


@pytest.mark.parametrize("which", ["mixed", "wide_switch", "statistics"])
def test_switch_off_is_the_per_agent_fallback(ssc, which, monkeypatch):
    """POPULATION_GROUPED_WIDE = False: the same populations, the same bits, every agent alone."""
    from smartstartcontinuous_amd import agents as agents_mod
    monkeypatch.setattr(agents_mod, "POPULATION_GROUPED_WIDE", False)
    if which == "wide_switch":
        monkeypatch.setenv("SSC_DDPG_WIDE", "1")
    if which == "statistics":
        agents, twins = ([agent_of(ssc, p, (128, 64), normalize_observations=p == 3) for p in range(4)] for _ in range(2))
        with_statistics(agents, twins, [3])
    else:
        agents, twins = ([agent_of(ssc, p, *(MIXED[p] if which == "mixed" else ((64, 32), None))) for p in range(4)] for _ in range(2))
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("alone",) * 4


def test_a_popart_agent_trains_alone_the_rest_grouped(ssc, single_agent_calls):
    kw = [dict(), dict(normalize_returns=True, enable_popart=True), dict(), dict()]
    agents, twins = ([agent_of(ssc, p, (128, 64), **kw[p]) for p in range(4)] for _ in range(2))
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("wide", "alone", "wide", "wide")
    assert set(single_agent_calls) == {"ssc_ddpg_train_ws_popart"}
    assert torch.equal(agents[1].ret_rms.block, twins[1].ret_rms.block)


def test_a_lone_wide_agent_trains_alone(ssc):
    agents, twins = ([agent_of(ssc, p, (128, 64) if p == 1 else (64, 32)) for p in range(4)] for _ in range(2))
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("one_workgroup", "alone", "one_workgroup", "one_workgroup")


# ---- the loop ----------------------------------------------------------------------------------------------------------
def _loop_pairs(ssc):
    envs = [ssc.VecEnv("MountainCarContinuous-v0", 64, seed=20 + p, max_episode_steps=20) for p in range(3)]
    for e in envs:
        e.reset()
    shapes = [(64, 32), (128, 64), (200, 100)]
    return envs, [agent_of(ssc, p, shapes[p], reward_scale=0.5 + 0.25 * p, num_train_iterations=5) for p in range(3)]


def test_population_loop_on_mixed_layer_sizes_is_bitwise_the_single_loops(ssc, monkeypatch):
    """P = 3 pairs of 64 envs with hidden sizes 64-32 / 128-64 / 200-100, 4 chunks of 16 steps, 3 iterations per chunk on
    rings of 4096: parameters, losses, Summary records and the final epsilon equal three separate rl_train_vec_ddpg runs."""
    from smartstartcontinuous_amd import agents as agents_mod
    ways = []
    inner = agents_mod.DDPGPopulation.train_from

    def spy(self, *a, **kw):
        out = inner(self, *a, **kw)
        ways.append(self.ways)
        return out
    monkeypatch.setattr(agents_mod.DDPGPopulation, "train_from", spy)
    kw = dict(num_chunks=4, chunk_steps=16, train_iters=3, replay_capacity=4096)
    envs, agents = _loop_pairs(ssc)
    got = ssc.rl_train_vec_ddpg_population(envs, agents, seed=[3, 4, 5], **kw)
    assert ways == [("one_workgroup", "wide", "wide")] * 4
    t_envs, twins = _loop_pairs(ssc)
    for p in range(3):
        summary, losses, replay = ssc.rl_train_vec_ddpg(t_envs[p], twins[p], seed=3 + p, **kw)
        g_summary, g_losses, g_replay = got[p]
        assert len(losses) == 4 and len(g_losses) == 4 and all(torch.equal(x, y) for x, y in zip(g_losses, losses))
        assert g_summary.episodes == summary.episodes and len(summary.episodes) == 3 * 64
        assert g_summary.dropped_episode_records == summary.dropped_episode_records == 0
        assert g_replay.count == replay.count and g_replay._batches_drawn == replay._batches_drawn == 12
        assert torch.equal(g_replay.s, replay.s) and torch.equal(g_replay.r, replay.r)
        assert agents[p].decaying_ou_action_noise.epsilon == twins[p].decaying_ou_action_noise.epsilon < 1.0
    assert_agents_equal(agents, twins)
