"""Pop-Art agents of any mix of shapes in grouped launches (ssc_ddpg_train_many_popart, the "wide_popart" route of
DDPGPopulation, rl_train_vec_ddpg_population on Pop-Art pairs).  Every result is DEFINED as what ssc_ddpg_train_ws_popart
gives agent by agent, so the comparisons are torch.equal: no tolerance.  One grouped agent is also held to the fp64
restatement of tests/popart_cases.py at the tolerances of tests/test_gpu_ddpg_popart.py, so that the file does not rest
on the twin alone.

The ABI tests drive the C entry points on arrays of their own, every array, workspace, loss block and ret_rms block
between guard bands."""
import copy
import ctypes

import numpy as np
import pytest

from tests.gpu_util import rms_edge_stats
from tests.test_gpu_ddpg_many import _population_vs_agents, assert_agents_equal
from tests.test_gpu_ddpg_many_wide import (ARRAYS, CAP, G, GB, SENT, SENT_B, SENT_I, agent_of, n_params, pad4,
                                           single_agent_calls)  # noqa: F401  (a fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# the issue's population: (actor, critic, batch, obs_dim, last_layer_tanh, layer_norm, critic_l2_reg, clip_norm, n_iters)
SPECS = [
    ((128, 64), (64, 32), 64, 2, 1, 0, 0.0, 0.0, 3),        # a
    ((200, 100), (200, 100), 17, 2, 1, 0, 0.0, 0.0, 1),     # b: two tiles, the second with one valid row; LDS above 64 KB
    ((7, 5), (9, 3), 16, 3, 0, 0, 0.0, 0.0, 2),             # c: sizes off every tile multiple
    ((64, 32), (64, 32), 48, 2, 1, 1, 0.0, 0.0, 2),         # d: LayerNorm
    ((64, 32), (64, 32), 64, 2, 1, 0, 1e-2, 0.5, 3),        # e: critic_l2_reg and clip_norm
    ((64, 32), (64, 32), 64, 2, 1, 0, 0.0, 0.0, 2),         # f: the shipped shape
    ((128, 64), (128, 64), 64, 2, 1, 0, 0.0, 0.0, 0),       # g: nothing to do; its arrays and its block are sentinel and stay so
]
WARM = (1, 3, 5)          # ret_rms blocks warmed with 200 returns from N(-20, 6); the others fresh (0, 1e-2, 1e-2)
N_MAX = 3
GD = 8                    # guard doubles either side of a ret_rms block


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


@pytest.fixture
def min_group_two(monkeypatch):
    """the routing asserts do not depend on the measured minimum"""
    from smartstartcontinuous_amd import agents as agents_mod
    monkeypatch.setattr(agents_mod, "POPULATION_POPART_MIN_GROUP", 2)
    return agents_mod


class PopartPop:
    """The agents of SPECS as raw arrays: distinct parameters, non-zero Adam moments and step counters, distinct gamma /
    tau / learning rates, a ring of CAP random records (one in ten terminal), N_MAX index batches, a Pop-Art workspace and
    a ret_rms block each."""

    def __init__(self, ffi, seed=0, stats=()):
        self.P = len(SPECS)
        rng = np.random.default_rng(3000 + seed)
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
            block = np.full(GD + 3 + GD, SENT, np.float64)
            if n_it > 0:
                block[GD:GD + 3] = (0.0, 1e-2, 1e-2)
                if p in WARM:
                    y = rng.normal(-20.0, 6.0, 200).astype(np.float32).astype(np.float64)
                    block[GD:GD + 3] += (y.sum(), np.square(y).sum(), 200.0)
            T["ret_rms"] = dev(block, torch.float64)
            self.T.append(T)
            self.n.append(n)
            obs_block, (lo, hi) = (None, (-1.2, 0.6))
            if p in stats:
                r, (lo, hi) = rms_edge_stats(O, "floor" if p == 2 else "wide")
                obs_block = r.block.clone()
            self.rms.append(obs_block)
            s = rng.uniform(lo, hi, (CAP, O))
            self.ring.append((dev(s, torch.float32), dev(rng.uniform(-1, 1, (CAP, 1)), torch.float32), dev(0.5 * rng.normal(size=CAP), torch.float32),
                              dev(rng.random(CAP) < 0.1, torch.uint8), dev(s + 0.01 * rng.normal(size=s.shape), torch.float32)))
            self.idx.append(dev(np.stack([rng.permutation(CAP)[:B] for _ in range(N_MAX)]), torch.int32))
        self.hyper = [dict(gamma=0.9 + 0.02 * (p % 5), tau=0.001 * (1 + p % 4), actor_lr=1e-4 * (1 + p % 3), critic_lr=1e-3 / (1 + p % 2))
                      for p in range(self.P)]
        self.ws, self.tail0 = [], []
        for p in range(self.P):
            d = self.desc(ffi, p)
            need = int(lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d)))
            self.tail0.append((int(lib.ssc_ddpg_train_workspace_bytes(ctypes.byref(d))) + 255) // 256 * 256)
            self.ws.append(torch.full((GB + need + GB,), SENT_B, dtype=torch.uint8, device="cuda"))

    def clone(self):
        other = copy.copy(self)
        other.T = [{k: v.clone() for k, v in T.items()} for T in self.T]     # rings, indices, obs statistics: read-only, shared
        other.ws = [w.clone() for w in self.ws]
        return other

    def view(self, name, p):
        if name == "adam_t":
            return self.T[p][name][4:6]
        if name == "losses":
            return self.T[p][name][G:G + 2 * (N_MAX + 2)].view(-1, 2)
        if name == "ret_rms":
            return self.T[p][name][GD:GD + 3]
        return self.T[p][name][G:G + self.n[p][name]]

    def desc(self, ffi, p):
        A, C, B, O, llt, ln, l2, clip, _ = SPECS[p]
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

    def popart_tail(self, p):
        """[y | partials | scalars] of the workspace, as the single call lays it out"""
        return self.workspace(p)[self.tail0[p]:]

    def train_single(self, ffi, p):
        """what agent.train_on calls today"""
        n = SPECS[p][8]
        if n == 0:
            return
        d, rv, ws, lib = self.desc(ffi, p), self.replay(ffi, p), self.workspace(p), ffi.lib()
        ffi.check(lib.ssc_ddpg_train_ws_popart(ctypes.byref(d), ctypes.byref(rv), ffi.ptr(self.idx[p]), n, ffi.ptr(self.view("losses", p)),
                                               ffi.ptr(ws), ws.numel(), ffi.stream(), None if self.rms[p] is None else ffi.ptr(self.rms[p]),
                                               ffi.ptr(self.view("ret_rms", p))))

    def plan(self, ffi):
        lib = ffi.lib()
        items = (ffi.DdpgManyPopartItem * self.P)()
        for p, it in enumerate(items):
            it.ddpg, it.replay = self.desc(ffi, p), self.replay(ffi, p)
            it.d_batch_idx, it.d_losses = self.idx[p].data_ptr(), self.view("losses", p).data_ptr()
            it.d_rms = None if self.rms[p] is None else self.rms[p].data_ptr()
            it.n_iters = SPECS[p][8]
            it.d_workspace, it.workspace_bytes = self.workspace(p).data_ptr(), self.workspace(p).numel()
            it.d_ret_rms = self.view("ret_rms", p).data_ptr()
        nbytes = int(lib.ssc_ddpg_train_many_popart_plan_bytes(self.P))
        h_plan = torch.full((nbytes + 2 * GB,), SENT_B, dtype=torch.uint8)
        ffi.check(lib.ssc_ddpg_train_many_popart_plan(ctypes.addressof(items), self.P, h_plan[GB:].data_ptr(), nbytes))
        assert bool((h_plan[:GB] == SENT_B).all()) and bool((h_plan[GB + nbytes:] == SENT_B).all())      # the builder stays inside
        h_plan = h_plan[GB:GB + nbytes].clone()
        return items, h_plan, h_plan.cuda()

    def train_many(self, ffi, plan):
        items, h_plan, d_plan = plan
        ffi.check(ffi.lib().ssc_ddpg_train_many_popart(ctypes.addressof(items), h_plan.data_ptr(), d_plan.data_ptr(), self.P, ffi.stream()))
        torch.cuda.synchronize()

    def assert_equal(self, other):
        for p in range(self.P):
            for name in self.T[p]:
                a, b = self.T[p][name], other.T[p][name]
                if name == "losses":                     # NaN where no iteration wrote
                    assert torch.equal(torch.isnan(a), torch.isnan(b)), (p, name)
                    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
                assert torch.equal(a, b), (p, name)
            assert torch.equal(self.popart_tail(p), other.popart_tail(p)), (p, "workspace tail")

    def assert_guards(self):
        for p in range(self.P):
            for name, t in self.T[p].items():
                if name == "adam_t":
                    assert bool((t[:4] == SENT_I).all()) and bool((t[6:] == SENT_I).all()), (p, name)
                    continue
                if name == "ret_rms":
                    assert bool((t[:GD] == SENT).all()) and bool((t[GD + 3:] == SENT).all()), (p, name)
                    continue
                n = 2 * (N_MAX + 2) if name == "losses" else self.n[p][name]
                assert bool((t[:G] == SENT).all()) and bool((t[G + n:] == SENT).all()), (p, name)
            w = self.ws[p]
            assert bool((w[:GB] == SENT_B).all()) and bool((w[w.numel() - GB:] == SENT_B).all()), (p, "workspace")


@pytest.mark.parametrize("stats", [(), (0, 2, 4)], ids=["plain", "statistics_on_a_c_e"])
def test_grouped_launches_are_bitwise_the_single_launches(ssc, stats):
    """The seven agents of the issue, n_iters (3, 1, 2, 2, 3, 2, 0), in ONE ssc_ddpg_train_many_popart call: parameters,
    targets, the four Adam moment arrays, adam_t, the losses, the ret_rms block and the Pop-Art tail of the workspace of
    every agent equal those of its copy trained alone by ssc_ddpg_train_ws_popart (with statistics on a, c and e both
    instantiations of the target and of the gradient launch run).  Guard bands around every array, workspace, loss block
    and ret_rms block are intact; a second call on the same plan continues the chain."""
    ffi = ssc._ffi
    pop = PopartPop(ffi, seed=len(stats), stats=stats)
    ref, before = pop.clone(), pop.clone()
    plan = pop.plan(ffi)
    for call in range(2):
        for p in range(pop.P):
            ref.train_single(ffi, p)
        pop.train_many(ffi, plan)
        pop.assert_equal(ref)
        pop.assert_guards()
        for p, spec in enumerate(SPECS):
            n, B = spec[8], spec[2]
            assert [int(x) for x in pop.view("adam_t", p) - before.view("adam_t", p)] == [(call + 1) * n] * 2, p
            rows = pop.view("losses", p)
            assert bool(torch.isfinite(rows[:n]).all()) and bool(torch.isnan(rows[n:]).all()), p
            if n > 0:
                count = float(before.view("ret_rms", p)[2])
                for _ in range((call + 1) * n):
                    count += float(B)
                assert float(pop.view("ret_rms", p)[2]) == count, p
    assert all(not torch.equal(pop.view(name, p), before.view(name, p)) for name in ARRAYS + ("ret_rms",) for p in range(6))   # they trained
    for name in ARRAYS + ("adam_t", "ret_rms"):                                                                        # g did not
        assert torch.equal(pop.T[6][name], before.T[6][name]) and bool((pop.view(name, 6) == (SENT_I if name == "adam_t" else SENT)).all())
    assert torch.equal(pop.ws[6], before.ws[6])


def test_same_bits_run_to_run(ssc):
    ffi = ssc._ffi
    start = PopartPop(ffi, seed=5, stats=(2,))
    runs = []
    for _ in range(2):
        pop = start.clone()
        pop.train_many(ffi, pop.plan(ffi))
        runs.append(pop)
    runs[0].assert_equal(runs[1])
    assert not torch.equal(runs[0].view("critic", 0), start.view("critic", 0))


def test_a_grouped_agent_against_the_fp64_restatement(ssc, min_group_two):
    """The shipped 64-32 x 64 shape ("64-32-b64-moving" of tests/test_gpu_ddpg_popart.py: the shape that has no
    one-workgroup kernel to fall back on) after six iterations in a grouped call whose other member is a 37-19 agent at
    batch 77 on rows of its own, held to PC.run_restatement at that test's tolerances: parameters and targets 5e-6, moments
    rtol 1e-3 / 2e-3, losses rtol 2e-4, count exact, sum / sumsq 2e-6 of sum |y| / sum y^2, y of the last iteration within
    1e-5 sqrt(h2 + 1) sigma_old + 4 * 2^-24 |y|."""
    from oracle import ssc_oracle as O
    from tests import popart_cases as PC
    from tests.test_gpu_ddpg_popart import TOL, device_rows, make_agent, state_of
    case, mate_case = PC.make_case(2, 64, 32, 64, "moving"), PC.make_case(8, 37, 19, 77, "moving")
    ref = PC.run_restatement(case)
    agent, mate = make_agent(case), make_agent(mate_case)
    idx = [torch.as_tensor(c["idx"], dtype=torch.int32, device="cuda").contiguous() for c in (case, mate_case)]
    pop = ssc.DDPGPopulation([agent, mate])
    losses = pop.train_on([device_rows(case), device_rows(mate_case)], idx, [PC.N_ITERS, PC.N_ITERS], copy=True)[0]
    torch.cuda.synchronize()
    assert pop.ways == ("wide_popart", "wide_popart")
    got = state_of(agent)
    ws = {k: v.cpu().numpy() for k, v in agent.popart_workspace().items()}
    B, h2 = case["B"], case["h2"]
    assert got["adam_t"].tolist() == [PC.N_ITERS, PC.N_ITERS]
    err = {k: float(np.max(np.abs(got[k] - O.flatten_params(ref[k])))) for k in ("actor", "critic", "target_actor", "target_critic")}
    print("max parameter errors", err, "block", got["block"].tolist(), "ref", ref["block"].tolist())
    got_l = losses.cpu().numpy()
    assert np.allclose(got_l, ref["losses"], rtol=2e-4, atol=1e-6), (got_l, ref["losses"])
    for k, e in err.items():
        assert e <= TOL, (k, e)
    for net in ("actor", "critic"):
        assert np.allclose(got["m_" + net], ref["adam"]["m_" + net], rtol=1e-3, atol=1e-7), "m_" + net
        assert np.allclose(got["v_" + net], ref["adam"]["v_" + net], rtol=2e-3, atol=1e-9), "v_" + net
    count = 1e-2
    for _ in range(PC.N_ITERS):
        count += float(B)
    assert got["block"][2] == count
    all_y = np.concatenate(ref["y"])
    assert abs(got["block"][0] - ref["block"][0]) <= 2e-6 * np.sum(np.abs(all_y))
    assert abs(got["block"][1] - ref["block"][1]) <= 2e-6 * np.sum(np.square(all_y))
    sg_old = ref["scalars"][-1][1]
    y_tol = 1e-5 * np.sqrt(h2 + 1) * sg_old + 4 * 2.0 ** -24 * np.abs(ref["y"][-1])
    assert np.all(np.abs(ws["y"] - ref["y"][-1]) <= y_tol), float(np.max(np.abs(ws["y"] - ref["y"][-1]) / y_tol))
    want_sc = np.asarray(ref["scalars"][-1])
    for j in (0, 2):
        assert abs(ws["scalars"][j] - want_sc[j]) <= 2e-6 * np.mean(np.abs(all_y)) + 2.0 ** -23 * abs(want_sc[j]), j
    assert np.allclose(ws["scalars"][[1, 3]], want_sc[[1, 3]], rtol=1e-5, atol=0)


# ---- DDPGPopulation on agent objects ---------------------------------------------------------------------------------
POPART = dict(normalize_returns=True, enable_popart=True)
MIXED = [((64, 32), None), ((128, 64), None), ((64, 32), None), ((200, 100), (128, 64))]


def warm(agents, twins):
    """every other agent's return statistics away from (0, 1)"""
    for p in range(1, len(agents), 2):
        rows = np.random.default_rng(3 + p).normal(-20.0, 6.0, (200, 1)).astype(np.float32)
        agents[p].ret_rms.update_rows(rows); twins[p].ret_rms.update_rows(rows)


def assert_blocks_equal(agents, twins):
    for p, (a, b) in enumerate(zip(agents, twins)):
        assert (a.ret_rms is None) == (b.ret_rms is None), p
        if a.ret_rms is not None:
            assert torch.equal(a.ret_rms.block, b.ret_rms.block), p


def test_popart_agents_of_mixed_shapes_are_grouped(ssc, min_group_two, single_agent_calls):
    """[64-32, 128-64, 64-32, 200-100 / 128-64], all Pop-Art, the third on a ring below batch_size: all four "wide_popart",
    no single-agent entry point called from inside the population; train_from over three calls and train_on equal the
    twins -- agents, losses, ret_rms.block, _batches_drawn -- and so does what agent.popart_workspace() reads."""
    agents, twins = ([agent_of(ssc, p, *MIXED[p], **POPART) for p in range(4)] for _ in range(2))
    warm(agents, twins)
    pop, replays, twin_replays = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("wide_popart",) * 4 and pop.fused is False
    assert single_agent_calls == []
    assert_blocks_equal(agents, twins)
    assert torch.equal(agents[2].ret_rms.block, torch.tensor([0.0, 1e-2, 1e-2], dtype=torch.float64, device="cuda"))   # below batch_size
    for p in (0, 1, 3):
        got, want = agents[p].popart_workspace(), twins[p].popart_workspace()
        assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want), p
    # the index-explicit form, on the same split (the third ring has filled up meanwhile)
    replays[2].count = twin_replays[2].count = 64
    idx = [r.sample_indices(k, 64) for r, k in zip(twin_replays, (1, 0, 2, 3))]
    views = [(r.s, r.a, r.r, r.t, r.s2) for r in replays]
    got = pop.train_on(views, idx, (1, 0, 2, 3))
    want = [a.train_on(r.s, r.a, r.r, r.t, r.s2, i, k) if k else None for a, r, i, k in zip(twins, twin_replays, idx, (1, 0, 2, 3))]
    assert pop.ways == ("wide_popart",) * 4 and single_agent_calls == []
    assert [g is None for g in got] == [w is None for w in want] and all(torch.equal(g, w) for g, w in zip(got, want) if g is not None)
    assert_agents_equal(agents, twins)
    assert_blocks_equal(agents, twins)
    got, want = agents[2].popart_workspace(), twins[2].popart_workspace()
    assert all(torch.equal(got[k], want[k]) for k in want)


def test_plain_and_popart_agents_each_make_their_own_call(ssc, min_group_two, single_agent_calls):
    """[plain 128-64, Pop-Art, Pop-Art, plain 200-100]: ("wide", "wide_popart", "wide_popart", "wide")"""
    shapes = [(128, 64), (64, 32), (128, 64), (200, 100)]
    kw = [dict(), POPART, POPART, dict()]
    agents, twins = ([agent_of(ssc, p, shapes[p], **kw[p]) for p in range(4)] for _ in range(2))
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("wide", "wide_popart", "wide_popart", "wide") and single_agent_calls == []
    assert_blocks_equal(agents, twins)
    assert float(agents[1].ret_rms.block[2]) > 1e-2


def test_switch_off_is_the_per_agent_fallback(ssc, min_group_two, monkeypatch):
    """POPULATION_GROUPED_WIDE = False: the same population, the same bits, every agent alone"""
    monkeypatch.setattr(min_group_two, "POPULATION_GROUPED_WIDE", False)
    agents, twins = ([agent_of(ssc, p, *MIXED[p], **POPART) for p in range(4)] for _ in range(2))
    warm(agents, twins)
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("alone",) * 4
    assert_blocks_equal(agents, twins)


def test_fewer_popart_agents_than_the_minimum_train_alone(ssc, monkeypatch):
    from smartstartcontinuous_amd import agents as agents_mod
    monkeypatch.setattr(agents_mod, "POPULATION_POPART_MIN_GROUP", 3)
    kw = [dict(), POPART, POPART, dict()]
    agents, twins = ([agent_of(ssc, p, (128, 64), **kw[p]) for p in range(4)] for _ in range(2))
    pop, _, _ = _population_vs_agents(ssc, agents, twins, False)
    assert pop.ways == ("wide", "alone", "alone", "wide")
    assert_blocks_equal(agents, twins)


# ---- the loop ----------------------------------------------------------------------------------------------------------
def _loop_pairs(ssc):
    envs = [ssc.VecEnv("MountainCarContinuous-v0", 64, seed=20 + p, max_episode_steps=20) for p in range(3)]
    for e in envs:
        e.reset()
    shapes = [(64, 32), (128, 64), (200, 100)]
    return envs, [agent_of(ssc, p, shapes[p], reward_scale=0.5 + 0.25 * p, num_train_iterations=5, **POPART) for p in range(3)]


def test_population_loop_on_popart_pairs_is_bitwise_the_single_loops(ssc, min_group_two, monkeypatch):
    """P = 3 Pop-Art pairs of 64 envs with hidden sizes 64-32 / 128-64 / 200-100, 4 chunks of 16 steps, 3 iterations per
    chunk, diagnostics every chunk (the population loop's form of stats_every=1 is its monitor): parameters, losses, Summary records, summary.ret_rms and the diagnostics equal three separate
    rl_train_vec_ddpg runs."""
    ways = []
    inner = min_group_two.DDPGPopulation.train_from

    def spy(self, *a, **kw):
        out = inner(self, *a, **kw)
        ways.append(self.ways)
        return out
    monkeypatch.setattr(min_group_two.DDPGPopulation, "train_from", spy)
    kw = dict(num_chunks=4, chunk_steps=16, train_iters=3, replay_capacity=4096)
    envs, agents = _loop_pairs(ssc)
    got = ssc.rl_train_vec_ddpg_population(envs, agents, seed=[3, 4, 5], monitor=ssc.PopulationMonitor(stats_every=1), **kw)
    assert ways == [("wide_popart",) * 3] * 4
    t_envs, twins = _loop_pairs(ssc)
    for p in range(3):
        summary, losses, replay = ssc.rl_train_vec_ddpg(t_envs[p], twins[p], seed=3 + p, stats_every=1, **kw)
        g_summary, g_losses, g_replay = got[p]
        assert len(losses) == 4 and len(g_losses) == 4 and all(torch.equal(x, y) for x, y in zip(g_losses, losses))
        assert g_summary.episodes == summary.episodes and len(summary.episodes) == 3 * 64
        assert g_replay.count == replay.count and g_replay._batches_drawn == replay._batches_drawn == 12
        for k in ("mean", "std"):
            assert g_summary.ret_rms[k].shape == (4,) and g_summary.ret_rms[k].tobytes() == summary.ret_rms[k].tobytes(), (p, k)
        assert sorted(g_summary.agent_stats) == sorted(summary.agent_stats)
        for k, v in summary.agent_stats.items():
            assert np.asarray(g_summary.agent_stats[k]).tobytes() == np.asarray(v).tobytes(), (p, k)
    assert_agents_equal(agents, twins)
    assert_blocks_equal(agents, twins)
