"""``ssc_param_noise_cycle_many`` -- the adaption interval of a whole population in one launch -- and
``DDPGPopulation.param_noise_cycle`` over it.  Results are defined, not toleranced: workgroup p does what pair p's own launch
does, so every array is compared as uint32 bits against the per-pair yardstick run from the same state:

  m > 0    ``torch.index_select`` of the batch out of the ring's state column, then ``ssc_param_noise_cycle``;
  m == 0   ``ssc_param_noise_perturb`` (the interval while a ring holds no batch).

The arrays: ``d_dst`` with a guard band of 64 floats on either side filled with a sentinel, ``*d_stddev``, ``*d_distance``.
``desired`` is placed a factor 4 above or below the distance the pair's own launch measures, alternating pair by pair, so
both branches of the adapt rule are taken within one launch.  Every batch's indices hold repeats, the last row of the ring
and row 0 (a one-row batch: the last row)."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import rms_edge_stats
from tests.test_gpu_param_noise_cycle import COEF, Net, bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FC1BEEF                                  # a NaN with a payload no kernel here produces
RING_ROWS = 301
SINGLE_SHAPES = [(2, 64, 32, False), (3, 64, 32, False), (8, 8, 8, True), (3, 200, 100, False)]


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_NETS = {}


def net_of(ssc, shape):
    if shape not in _NETS:
        _NETS[shape] = Net(ssc, *shape)
    return _NETS[shape]


class Pair:
    """One pair's inputs (never modified) and fresh outputs per run."""

    def __init__(self, ssc, shape, m, p, floor=False, stddev=None):
        self.net, self.m, self.p = net_of(ssc, shape), m, p
        od = shape[0]
        rng = np.random.default_rng(7000 + 131 * p + m)
        self.rms = None
        if floor:
            self.rms, (lo, hi) = rms_edge_stats(od, "floor")
            ring = rng.uniform(lo, hi, size=(RING_ROWS, od)).astype(np.float32)
        else:
            ring = rng.uniform(-1.5, 1.5, size=(RING_ROWS, od)).astype(np.float32)
        self.ring = torch.from_numpy(ring).cuda()
        idx = rng.integers(0, RING_ROWS, size=max(m, 1)).astype(np.int32)
        idx[0] = RING_ROWS - 1
        if m >= 3:
            idx[1], idx[2] = 0, RING_ROWS - 1
        self.idx = torch.from_numpy(idx[:m].copy()).cuda() if m > 0 else None
        self.seed = 0x5EED0000BEEF + 977 * p
        self.gen_adaptive, self.gen_acting = (10 + 2 * p, 11 + 2 * p) if m > 0 else (5 + p, 5 + p)
        self.stddev = float(np.float32(0.05 + 0.01 * (p % 23))) if stddev is None else stddev
        self.desired = 1.0
        if m > 0 and self.stddev > 0.0:
            # the distance does not depend on `desired`: the pair's own launch measures it
            dist = self.yardstick()[2].view(np.float32)[0]
            assert np.isfinite(dist) and dist > 1e-5, dist
            self.desired = float(dist) / 4.0 if p % 2 == 0 else float(dist) * 4.0
            self.divides = p % 2 == 0

    def outputs(self):
        dst = torch.empty(self.net.n + 2 * GUARD, dtype=torch.float32, device="cuda")
        dst.view(torch.int32).fill_(SENTINEL)
        sd = torch.tensor([self.stddev], dtype=torch.float32, device="cuda")
        dist = torch.empty(1, dtype=torch.float32, device="cuda")
        dist.view(torch.int32).fill_(SENTINEL)
        return dst, sd, dist

    def yardstick(self):
        f, net = self.net.f, self.net
        dst, sd, dist = self.outputs()
        if self.m == 0:
            f.check(f.lib().ssc_param_noise_perturb(net.n, f.ptr(net.flat), dst.data_ptr() + 4 * GUARD, f.ptr(sd), *net.skip, self.seed,
                                                    self.gen_acting, stream()))
        else:
            batch = torch.index_select(self.ring, 0, self.idx.long())
            f.check(f.lib().ssc_param_noise_cycle(ctypes.byref(net.desc), self.m, f.ptr(batch),
                                                  None if self.rms is None else f.ptr(self.rms.block), net.n, f.ptr(net.flat),
                                                  *net.skip, self.seed, self.gen_adaptive, self.gen_acting, self.desired, COEF,
                                                  f.ptr(sd), f.ptr(dist), dst.data_ptr() + 4 * GUARD, stream()))
        torch.cuda.synchronize()
        return bits(dst).copy(), bits(sd).copy(), bits(dist).copy()


def launch(ssc, pairs):
    """one ssc_param_noise_cycle_many over fresh outputs -> [(dst bits with guards, stddev bits, distance bits)] per pair"""
    from smartstartcontinuous_amd.population import DeviceItems
    f = ssc._ffi
    P = len(pairs)
    items, cursors = DeviceItems(f.ParamNoiseManyItem, P, "cuda"), DeviceItems(f.ParamNoiseCursor, P, "cuda")
    outs = [pr.outputs() for pr in pairs]
    for it, cu, pr, (dst, sd, dist) in zip(items.items, cursors.items, pairs, outs):
        net = pr.net
        it.actor, it.d_obs = net.desc, pr.ring.data_ptr()
        it.d_idx = None if pr.idx is None else pr.idx.data_ptr()
        it.d_rms = None if pr.rms is None else pr.rms.block.data_ptr()
        it.n, it.d_src = net.n, net.flat.data_ptr()
        it.skip0_begin, it.skip0_end, it.skip1_begin, it.skip1_end = net.skip
        it.seed, it.desired, it.coefficient = pr.seed, pr.desired, COEF
        it.d_stddev, it.d_distance, it.d_dst = sd.data_ptr(), dist.data_ptr(), dst.data_ptr() + 4 * GUARD
        cu.generation_adaptive, cu.generation_acting, cu.m = pr.gen_adaptive, pr.gen_acting, pr.m
    items.upload()
    cursors.upload()
    f.check(f.lib().ssc_param_noise_cycle_many(items.h_ptr, items.d_ptr, cursors.h_ptr, cursors.d_ptr, P, stream()))
    torch.cuda.synchronize()
    for pr in pairs:
        assert np.array_equal(bits(pr.net.flat), pr.net.host.view(np.uint32))      # the sources are untouched
    return [(bits(dst).copy(), bits(sd).copy(), bits(dist).copy()) for dst, sd, dist in outs]


def check(ssc, pairs):
    want = [pr.yardstick() for pr in pairs]
    got = launch(ssc, pairs)
    again = launch(ssc, pairs)
    f32 = np.float32
    for pr, w, g, a in zip(pairs, want, got, again):
        tag = (pr.p, pr.net.dims, pr.m)
        for name, x, y, z in zip(("dst", "stddev", "distance"), w, g, a):
            assert np.array_equal(x, y), (tag, name, int(np.sum(x != y)))
            assert np.array_equal(y, z), (tag, name, "two launches from the same state differ")
        dst = g[0]
        assert np.all(dst[:GUARD] == SENTINEL) and np.all(dst[-GUARD:] == SENTINEL), tag    # nothing outside [d_dst, d_dst + n)
        assert np.all(np.isfinite(dst[GUARD:-GUARD].view(f32))), tag                        # every element inside was written
        if pr.m == 0:                                        # perturb only: neither scalar is touched
            assert g[1][0] == f32(pr.stddev).view(np.uint32) and g[2][0] == SENTINEL, tag
        elif pr.stddev > 0.0:                                # the branch of the adapt rule this pair was set up to take
            sd = f32(pr.stddev)
            assert g[1].view(f32)[0] == (sd / f32(COEF) if pr.divides else sd * f32(COEF)), tag
    return got


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("shape", SINGLE_SHAPES)
def test_one_pair_equals_its_own_launch(ssc, shape, m):
    """staged (64-32, 8-8) and unstaged (200-100) instantiation, a partial tile, exactly one tile, a second tile, no batch;
    both sides of `desired` (the parity of p)"""
    for p in (0, 1):
        check(ssc, [Pair(ssc, shape, m, p)])


def test_tile_loop_of_the_unstaged_path(ssc):
    check(ssc, [Pair(ssc, (3, 200, 100, False), 1024, 0)])


def mixed(ssc):
    return [Pair(ssc, (2, 64, 32, False), 64, 0), Pair(ssc, (8, 8, 8, True), 1, 1, floor=True), Pair(ssc, (3, 200, 100, False), 65, 2),
            Pair(ssc, (3, 64, 32, False), 0, 3)]


def test_mixed_launch_with_and_without_staging(ssc):
    """four shapes and intervals in one launch: the 200-100 pair fits one copy only, so staging is off for all; without it
    staging is on -- and the pairs common to both launches carry the same bits in both"""
    pairs = mixed(ssc)
    off = check(ssc, pairs)
    on = check(ssc, [pairs[0], pairs[1], pairs[3]])
    for a, b in zip((off[0], off[1], off[3]), on):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_more_workgroups_than_compute_units(ssc):
    """260 pairs of one shape with distinct seeds, stddevs and generations, both branches of the adapt rule"""
    check(ssc, [Pair(ssc, (2, 64, 32, False), 64, p) for p in range(260)])


def test_stddev_zero_is_a_bit_copy(ssc):
    pr = Pair(ssc, (2, 64, 32, False), 64, 0, stddev=0.0)
    (dst, sd, dist), = check(ssc, [pr])
    assert np.array_equal(dst[GUARD:-GUARD], pr.net.host.view(np.uint32))                   # -0.0 included
    assert sd[0] == 0 and dist.view(np.float32)[0] == 0.0


# ---- the wrapper -----------------------------------------------------------------------------------------------------
def population_case(ssc, batch_size):
    """3 agents (two noisy with different shapes, stddevs and seeds, one plain) with rings: one below batch_size, two above"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer

    def agent(seed, stddev, h=(64, 32), **kw):
        env = ssc.SingleEnvView(ssc.VecEnv("MountainCarContinuous-v0", 1, seed=seed))
        return DDPG_Baselines_agent(env, None, batch_size=batch_size, actor_h1=h[0], actor_h2=h[1], critic_h1=64, critic_h2=32,
                                    lastLayerTanh=True, seed=seed, param_noise_stddev=stddev, **kw)
    agents = [agent(3, 0.2, normalize_observations=True), agent(4, None), agent(5, 0.05, h=(200, 100)), agent(6, 0.1)]
    records = [batch_size + 37, 500, 1000, batch_size - 1]
    rings = []
    for p, (a, n) in enumerate(zip(agents, records)):
        r = DeviceReplayBuffer(4096, 2, 1, "cuda", seed=40 + p)
        rng = np.random.default_rng(90 + p)
        r.s[:n] = torch.from_numpy(rng.uniform(-1.2, 0.6, size=(n, 2)).astype(np.float32)).cuda()
        r.count = n
        rings.append(r)
        if a.obs_rms is not None:
            a.obs_rms.update_rows(rng.uniform(-1.2, 0.6, size=(200, 2)).astype(np.float32))
    assert [len(r) for r in rings] == records
    return agents, rings


def agent_state(a):
    if a.param_noise is None:
        return None
    return (bits(a.perturbed_actor_flat).copy(), bits(a.d_param_noise_stddev).copy(), bits(a.d_param_noise_distance).copy(),
            a.param_noise_generation, a.perturbed_generation)


@pytest.mark.parametrize("batch_size,fused", [(64, True), (128, False)])
def test_population_wrapper_equals_the_per_agent_calls(ssc, batch_size, fused):
    from smartstartcontinuous_amd.agents import DDPGPopulation
    from smartstartcontinuous_amd.rl_train import adapt_and_perturb
    ours, our_rings = population_case(ssc, batch_size)
    theirs, their_rings = population_case(ssc, batch_size)      # the same seeds: cloned agents and rings
    pop = DDPGPopulation(ours)
    assert pop.pn_fused is None
    for call in range(3):                                        # the third call perturbs into arrays of the caller's
        dsts = [None] * 4
        if call == 2:
            dsts = [torch.empty_like(a.actor_flat) for a in ours]
        their_dsts = [None if d is None else torch.empty_like(d) for d in dsts]
        pop.param_noise_cycle(our_rings, dsts)
        for a, r, d in zip(theirs, their_rings, their_dsts):
            if a.param_noise is not None:
                adapt_and_perturb(a, r, dst=d, cycle=True)
        torch.cuda.synchronize()
        assert pop.pn_fused is fused
        for p, (a, b) in enumerate(zip(ours, theirs)):
            sa, sb = agent_state(a), agent_state(b)
            if sa is None:
                assert sb is None
                continue
            for x, y in zip(sa, sb):
                assert np.array_equal(x, y), (call, p)
            if dsts[p] is not None:
                assert np.array_equal(bits(dsts[p]), bits(their_dsts[p])), (call, p)
        assert [r._batches_drawn for r in our_rings] == [r._batches_drawn for r in their_rings] == [call + 1, 0, call + 1, 0]
    assert [a.param_noise_generation for a in ours if a.param_noise is not None] == [7, 7, 4]   # (1 at construction) + 2 / + 1 per call
