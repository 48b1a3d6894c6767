"""``ssc_param_noise_cycle`` -- perturb the adaptive copy, both actor forwards, adapt, perturb the acting copy, in one launch --
against the four-call sequence it replaces (``ssc_param_noise_perturb``, two ``ssc_actor_forward[_rms]``,
``ssc_param_noise_adapt``, ``ssc_param_noise_perturb``) and against the fp64 oracle forward.

The fp64 reference of a case: the oracle's actor forward on the plain fp32 parameters and on the adaptive copy's fp32
parameters (the bits ``ssc_param_noise_perturb`` writes: the stream is the documented one, so the copy in LDS holds the same),
distance = sqrt(mean((a - b)^2)) in fp64.  ``desired`` is placed a factor 4 above or below that distance, so both paths take
the same side whatever their rounding.

DISTANCE_BOUND is the bound ``tests/test_gpu_param_noise.py`` applies to ``ssc_param_noise_adapt``: 1e-6 of the distance.  The
in-kernel forward sums every unit in the order of the stand-alone fp32 forward kernels, so it can share it: on one MI355X the
fused kernel's distance carried the bits of the composed path's in every case below, the largest error of either against the
fp64 reference being 5.2e-7 of the distance (a one-row batch, where the fp32 rounding of the two actions is all there is;
3.5e-7 and below from 63 rows on).  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests.gpu_util import actor_weights, rms_edge_stats, x_hat64

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 0x5EED0000BEEF
GEN_ADAPTIVE, GEN_ACTING = 6, 7
COEF = 1.01
DISTANCE_BOUND = 1e-6             # relative: the bound of test_adapt_matches_numpy
# (obs_dim, h1, h2, layer_norm)
SHAPES = [(2, 64, 32, False), (3, 64, 32, False), (8, 8, 8, True), (3, 200, 100, False)]
BATCHES = [1, 63, 64, 65, 1024, 4096]
KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
LN_ORDER = ("W1", "b1", "ln1_b", "ln1_g", "W2", "b2", "ln2_b", "ln2_g", "W3", "b3")


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


class Net:
    """A flat parameter array on the device in the layout of ``actor_flat``, its descriptor, its skip ranges."""

    def __init__(self, ssc, obs_dim, h1, h2, ln, seed=5):
        w = actor_weights(obs_dim, h1, h2, seed=seed, w3_scale=0.5)
        order = KEYS
        if ln:
            rng = np.random.default_rng(seed + 1)
            w.update(ln1_b=(0.1 * rng.normal(size=h1)).astype(np.float32), ln1_g=rng.uniform(0.5, 1.5, h1).astype(np.float32),
                     ln2_b=(0.1 * rng.normal(size=h2)).astype(np.float32), ln2_g=rng.uniform(0.5, 1.5, h2).astype(np.float32))
            order = LN_ORDER
        self.order, self.shapes, self.ln = order, {k: w[k].shape for k in order}, ln
        self.host = np.concatenate([w[k].reshape(-1) for k in order]).astype(np.float32)
        self.host[0] = -0.0                                     # a bit copy keeps the sign of zero
        self.n = len(self.host)
        self.offsets, o = {}, 0
        for k in order:
            self.offsets[k] = o
            o += int(np.prod(self.shapes[k]))
        self.skip = (0, 0, 0, 0)
        if ln:
            self.skip = (self.offsets["ln1_b"], self.offsets["ln1_b"] + 2 * h1, self.offsets["ln2_b"], self.offsets["ln2_b"] + 2 * h2)
        self.dims = (obs_dim, h1, h2)
        self.f = ssc._ffi
        self.flat = torch.from_numpy(self.host).cuda()
        self.desc = self.desc_over(self.flat)

    def desc_over(self, flat):
        f = self.f
        d = f.ActorDesc()
        d.obs_dim, d.h1, d.h2, d.act_dim = self.dims[0], self.dims[1], self.dims[2], 1
        for k in self.order:
            setattr(d, k, flat.data_ptr() + 4 * self.offsets[k])
        d.last_layer_tanh, d.precision, d.obs_clip = 1, f.SSC_PREC_F32, 5.0
        return d

    def params64(self, flat_host):
        """oracle keywords of a flat fp32 array"""
        p = {k: flat_host[self.offsets[k]:self.offsets[k] + int(np.prod(self.shapes[k]))].reshape(self.shapes[k]).astype(np.float64)
             for k in self.order}
        kw = {k: p[k] for k in KEYS}
        if self.ln:
            kw["layer_norm"] = ((p["ln1_g"], p["ln1_b"]), (p["ln2_g"], p["ln2_b"]))
        return kw

    # ---- the existing entry points ---------------------------------------------------------------------------------
    def perturb(self, sd, generation):
        f = self.f
        dst = torch.full_like(self.flat, float("nan"))
        f.check(f.lib().ssc_param_noise_perturb(self.n, f.ptr(self.flat), f.ptr(dst), f.ptr(sd), *self.skip, SEED, generation,
                                                stream()))
        return dst

    def forward(self, flat, obs, rms):
        f = self.f
        out = torch.empty((obs.shape[0], 1), dtype=torch.float32, device="cuda")
        d = self.desc_over(flat)
        f.check(f.lib().ssc_actor_forward_rms(ctypes.byref(d), obs.shape[0], f.ptr(obs), f.ptr(out), stream(),
                                              None if rms is None else f.ptr(rms.block)))
        return out

    def composed(self, obs, rms, stddev, desired):
        """the four-call sequence -> (stddev bits, acting copy bits, distance, adaptive copy on the host)"""
        f = self.f
        sd = torch.tensor([stddev], dtype=torch.float32, device="cuda")
        dist = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        adaptive = self.perturb(sd, GEN_ADAPTIVE)
        a, b = self.forward(self.flat, obs, rms), self.forward(adaptive, obs, rms)
        f.check(f.lib().ssc_param_noise_adapt(a.numel(), f.ptr(a), f.ptr(b), desired, COEF, f.ptr(sd), f.ptr(dist), stream()))
        dst = self.perturb(sd, GEN_ACTING)
        return bits(sd).copy(), bits(dst).copy(), float(dist.item()), adaptive.cpu().numpy()

    # ---- the new one ---------------------------------------------------------------------------------------------
    def cycle(self, obs, rms, stddev, desired):
        f = self.f
        sd = torch.tensor([stddev], dtype=torch.float32, device="cuda")
        dist = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        dst = torch.full_like(self.flat, float("nan"))
        f.check(f.lib().ssc_param_noise_cycle(ctypes.byref(self.desc), obs.shape[0], f.ptr(obs),
                                              None if rms is None else f.ptr(rms.block), self.n, f.ptr(self.flat), *self.skip, SEED,
                                              GEN_ADAPTIVE, GEN_ACTING, desired, COEF, f.ptr(sd), f.ptr(dist), f.ptr(dst),
                                              stream()))
        torch.cuda.synchronize()
        assert np.array_equal(bits(self.flat), self.host.view(np.uint32))           # the source is untouched
        return bits(sd).copy(), bits(dst).copy(), float(dist.item())

    def distance64(self, adaptive_host, x64):
        a = O.actor_forward(x64, **self.params64(self.host))
        b = O.actor_forward(x64, **self.params64(adaptive_host))
        return float(np.sqrt(np.mean((a - b) ** 2)))


_NETS, _CASES = {}, {}


def net_of(ssc, shape):
    if shape not in _NETS:
        _NETS[shape] = Net(ssc, *shape)
    return _NETS[shape]


def case(ssc, shape, m, floor):
    """Inputs, the fp64 reference and the composed path of one (shape, batch, statistics) case -- computed once, shared by
    the tests below, never modified."""
    key = (shape, m, floor)
    if key in _CASES:
        return _CASES[key]
    net = net_of(ssc, shape)
    rng = np.random.default_rng(1000 * m + shape[0] + shape[1])
    rms = None
    if floor:
        rms, (lo, hi) = rms_edge_stats(shape[0], "floor")
        obs_h = rng.uniform(lo, hi, size=(m, shape[0])).astype(np.float32)
        if m >= 63:
            obs_h[0, 0], obs_h[1, 0] = lo[0], hi[0]                 # both clip edges are in the batch
        x64 = x_hat64(obs_h, rms)
        if m >= 63:
            assert np.any(x64 == 5.0) and np.any(x64 == -5.0)
    else:
        obs_h = rng.uniform(-1.5, 1.5, size=(m, shape[0])).astype(np.float32)
        x64 = np.clip(obs_h.astype(np.float64), -5.0, 5.0)
    obs = torch.from_numpy(obs_h).cuda()
    # the adaptive copy does not depend on `desired`: one composed call yields it and the reference distance
    _, _, _, adaptive = net.composed(obs, rms, 0.2, 1.0)
    ref = net.distance64(adaptive, x64)
    assert np.isfinite(ref) and ref > 1e-4, ref
    out = dict(net=net, obs=obs, rms=rms, ref=ref, x64=x64, sides={})
    for side, desired in (("above", ref / 4.0), ("below", ref * 4.0)):
        # verified on the CPU: the fp64 distance lies a factor 2 or more from `desired`, on the intended side
        assert (ref >= 2.0 * desired) if side == "above" else (2.0 * ref <= desired)
        out["sides"][side] = (desired, net.composed(obs, rms, 0.2, desired))
    _CASES[key] = out
    return out


def check_case(c):
    f32 = np.float32
    for side, (desired, (sd_c, dst_c, dist_c, _)) in c["sides"].items():
        sd_k, dst_k, dist_k = c["net"].cycle(c["obs"], c["rms"], 0.2, desired)
        err_c, err_k = abs(dist_c - c["ref"]) / c["ref"], abs(dist_k - c["ref"]) / c["ref"]
        print(f"cycle {c['net'].dims} ln={c['net'].ln} m={c['obs'].shape[0]} rms={c['rms'] is not None} {side}: ref {c['ref']:.9e} "
              f"composed {dist_c:.9e} (rel {err_c:.3e}) cycle {dist_k:.9e} (rel {err_k:.3e})")
        # 1. the adapted stddev and the acting copy: the bits of the four-call sequence
        want = f32(0.2) / f32(COEF) if side == "above" else f32(0.2) * f32(COEF)       # above `desired`: divided
        assert sd_c.view(np.float32)[0] == want
        assert np.array_equal(sd_k, sd_c), (side, sd_k, sd_c)
        assert np.array_equal(dst_k, dst_c), (side, int(np.sum(dst_k != dst_c)))
        assert np.all(np.isfinite(dst_k.view(np.float32)))                          # every element was written
        s = c["net"].skip
        for b, e in ((s[0], s[1]), (s[2], s[3])):
            assert np.array_equal(dst_k[b:e], c["net"].host.view(np.uint32)[b:e])   # LayerNorm segments: bit copies
        # 2. the distance against the fp64 reference
        assert err_k <= DISTANCE_BOUND, (side, dist_k, c["ref"], err_k)


@pytest.mark.parametrize("m", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cycle_equals_the_composed_path(ssc, shape, m):
    check_case(case(ssc, shape, m, False))


@pytest.mark.parametrize("m", [1, 65, 4096])
@pytest.mark.parametrize("shape", SHAPES)
def test_cycle_with_floor_statistics(ssc, shape, m):
    """d_rms on floor statistics (every std 0.1): observations land on the +-5 clip; cases 1 and 2 hold."""
    check_case(case(ssc, shape, m, True))


@pytest.mark.parametrize("shape", SHAPES)
def test_cycle_is_deterministic(ssc, shape):
    c = case(ssc, shape, 1024, False)
    desired = c["sides"]["above"][0]
    first = c["net"].cycle(c["obs"].clone(), None, 0.2, desired)
    again = c["net"].cycle(c["obs"].clone(), None, 0.2, desired)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert np.float32(first[2]).view(np.uint32) == np.float32(again[2]).view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES)
def test_cycle_stddev_zero(ssc, shape):
    """stddev 0: both copies are bit copies, the distance is exactly 0 and the stddev stays 0 under the multiplication"""
    c = case(ssc, shape, 65, False)
    sd, dst, dist = c["net"].cycle(c["obs"], None, 0.0, 0.2)
    assert dist == 0.0 and sd[0] == 0
    assert np.array_equal(dst, c["net"].host.view(np.uint32))


def test_agent_cycle_consumes_the_generations_of_the_pair(ssc):
    """DDPG_Baselines_agent.param_noise_cycle == adapt_param_noise + perturb_policy: counters, stddev and acting copy"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent

    def agent():
        return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0", seed=1), None, batch_size=64, actor_h1=64, actor_h2=32,
                                    critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7, param_noise_stddev=0.2,
                                    param_noise_desired_action_stddev=1e-4)      # far below any distance: the stddev is divided
    a, b = agent(), agent()
    obs = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(64, 2)).astype(np.float32)).cuda()
    for _ in range(2):
        a.adapt_param_noise(obs)
        a.perturb_policy()
        d = b.param_noise_cycle(obs)
        assert d.data_ptr() == b.d_param_noise_distance.data_ptr()
        assert (a.param_noise_generation, a.perturbed_generation) == (b.param_noise_generation, b.perturbed_generation)
        assert np.array_equal(bits(a.d_param_noise_stddev), bits(b.d_param_noise_stddev))
        assert np.array_equal(bits(a.perturbed_actor_flat), bits(b.perturbed_actor_flat))
    assert float(b.d_param_noise_stddev.item()) == float(np.float32(0.2) / np.float32(1.01) / np.float32(1.01))
    other = torch.empty_like(b.perturbed_actor_flat)
    before = bits(b.perturbed_actor_flat).copy()
    b.param_noise_cycle(obs, dst=other)
    a.adapt_param_noise(obs)
    a.perturb_policy()
    assert np.array_equal(bits(other), bits(a.perturbed_actor_flat)) and np.array_equal(bits(b.perturbed_actor_flat), before)
