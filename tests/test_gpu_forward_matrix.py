"""Every place that restates the fp32 DDPG network forward -- actor_f32_kernel, actor_row_kernel, actor_generic_kernel,
critic_kernel, net_rows through ssc_ddpg_stats and ssc_ddpg_eval_rollout, cycle_body through ssc_param_noise_cycle -- against
the fp64 forward of tests/forward_cases.py and the derived float32 bound: |x - ref| <= C_FWD 2^-24 A for every element of
every row, the means / population stds / parameter-noise distance to the bounds derived from it.  No flat term anywhere.

Every output lies between guard bands in a buffer pre-filled with a sentinel, with spare rows behind row m - 1: the guards
and the spare rows must come back untouched.  ``FWDRATIO <case> <max |x - ref| / (2^-24 A)>`` is printed before it is
asserted (C_FWD is the limit).  Where two entry points cover one case their outputs are compared bit for bit, as
tests/test_gpu_net_forward.py does for its shapes."""
import ctypes

import numpy as np
import pytest

from tests import forward_cases as F

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD, PAT = 4096, 0xA5
SENTINEL = -7.0
SPARE_ROWS = 3
MC = "MountainCarContinuous-v0"


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Buffers:
    """device arrays, each in the middle of a larger tensor whose other bytes hold PAT (tests/test_gpu_dyn_train_matrix.py)"""
    DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}

    def __init__(self):
        self.raw, self.view = {}, {}

    def add(self, name, arr):
        arr = np.array(arr, order="C")          # (a writable copy: the case data is read-only)
        raw = torch.full((GUARD + arr.nbytes + GUARD,), PAT, dtype=torch.uint8, device="cuda")
        raw[GUARD:GUARD + arr.nbytes].copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1)))
        self.raw[name] = raw
        self.view[name] = raw[GUARD:GUARD + arr.nbytes].view(self.DTYPES[arr.dtype]).view(arr.shape)
        assert self.view[name].data_ptr() % 16 == 0
        return self.view[name]

    def out(self, name, rows, cols, dtype=np.float32):
        """an output of ``rows`` rows with SPARE_ROWS more behind them, every element SENTINEL"""
        return self.add(name, np.full((rows + SPARE_ROWS, cols), SENTINEL, dtype))

    def guards_intact(self):
        return [k for k, raw in self.raw.items() if not (bool((raw[:GUARD] == PAT).all()) and bool((raw[-GUARD:] == PAT).all()))]

    def result(self, name, rows):
        """the first ``rows`` rows on the host; the spare rows must still hold SENTINEL and every guard PAT"""
        torch.cuda.synchronize()
        host = self.view[name].cpu().numpy()
        assert np.all(host[rows:] == SENTINEL), name
        assert self.guards_intact() == []
        return host[:rows].copy()


def _device(w, kind, case):
    from tests.test_gpu_ddpg_stats import Device
    dev = Device({k: np.array(v) for k, v in w.items()}, kind, case.obs, case.act, case.llt)     # (writable copies: the case data is read-only)
    dev.desc.obs_clip = F.OBS_CLIP if case.clip else 0.0
    return dev


def _block(d):
    return None if d["block"] is None else torch.as_tensor(np.array(d["block"])).cuda()


def actor_values(case, w, obs, block, buf=None, name="act"):
    """ssc_actor_forward_rms into a guarded buffer -> (return code, [m, act_dim] float32 or the whole buffer when refused)"""
    from smartstartcontinuous_amd import _ffi
    buf = _Buffers() if buf is None else buf
    dev, m = _device(w, "actor", case), obs.shape[0]
    out, x = buf.out(name, m, case.act), buf.add(name + "_obs", obs)
    rc = _ffi.lib().ssc_actor_forward_rms(ctypes.byref(dev.desc), m, _ffi.ptr(x), _ffi.ptr(out), _stream(), _ffi.ptr(block))
    return rc, buf.result(name, m) if rc == _ffi.SSC_OK else buf.view[name].cpu().numpy()


def critic_values(case, w, obs, act, block, buf=None, name="q"):
    from smartstartcontinuous_amd import _ffi
    buf = _Buffers() if buf is None else buf
    dev, m = _device(w, "critic", case), obs.shape[0]
    out, x, a = buf.out(name, m, 1), buf.add(name + "_obs", obs), buf.add(name + "_a", act)
    rc = _ffi.lib().ssc_critic_forward_rms(ctypes.byref(dev.desc), m, _ffi.ptr(x), _ffi.ptr(a), _ffi.ptr(out), _stream(), _ffi.ptr(block))
    return rc, buf.result(name, m) if rc == _ffi.SSC_OK else buf.view[name].cpu().numpy()


def _report(name, r):
    print("FWDRATIO %s %.3f" % (name, r))
    return r


def _family(case, base):
    """the case runs the kernel family under test, by the restated dispatch"""
    h = case.ah if case.ah is not None else case.ch
    assert F.launched(case.kind, case.obs, h[0], h[1], case.act, case.ln, case.m, case.stats is not None, critic=case.ch) == case.kernel
    assert case.kernel.split("<")[0] == base, (case.name, case.kernel)


def _of(base):
    return [c.name for c in F.CASES if c.kernel.split("<")[0] == base]


_GOT = {}


def _actor_case(name):
    """the device's values of an actor case, computed once"""
    if name not in _GOT:
        case = F.CASE_BY_NAME[name]
        d = F.case_data(case)
        rc, got = actor_values(case, d["actor"], d["obs"], _block(d))
        assert rc == 0, (name, rc)
        _GOT[name] = got
    return _GOT[name]


def _check_actor(name, base):
    case = F.CASE_BY_NAME[name]
    _family(case, base)
    got = _actor_case(name)
    ref, A = F.reference(case)
    assert got.shape == ref.shape == (case.m, case.act)
    assert _report(name, F.value_ratio(got, ref, A)) <= F.C_FWD


@pytest.mark.parametrize("name", _of("actor_f32_kernel"))
def test_actor_f32_kernel(ssc, name):
    _check_actor(name, "actor_f32_kernel")


@pytest.mark.parametrize("name", _of("actor_row_kernel"))
def test_actor_row_kernel(ssc, name):
    _check_actor(name, "actor_row_kernel")


@pytest.mark.parametrize("name", _of("actor_generic_kernel"))
def test_actor_generic_kernel(ssc, name):
    _check_actor(name, "actor_generic_kernel")


def _same_network(a, b):
    return (a.kind, a.obs, a.ah, a.act, a.ln, a.llt, a.stats) == (b.kind, b.obs, b.ah, b.act, b.ln, b.llt, b.stats)


ROW_GENERIC_PAIRS = [(r, g) for r in _of("actor_row_kernel") for g in _of("actor_generic_kernel")
                     if _same_network(F.CASE_BY_NAME[r], F.CASE_BY_NAME[g])]


@pytest.mark.parametrize("row,generic", ROW_GENERIC_PAIRS)
def test_row_and_generic_kernels_agree_to_the_bit(ssc, row, generic):
    """a row case and a generic case of one shape share their network and their leading rows (forward_cases.case_data): one
    256-thread block per row against one lane per row, m = 32 against m = 33 where the table has both"""
    r, g = F.CASE_BY_NAME[row], F.CASE_BY_NAME[generic]
    n = min(r.m, g.m)
    assert np.array_equal(F.case_data(r)["obs"][:n].view(np.uint32), F.case_data(g)["obs"][:n].view(np.uint32))
    assert np.array_equal(_actor_case(row)[:n].view(np.uint32), _actor_case(generic)[:n].view(np.uint32))


def test_row_generic_pairs_cover_the_switch():
    pairs = {(F.CASE_BY_NAME[r].m, F.CASE_BY_NAME[g].m) for r, g in ROW_GENERIC_PAIRS}
    assert (32, 33) in pairs and len(ROW_GENERIC_PAIRS) >= 8


@pytest.mark.parametrize("name", _of("critic_kernel"))
def test_critic_kernel(ssc, name):
    case = F.CASE_BY_NAME[name]
    _family(case, "critic_kernel")
    d = F.case_data(case)
    rc, got = critic_values(case, d["critic"], d["obs"], d["act"], _block(d))
    assert rc == 0
    ref, A = F.reference(case)
    assert got.shape == ref.shape == (case.m, 1)
    if case.head == "big":
        assert np.abs(ref).max() > 10.0
    assert _report(name, F.value_ratio(got, ref, A)) <= F.C_FWD


@pytest.mark.parametrize("refused", range(len(F.REFUSED_CASES)))
def test_refused_shapes_leave_the_output_alone(ssc, refused):
    """one hidden unit beyond 160 KB of LDS with LayerNorm: SSC_EUNSUPPORTED, the output buffer still at its sentinel"""
    from smartstartcontinuous_amd import _ffi
    kind, od, h1, h2, ad, ln, m = F.REFUSED_CASES[refused]
    assert F.launched(kind, od, h1, h2, ad, ln, m, False) == F.REFUSED
    case = F._c("refused_%d" % refused, kind, od, (h1, h2) if kind == "actor" else None, ad, ln, True, None, m,
                ch=(h1, h2) if kind == "critic" else None)
    assert case.kernel == F.REFUSED
    d = F.case_data(case)
    if kind == "actor":
        rc, whole = actor_values(case, d["actor"], d["obs"], None)
    else:
        rc, whole = critic_values(case, d["critic"], d["obs"], d["act"], None)
    assert rc == _ffi.SSC_EUNSUPPORTED
    assert np.all(whole == SENTINEL)


@pytest.mark.parametrize("name", _of("ddpg_stats_rows_kernel"))
def test_net_rows_through_ddpg_stats(ssc, name):
    """the eight mean / std slots against the derived mean and std bounds; at m = 1 every mean slot is the forward kernels'
    own float"""
    from tests.test_gpu_ddpg_stats import launch
    case = F.CASE_BY_NAME[name]
    _family(case, "ddpg_stats_rows_kernel")
    d, ref = F.case_data(case), F.reference(case)
    actor, critic = _device(d["actor"], "actor", case), _device(d["critic"], "critic", case)
    pert = _device(d["pert"], "actor", case) if case.pert else None
    buf = _Buffers()
    out = buf.add("out", np.full(11, SENTINEL, np.float64))
    obs, act = buf.add("obs", d["obs"]), buf.add("act", d["act"])
    block = _block(d)
    sd = torch.tensor([0.2], dtype=torch.float32, device="cuda") if case.pert else None
    launch(ssc, actor, critic, pert, obs, act, block, sd, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert buf.guards_intact() == []
    slots = [(2, "q"), (4, "qpi"), (6, "pi")] + ([(8, "pp")] if case.pert else [])
    worst = 0.0
    for slot, k in slots:
        o, A = ref[k]
        rm, rs = F.mean_ratio(got[slot], o, A), F.std_ratio(got[slot + 1], o, A)
        print("FWDRATIO %s slot %d mean %.3f std %.3f" % (name, slot, rm, rs))
        worst = max(worst, rm, rs)
    if not case.pert:
        assert np.all(np.isnan(got[8:10]))
    assert _report(name, worst) <= F.C_FWD
    if case.m == 1:      # net_rows against the stand-alone kernels, bit for bit
        _, pi = actor_values(case, d["actor"], d["obs"], block)
        _, q = critic_values(case, d["critic"], d["obs"], d["act"], block)
        _, qpi = critic_values(case, d["critic"], d["obs"], pi, block)
        assert got[2] == float(q[0, 0]) and got[4] == float(qpi[0, 0]) and got[6] == float(pi[0, 0])
        assert got[3] == got[5] == got[7] == 0.0


EVAL_CASES = _of("ddpg_eval_kernel")


@pytest.mark.parametrize("global_weights", [False, True])
@pytest.mark.parametrize("name", EVAL_CASES)
def test_net_rows_through_ddpg_eval_rollout(ssc, monkeypatch, name, global_weights):
    """MountainCar, n = 17 (the second workgroup holds one env), K = 5, both weight stagings: for every logged step log.act
    against the actor reference on log.obs, q against the critic reference on (log.obs, the device's log.act as an exact
    input), per element; and both against the stand-alone forward kernels, bit for bit"""
    from tests.test_gpu_ddpg_eval import call
    case = F.CASE_BY_NAME[name]
    _family(case, "ddpg_eval_kernel")
    fit = F.eval_weights_fit(case.obs, case.ah, case.ch, case.ln)         # (held to ddpg_eval.hip's carve on the CPU)
    assert F.launched("eval", case.obs, case.ah[0], case.ah[1], 1, case.ln, case.m, case.stats is not None, global_weights, critic=case.ch) == \
        F.EVAL % ("true" if fit and not global_weights else "false")
    n, K = 17, 5
    assert case.m == n * K
    d = F.case_data(case)
    actor, critic = _device(d["actor"], "actor", case), _device(d["critic"], "critic", case)
    block = _block(d)
    if global_weights:
        monkeypatch.setenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", "1")
    else:
        monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)
    env = ssc.VecEnv(MC, n, seed=5)
    env.reset()
    assert float(env.action_space.low[0]) == -1.0 and float(env.action_space.high[0]) == 1.0
    chunk = ssc.TransitionChunk(env.obs_dim, K, n, env.device)
    chunk.step0, chunk.env_id0 = env.t, env.env_id0
    buf = _Buffers()
    q = buf.out("q", K, n)
    out = buf.add("out", np.full(8, SENTINEL, np.float64))
    call(env, actor, critic, K, rms=block, chunk=chunk, q=q[:K], out=out)
    monkeypatch.delenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS", raising=False)
    q_dev = buf.result("q", K).reshape(K * n, 1)
    obs = chunk.obs.permute(1, 2, 0).reshape(K * n, 2).contiguous().cpu().numpy()
    act = chunk.act.reshape(K * n, 1).cpu().numpy()
    assert np.abs(act).max() < 1.0 and len(np.unique(act)) > n      # inside MountainCar's action range: the raw actor output
    if case.stats == "floor":       # std 0.1 around a mean of 0.2: every position of the valley lies beyond the clip
        assert np.abs(F.x_hat64(obs, d["mean"], d["std"], clip=False)).max() > F.OBS_CLIP
    kw = dict(mean=d["mean"], std=d["std"], llt=case.llt)
    pi_ref, pi_A = F.forward("actor", d["actor"], obs, **kw)
    q_ref, q_A = F.forward("critic", d["critic"], obs, act=act, **kw)
    assert (np.abs(q_ref).max() > 10.0) == (case.head == "big")
    r_pi, r_q = F.value_ratio(act, pi_ref, pi_A), F.value_ratio(q_dev, q_ref, q_A)
    tag = "%s/%s" % (name, "global" if global_weights else "lds")
    print("FWDRATIO %s act %.3f q %.3f" % (tag, r_pi, r_q))
    assert _report(tag, max(r_pi, r_q)) <= F.C_FWD
    _, pi_fwd = actor_values(case, d["actor"], obs, block)
    _, q_fwd = critic_values(case, d["critic"], obs, act, block)
    assert np.array_equal(act.view(np.uint32), pi_fwd.view(np.uint32))
    assert np.array_equal(q_dev.view(np.uint32), q_fwd.view(np.uint32))


CYCLE_SHAPES = {(2, 64, 32, False), (8, 8, 8, True)}


@pytest.mark.parametrize("name", _of("param_noise_cycle_kernel"))
def test_cycle_body_through_param_noise_cycle(ssc, name):
    """tests/test_gpu_param_noise_cycle.py's Net: the distance of ssc_param_noise_cycle against sqrt(mean((a - b)^2)) of the
    fp64 forwards on the plain parameters and on the perturbed ones read back from ssc_param_noise_perturb (exact float32
    inputs to the reference), to the derived distance bound"""
    from tests.gpu_util import rms_edge_stats
    from tests.test_gpu_param_noise_cycle import COEF, GEN_ACTING, GEN_ADAPTIVE, SEED, Net
    case = F.CASE_BY_NAME[name]
    _family(case, "param_noise_cycle_kernel")
    shape = (case.obs, case.ah[0], case.ah[1], case.ln)
    assert shape in CYCLE_SHAPES and case.act == 1
    net = Net(ssc, *shape)
    net.desc.last_layer_tanh = int(case.llt)       # (Net fixes 1: the relu second layer of cycle_body is reached here alone)
    f = net.f
    rng = np.random.default_rng(1000 * case.m + case.obs)
    rms = mean = std = lo = hi = None
    if case.stats:
        rms, (lo, hi) = rms_edge_stats(case.obs, case.stats)
        mean, std = rms.mean_std()
    obs_h = F._rows(rng, case.obs, mean, std, lo, hi, max(case.m, 4))[:case.m].copy()
    sd0 = torch.tensor([0.2], dtype=torch.float32, device="cuda")
    adaptive = net.perturb(sd0, GEN_ADAPTIVE).cpu().numpy()
    weights = lambda flat: {k: flat[net.offsets[k]:net.offsets[k] + int(np.prod(net.shapes[k]))].reshape(net.shapes[k]) for k in net.order}
    kw = dict(mean=mean, std=std, llt=case.llt)
    a, Aa = F.forward("actor", weights(net.host), obs_h, **kw)
    b, Ab = F.forward("actor", weights(adaptive), obs_h, **kw)
    ref = F.distance64(a, b)
    assert np.isfinite(ref) and ref > 1e-4
    buf = _Buffers()
    obs = buf.add("obs", obs_h)
    sd, dist = buf.add("sd", np.full(1, 0.2, np.float32)), buf.add("dist", np.full(1 + SPARE_ROWS, SENTINEL, np.float32))
    dst = buf.add("dst", np.full(net.n + SPARE_ROWS, SENTINEL, np.float32))
    f.check(f.lib().ssc_param_noise_cycle(ctypes.byref(net.desc), case.m, f.ptr(obs), None if rms is None else f.ptr(rms.block), net.n,
                                          f.ptr(net.flat), *net.skip, SEED, GEN_ADAPTIVE, GEN_ACTING, ref / 4.0, COEF, f.ptr(sd), f.ptr(dist),
                                          f.ptr(dst), _stream()))
    torch.cuda.synchronize()
    assert buf.guards_intact() == []
    dist_h, dst_h = dist.cpu().numpy(), dst.cpu().numpy()
    assert np.all(dist_h[1:] == SENTINEL) and np.all(dst_h[net.n:] == SENTINEL) and np.all(np.isfinite(dst_h[:net.n]))
    assert float(sd.item()) == float(np.float32(0.2) / np.float32(COEF))             # the distance lies above `desired`
    # the stand-alone forward kernel on both copies, per element, then the fused kernel's distance
    def stand_alone(flat):
        d = net.desc_over(flat)
        d.last_layer_tanh = int(case.llt)
        out = buf.out("fwd%d" % len(buf.raw), case.m, 1)
        f.check(f.lib().ssc_actor_forward_rms(ctypes.byref(d), case.m, f.ptr(obs), f.ptr(out), _stream(), None if rms is None else f.ptr(rms.block)))
        return out
    adaptive_d = torch.from_numpy(adaptive).cuda()
    fa, fb = stand_alone(net.flat)[:case.m], stand_alone(adaptive_d)[:case.m]
    torch.cuda.synchronize()
    assert buf.guards_intact() == [] and not np.array_equal(fa.cpu().numpy(), fb.cpu().numpy())
    # ... whose distance through ssc_param_noise_adapt carries the bits of the fused kernel's (tests/test_gpu_param_noise_cycle.py)
    sd2, dist2 = buf.add("sd2", np.full(1, 0.2, np.float32)), buf.add("dist2", np.full(1, SENTINEL, np.float32))
    f.check(f.lib().ssc_param_noise_adapt(case.m, f.ptr(fa), f.ptr(fb), ref / 4.0, COEF, f.ptr(sd2), f.ptr(dist2), _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(dist2.cpu().numpy().view(np.uint32), dist_h[:1].view(np.uint32))
    assert np.array_equal(sd2.cpu().numpy().view(np.uint32), sd.cpu().numpy().view(np.uint32))
    r_el = max(F.value_ratio(fa.cpu().numpy(), a, Aa), F.value_ratio(fb.cpu().numpy(), b, Ab))
    print("FWDRATIO %s forward kernels on both copies %.3f" % (name, r_el))
    assert r_el <= F.C_FWD
    assert _report(name, F.distance_ratio(dist_h[0], a, Aa, b, Ab)) <= F.C_FWD
