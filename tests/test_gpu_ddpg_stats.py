"""``ssc_ddpg_stats`` / ``DDPG_Baselines_agent.get_stats`` on the GPU against the fp64 oracle.

Expected values: ``O.actor_forward`` / ``O.critic_forward`` on the sample (normalised by ``obs_rms.normalize_f32`` where a
statistics block is given), then numpy f64 ``mean`` / ``std`` (ddof = 0).

Bound: a mean of values moves by at most the largest per-element error and a population std by at most
their rms, so every statistic inherits the per-element tolerance of the fp32 forward kernels --
``ssc_actor_forward``: 1e-5 abs, ``ssc_critic_forward``: 1e-5 * max(1, max |Q|) (tests/test_gpu_obs_rms_oracle.py,
tests/test_gpu_agents.py).  Q(s, pi(s)) is a critic evaluated at an action that itself carries the actor's tolerance, so its
bound adds what that tolerance can move Q by -- measured on the ORACLE alone: twice the largest |Q(s, a +- 1e-5 e_d) - Q(s, a)|
summed over the action dimensions."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests.net_weights import make_net, oracle_kw      # (numpy only; other test modules import them from here)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CLIP = 5.0
TOL_ACT = 1e-5
ENV = "MountainCarContinuous-v0"
NETS = {"64-32": ((64, 32), (64, 32), False), "64-64ln": ((64, 64), (64, 64), True), "200-100": ((200, 100), (200, 100), False),
        "mixed": ((64, 32), (128, 64), False)}


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


class Device:
    """the device copies of one network plus its descriptor"""

    def __init__(self, w, kind, obs_dim, act_dim, tanh):
        from smartstartcontinuous_amd import _ffi
        self.t = {k: torch.as_tensor(v).cuda().contiguous() for k, v in w.items()}
        d = _ffi.ActorDesc() if kind == "actor" else _ffi.CriticDesc()
        d.obs_dim, d.act_dim, d.h1, d.h2 = obs_dim, act_dim, w["W1"].shape[1], w["W2"].shape[1]
        for k, v in self.t.items():
            setattr(d, k, v.data_ptr())
        d.last_layer_tanh, d.obs_clip = int(tanh), CLIP
        self.desc = d


def launch(ssc, actor, critic, pert, obs, act, rms=None, stddev=None, out=None):
    from smartstartcontinuous_amd import _ffi
    lib = _ffi.lib()
    m = obs.shape[0]
    ws = torch.empty(int(lib.ssc_ddpg_stats_workspace_bytes(m)), dtype=torch.uint8, device="cuda")
    out = torch.zeros(_ffi.SSC_DDPG_N_STATS, dtype=torch.float64, device="cuda") if out is None else out
    _ffi.check(lib.ssc_ddpg_stats(ctypes.byref(actor.desc), ctypes.byref(critic.desc),
                                  None if pert is None else ctypes.byref(pert.desc), m, _ffi.ptr(obs), _ffi.ptr(act), _ffi.ptr(rms),
                                  _ffi.ptr(stddev), _ffi.ptr(out), _ffi.ptr(ws), ws.numel(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


CASES = [   # m, (obs_dim, act_dim), network, lastLayerTanh, statistics block, perturbed actor
    (1, (2, 1), "64-32", True, False, False),
    (15, (3, 1), "64-64ln", False, True, True),
    (16, (3, 2), "200-100", True, True, False),
    (17, (2, 1), "mixed", False, False, True),
    (64, (2, 1), "64-32", True, True, True),
    (1000, (3, 2), "64-64ln", True, False, True),
    (64, (3, 1), "200-100", False, False, True),
    (1000, (2, 1), "mixed", True, True, False),
    (17, (3, 2), "64-32", False, True, True),
    (15, (2, 1), "200-100", True, False, False),
    (16, (2, 1), "64-64ln", False, False, False),
    (1, (3, 2), "mixed", True, True, True),
    (64, (3, 2), "mixed", False, True, False),
    (1000, (3, 1), "64-32", False, False, False),
]


def build_case(m, dims, net, tanh, with_rms, with_pert, seed):
    """inputs, networks and the oracle's per-row values -- CPU only"""
    from smartstartcontinuous_amd import obs_rms as R
    od, ad = dims
    (ah1, ah2), (ch1, ch2), ln = NETS[net]
    rng = np.random.default_rng(seed)
    aw = make_net(rng, od, ah1, 0, ah2, ad, ln, 0.25, 0.0)
    cw = make_net(rng, od, ch1, ad, ch2, 1, ln, 1.5, 20.0)      # Q of O(10): a bias of 20 and a spread of a few units
    pw = None
    if with_pert:       # actor + N(0, 0.2^2) on the perturbable variables (LayerNorm gamma / beta stay)
        pw = {k: (v + (0.2 * rng.normal(size=v.shape)).astype(np.float32) if not k.startswith("ln") else v) for k, v in aw.items()}
    block = None
    if with_rms:
        mean, std = np.array([0.3, -0.6, 1.5])[:od], np.array([0.4, 2.0, 0.7])[:od]
        rows = rng.normal(mean, std, size=(4000, od)).astype(np.float32).astype(np.float64)
        block = R.rms_initial(od)
        block[:od] += rows.sum(0)
        block[od:2 * od] += (rows ** 2).sum(0)
        block[2 * od] += len(rows)
        got_mean, got_std = R.mean_std_f32(block)
        assert np.all(np.abs(got_mean) > 0.2) and np.all(np.abs(got_std - 1.0) > 0.2)       # well away from (0, 1)
        obs = (mean + std * rng.uniform(-7.5, 7.5, size=(m, od))).astype(np.float32)     # |u| > 5 for a third of the draws
        x = R.normalize_f32(obs, block, CLIP).astype(np.float64)
        if m >= 64:
            share = np.mean(np.abs(x) == CLIP)
            assert 0.2 <= share <= 0.45, share
        else:
            assert np.any(np.abs(x) == CLIP) or m == 1
    else:
        obs = rng.uniform(-1.5, 1.5, size=(m, od)).astype(np.float32)
        obs[::5] *= 5.0                                               # some raw components beyond the plain +-5 clip
        x = obs.astype(np.float64)
    act = rng.uniform(-1, 1, size=(m, ad)).astype(np.float32)
    a_ref = O.actor_forward(x, **oracle_kw(aw), last_layer_tanh=tanh, obs_clip=CLIP)
    p_ref = O.actor_forward(x, **oracle_kw(pw), last_layer_tanh=tanh, obs_clip=CLIP) if with_pert else None
    critic = lambda a: O.critic_forward(x, a, **oracle_kw(cw), last_layer_tanh=tanh, obs_clip=CLIP)[:, 0]
    q_ref, qpi_ref = critic(act), critic(a_ref)
    # what the actor's own tolerance can move Q(s, pi(s)) by, from the oracle alone
    moved = np.zeros(m)
    for d in range(ad):
        for sgn in (-1.0, 1.0):
            e = np.zeros(ad)
            e[d] = sgn * TOL_ACT
            moved = np.maximum(moved, np.abs(critic(a_ref + e) - qpi_ref))
    tol_q = 1e-5 * max(1.0, np.abs(q_ref).max())
    tol_qpi = 1e-5 * max(1.0, np.abs(qpi_ref).max()) + 2 * ad * moved.max()
    return dict(od=od, ad=ad, aw=aw, cw=cw, pw=pw, block=block, obs=obs, act=act, a_ref=a_ref, p_ref=p_ref, q_ref=q_ref,
                qpi_ref=qpi_ref, tol_q=tol_q, tol_qpi=tol_qpi, tanh=tanh)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_stats_vs_oracle(ssc, case):
    from smartstartcontinuous_amd import obs_rms as R
    m, dims, net, tanh, with_rms, with_pert = CASES[case]
    c = build_case(m, dims, net, tanh, with_rms, with_pert, seed=100 + case)
    # the sample is worth looking at: Q of O(1) .. O(100), less than half of the actions saturated (oracle only)
    saturated = float(np.mean(np.abs(c["a_ref"]) > 0.999))
    assert saturated < 0.5, saturated
    assert 1.0 <= np.abs(c["q_ref"]).max() <= 300.0
    actor = Device(c["aw"], "actor", *dims, tanh)
    critic = Device(c["cw"], "critic", *dims, tanh)
    pert = Device(c["pw"], "actor", *dims, tanh) if with_pert else None
    rms = torch.as_tensor(c["block"]).cuda() if with_rms else None
    sd = torch.tensor([0.2], dtype=torch.float32, device="cuda") if with_pert else None
    obs, act = torch.as_tensor(c["obs"]).cuda(), torch.as_tensor(c["act"]).cuda()
    got = launch(ssc, actor, critic, pert, obs, act, rms, sd).cpu().numpy()
    again = launch(ssc, actor, critic, pert, obs, act, rms, sd).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))          # run to run: the same 11 doubles
    want = [(2, c["q_ref"], c["tol_q"]), (4, c["qpi_ref"], c["tol_qpi"]), (6, c["a_ref"], TOL_ACT)]
    if with_pert:
        want.append((8, c["p_ref"], TOL_ACT))
    for slot, ref, tol in want:
        ref = np.asarray(ref, np.float64).reshape(-1)
        d_mean, d_std = abs(got[slot] - ref.mean()), abs(got[slot + 1] - ref.std())
        print(f"case {case} slot {slot}: mean {got[slot]:.9g} (d {d_mean:.3g}) std {got[slot + 1]:.9g} (d {d_std:.3g}) tol {tol:.3g}")
        assert d_mean <= tol and d_std <= tol, (slot, got[slot], ref.mean(), got[slot + 1], ref.std(), tol)
    if with_rms:       # the fp32 mean / std the networks use, averaged over the dimensions in f64
        mean, std = R.mean_std_f32(c["block"])
        assert abs(got[0] - mean.astype(np.float64).mean()) <= 1e-15
        assert abs(got[1] - std.astype(np.float64).mean()) <= 1e-15
    else:
        assert np.isnan(got[0]) and np.isnan(got[1])
    if with_pert:
        assert got[10] == float(np.float32(0.2))
    else:
        assert np.all(np.isnan(got[8:11]))


def test_nan_slots_and_stddev_without_perturbed_actor(ssc):
    c = build_case(17, (2, 1), "64-32", True, False, False, seed=5)
    actor, critic = Device(c["aw"], "actor", 2, 1, True), Device(c["cw"], "critic", 2, 1, True)
    obs, act = torch.as_tensor(c["obs"]).cuda(), torch.as_tensor(c["act"]).cuda()
    sd = torch.tensor([0.125], dtype=torch.float32, device="cuda")
    out = torch.full((11,), 7.0, dtype=torch.float64, device="cuda")       # every slot is written, NaN included
    got = launch(ssc, actor, critic, None, obs, act, None, sd, out=out).cpu().numpy()
    assert np.all(np.isnan(got[[0, 1, 8, 9]])) and got[10] == 0.125 and np.all(np.isfinite(got[2:8]))


@pytest.mark.parametrize("c", [100.0, -3.25])
@pytest.mark.parametrize("m", [17, 1000])
def test_reduction_in_isolation(ssc, c, m):
    """Zero hidden weights and b3 = c: every row of a stream carries the same value, so the mean IS that value and the std
    is 0 up to f64 rounding (2^-40 relative; the tile means and Chan's merge give exactly c and 0).  sum(x^2) / n - mean^2
    in fp32 or with fp32 partials does not get there.  Q = c exactly; the actor's constant is tanh_fast(c) as
    ssc_actor_forward returns it for one row (1.0 for c = 100)."""
    from smartstartcontinuous_amd import _ffi
    rng = np.random.default_rng(3)
    zero = lambda i, h1, x, h2, o: dict(W1=np.zeros((i, h1), np.float32), b1=np.zeros(h1, np.float32),
                                        W2=np.zeros((h1 + x, h2), np.float32), b2=np.zeros(h2, np.float32),
                                        W3=np.zeros((h2, o), np.float32), b3=np.full(o, c, np.float32))
    actor, critic = Device(zero(3, 64, 0, 32, 2), "actor", 3, 2, False), Device(zero(3, 64, 2, 32, 1), "critic", 3, 2, False)
    obs = torch.as_tensor(rng.uniform(-1, 1, size=(m, 3)).astype(np.float32)).cuda()
    act = torch.as_tensor(rng.uniform(-1, 1, size=(m, 2)).astype(np.float32)).cuda()
    one = torch.empty((1, 2), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().ssc_actor_forward(ctypes.byref(actor.desc), 1, _ffi.ptr(obs), _ffi.ptr(one),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    c_act = float(one[0, 0].item())
    assert abs(c_act - np.tanh(c)) <= 1e-6 and float(one[0, 1].item()) == c_act
    got = launch(ssc, actor, critic, actor, obs, act).cpu().numpy()
    eps = 2.0 ** -40
    for slot, value in ((2, c), (4, c), (6, c_act), (8, c_act)):
        print(f"c {c} m {m} slot {slot}: mean - value {got[slot] - value:.3g}, std {got[slot + 1]:.3g}")
        assert abs(got[slot] - value) <= eps * abs(value), (slot, got[slot], value)
        assert 0.0 <= got[slot + 1] <= eps * abs(value), (slot, got[slot + 1])


# ---- the agent's methods -------------------------------------------------------------------------------------------
def make_agent(ssc, **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    args = dict(batch_size=64, num_train_iterations=3, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True,
                seed=7, actor_lr=1e-3, critic_lr=1e-2)
    args.update(kw)
    return DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, **args)


def device_ring(ssc, seed=3, chunks=1):
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    env = ssc.VecEnv(ENV, 64, seed=5)
    env.reset()
    replay = DeviceReplayBuffer(1 << 12, env.obs_dim, 1, env.device, seed=seed)
    for _ in range(chunks):
        replay.append_chunk(env.rollout(8, ssc.RandomPolicy()))
    return env, replay


def oracle_stats(agent, obs, act):
    aw = {k: v.cpu().numpy() for k, v in agent.weights.items()}
    cw = {k: v.cpu().numpy() for k, v in agent.critic_weights.items()}
    x = obs.astype(np.float64)
    a = O.actor_forward(x, **oracle_kw(aw), last_layer_tanh=True, obs_clip=CLIP)
    q = O.critic_forward(x, act, **oracle_kw(cw), last_layer_tanh=True, obs_clip=CLIP)[:, 0]
    qpi = O.critic_forward(x, a, **oracle_kw(cw), last_layer_tanh=True, obs_clip=CLIP)[:, 0]
    return dict(reference_Q_mean=q.mean(), reference_Q_std=q.std(), reference_actor_Q_mean=qpi.mean(),
                reference_actor_Q_std=qpi.std(), reference_action_mean=a.mean(), reference_action_std=a.std())


def test_get_stats_device_replay(ssc):
    agent = make_agent(ssc)
    env, replay = device_ring(ssc)
    first = agent.get_stats(replay)
    assert list(first) == list(agent.STATS_NAMES[2:8])
    obs, act = (t.clone() for t in agent.stats_sample)
    assert obs.shape == (64, 2) and act.shape == (64, 1)
    ring_rows = {tuple(r) for r in torch.cat([replay.s, replay.a], 1)[:len(replay)].cpu().numpy().tolist()}
    assert all(tuple(r) in ring_rows for r in torch.cat([obs, act], 1).cpu().numpy().tolist())     # records of the ring
    ref = oracle_stats(agent, obs.cpu().numpy(), act.cpu().numpy())
    for k, v in ref.items():
        assert abs(first[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, first[k], v)
    replay.append_chunk(env.rollout(8, ssc.RandomPolicy()))              # further appends: the same rows
    assert agent.get_stats(replay) == first
    assert torch.equal(agent.stats_sample[0], obs) and torch.equal(agent.stats_sample[1], act)
    assert agent.train_from(replay, 3) is not None
    after = agent.get_stats(replay)
    assert after["reference_Q_mean"] != first["reference_Q_mean"] and after["reference_actor_Q_mean"] != first["reference_actor_Q_mean"]
    assert torch.equal(agent.stats_sample[0], obs) and torch.equal(agent.stats_sample[1], act)
    ref = oracle_stats(agent, obs.cpu().numpy(), act.cpu().numpy())
    for k, v in ref.items():
        assert abs(after[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, after[k], v)


def test_get_stats_host_replay(ssc):
    import random
    agent = make_agent(ssc, param_noise_stddev=0.2, normalize_observations=True, training=False)
    rng = np.random.default_rng(2)

    def add(n):
        for _ in range(n):
            s = rng.uniform(-1, 0.5, size=2)
            agent.observe(s, rng.uniform(-1, 1, size=1), float(rng.normal()), s + 0.01, False)
    add(150)
    random.seed(5)
    first = agent.get_stats()
    assert random.random() == random.Random(5).random()                  # the host sampler's state did not move
    assert list(first) == list(agent.STATS_NAMES)
    assert first["param_noise_stddev"] == pytest.approx(0.2)
    obs, act = (t.clone() for t in agent.stats_sample)
    add(40)
    second = agent.get_stats()
    assert torch.equal(agent.stats_sample[0], obs) and torch.equal(agent.stats_sample[1], act)
    # the sample stayed, the observation statistics moved on: only slots that read them may differ
    assert second["obs_rms_mean"] != first["obs_rms_mean"]
    agent.training_enabled = True
    assert agent.train() is not None
    third = agent.get_stats()
    assert third["reference_Q_mean"] != second["reference_Q_mean"]
    assert torch.equal(agent.stats_sample[0], obs) and torch.equal(agent.stats_sample[1], act)
    explicit = make_agent(ssc)
    explicit.set_stats_sample(obs.cpu().numpy(), act)                    # host array and device tensor
    assert torch.equal(explicit.stats_sample[0], obs) and list(explicit.get_stats()) == list(agent.STATS_NAMES[2:8])


def test_stats_sample_leaves_the_learners_batches_alone(ssc):
    agent = make_agent(ssc)
    _, ring_a = device_ring(ssc)
    _, ring_b = device_ring(ssc)
    agent.get_stats(ring_a)
    idx_a, idx_b = ring_a.sample_indices(2, 64), ring_b.sample_indices(2, 64)
    assert torch.equal(idx_a, idx_b) and ring_a._batches_drawn == ring_b._batches_drawn == 2
    sample = torch.cat(list(agent.stats_sample), 1).cpu().numpy()
    batch = torch.cat([ring_a.s, ring_a.a], 1)[idx_a[0].long()].cpu().numpy()
    assert not np.array_equal(sample, batch)                             # a draw of its own, not the learner's next batch
