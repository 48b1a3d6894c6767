"""The SmartStart selection chain on the GPU (csrc/smartstart.hip: kde_kernel<1|2|3|0>, ucb_kernel; csrc/replay.hip:
smart_start_indices_kernel, episode_path_kernel; smartstart.kde_scott_bandwidth, device_smart_start_path) held to the
fp64 oracle by the bounds of tests/select_cases.py: |pdf - ref| <= C_KDE * 2^-24 * A_i for every query of every case and
|ucb - ref| <= C_UCB * 2^-24 * A_i for every candidate, both fixed on the CPU from a float32 emulation of the kernel's
arithmetic (tests/test_select_cases_cpu.py) -- about what float32 costs, where tests/test_gpu_agents.py accepted 2e-4 and
1e-4.  Then what no error bound pins: identical bits for identical queries, the flush to zero, the output buffer past m,
the argmax's lowest-index rule through the wave shuffle and the four-wave epilogue, +inf scores, the NaN policy (a NaN
score never wins; every score NaN -> index 0, where np.argmax returns the first NaN), the d_ucb = NULL form, the whole
chain on a MountainCar and a Pendulum ring, and the index sampler's four-slots-per-thread layout and exhausted rounds.

Measured on an MI355X (worst |err| / bound per instantiation): NOTEBOOK §18."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import select_cases as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _dev(x):
    return torch.as_tensor(np.array(x), device="cuda")       # (a copy: the case data is read-only)


def kde_device(data, points, wh, norm):
    """ssc_kde_evaluate into a NaN-prefilled buffer of m + PAD floats -> numpy [m + PAD]"""
    from smartstartcontinuous_amd import _ffi
    n, d = data.shape
    m = len(points)
    pdf = torch.full((m + S.PAD,), float("nan"), dtype=torch.float32, device="cuda")
    whc = (ctypes.c_float * (d * d))(*np.asarray(wh, np.float32).reshape(-1).tolist())
    dt, pt = _dev(data), _dev(points)
    _ffi.check(_ffi.lib().ssc_kde_evaluate(d, n, _ffi.ptr(dt), m, _ffi.ptr(pt), whc, float(norm), _ffi.ptr(pdf), _ffi.stream()))
    torch.cuda.synchronize()
    return pdf.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _kde_of(name):
    """the kernel's output buffer for a case: one launch per case, shared by the tests below, never modified"""
    cd = S.kde_case_data(S.KDE_CASE_BY_NAME[name])
    out = kde_device(cd["data"], cd["points"], cd["wh"], cd["norm"])
    out.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------------------------------- KDE --
@pytest.mark.parametrize("case", S.KDE_CASES, ids=lambda c: c.name)
def test_kde_within_float32_bound_of_oracle(ssc, case):
    r, x = S.kde_reference(case), _kde_of(case.name)
    worst = S.kde_distance(x, r["ref"], r["bound"])
    print("SELECT_MATRIX %s %s worst |pdf - ref| / bound = %.3f" % (case.name, case.kernel, worst))
    assert np.all(np.abs(x[:case.m].astype(np.float64) - r["ref"]) <= r["bound"]), worst


@pytest.mark.parametrize("case", S.KDE_CASES, ids=lambda c: c.name)
def test_kde_bits(ssc, case):
    """identical queries give identical bits whatever their slot and block; a query no float32 term of which survives gives
    exactly 0.0 (or, should the hardware keep denormal terms, a value within the floor norm * n * 2^-126); the buffer past
    m still holds the NaN it was filled with"""
    cd, r, x = S.kde_case_data(case), S.kde_reference(case), _kde_of(case.name)
    for i, src in cd["dup_of"].items():
        assert x[i].tobytes() == x[src].tobytes(), (i, src)
    fl = x[:case.m][r["flushed"]]
    assert np.all((fl == 0.0) | ((fl > 0.0) & (fl <= cd["norm"] * case.n * S.FLUSH))), fl
    assert np.isnan(x[case.m:]).all() and np.isfinite(x[:case.m]).all() and (x[:case.m] >= 0.0).all()


def _cpu_order_spread(data):
    """What two fp64 summation orders of Scott's covariance differ by on the CPU: O.kde_scott (np.cov) against the
    two-pass form kde_scott_bandwidth uses, summed sequentially over the rows in reverse -> (max |wh - wh'|, |norm'/norm - 1|)"""
    x = np.asarray(data, np.float64)[::-1]
    n, d = x.shape
    xc = x - np.cumsum(x, axis=0)[-1] / n
    cov = np.cumsum(xc[:, :, None] * xc[:, None, :], axis=0)[-1] / (n - 1) * (n ** (-1.0 / (d + 4))) ** 2
    wh = np.linalg.cholesky(np.linalg.inv(cov)).T
    norm = 1.0 / (n * np.sqrt(np.linalg.det(2 * np.pi * cov)))
    _, wh_ref, norm_ref = O.kde_scott(data)
    return float(np.abs(wh - wh_ref).max()), float(abs(norm / norm_ref - 1.0))


@pytest.mark.parametrize("case", [c for c in S.KDE_CASES if c.n >= c.d + 2], ids=lambda c: c.name)
def test_kde_scott_bandwidth(ssc, case):
    """kde_scott_bandwidth (fp64 moments on the device, d x d algebra on the host) against O.kde_scott.  The whitening
    must be float32(wh_ref) to within the larger of one float32 ulp and what two fp64 covariance orders differ by on the
    CPU on that data; the latter is 0 .. 2.8e-10 absolute, 4e-5 float32 ulp at the most (rho = 0.999, n = 9217), so the
    ulp decides everywhere.  norm: the CPU orders agree to 1e-12 on every data set but the rho = 0.999 ones (the
    covariance's condition number 500 enters the determinant: 5e-13 .. 2.7e-12 there), so norm is held to the larger of
    1e-12 and 4 x the CPU spread -- a third order is a third draw of the same rounding."""
    from smartstartcontinuous_amd import smartstart as SS
    data = S.kde_case_data(case)["data"]
    wh, norm = SS.kde_scott_bandwidth(_dev(data))
    _, wh_ref, norm_ref = O.kde_scott(data)
    wh_spread, norm_spread = _cpu_order_spread(data)
    want = wh_ref.astype(np.float32)
    tol = np.maximum(np.spacing(np.abs(want)).astype(np.float64), wh_spread)
    print("SELECT_MATRIX scott %s cpu spread wh %.1e norm %.1e; device |wh - f32(ref)| / ulp = %.2f, |norm / ref - 1| = %.1e" % (
        case.name, wh_spread, norm_spread, float((np.abs(wh.astype(np.float64) - want) / np.spacing(np.abs(want) + 1e-30)).max()),
        abs(norm / norm_ref - 1.0)))
    assert wh.dtype == np.float32 and wh.shape == (case.d, case.d)
    assert np.all(np.abs(wh.astype(np.float64) - want.astype(np.float64)) <= tol)
    assert np.all(wh[np.tril_indices(case.d, -1)] == 0.0)
    assert abs(norm / norm_ref - 1.0) <= max(1e-12, 4.0 * norm_spread)


# -------------------------------------------------------------------------------------------------------------- UCB --
def ucb_device(values, pdf, case, want_ucb=True):
    """ssc_ucb_argmax through _ffi -> (ucb numpy [m] or None with d_ucb = NULL, best)"""
    from smartstartcontinuous_amd import _ffi
    m = len(values)
    v, p = _dev(values), _dev(pdf)
    ucb = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda") if want_ucb else None
    best = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _ffi.check(_ffi.lib().ssc_ucb_argmax(m, _ffi.ptr(v), _ffi.ptr(p), float(case.alpha), float(case.beta), float(case.buffer_len),
                                         float(case.volume), _ffi.ptr(ucb), _ffi.ptr(best), _ffi.stream()))
    torch.cuda.synchronize()
    return (ucb.cpu().numpy() if want_ucb else None), int(best.item())


@pytest.mark.parametrize("case", S.UCB_CASES, ids=lambda c: c.name)
def test_ucb_within_bound_and_exact_argmax(ssc, case):
    """every placement of the winner: scores within the bound where the reference is finite, exactly +inf where pdf = 0,
    NaN where the reference is NaN; best is np.argmax of the kernel's own scores (the lowest index on ties) with NaN
    scores left out, index 0 when there is nothing else; the placed winner wins; the reference score of best is within
    the two bounds of the reference's maximum; d_ucb = NULL returns the same best"""
    worst = 0.0
    for label, v, p, want_best in S.ucb_placements(case):
        ref, A = S.ucb_scale(v, p, case)
        bound = S.C_UCB * S.EPS32 * A
        ucb, best = ucb_device(v, p, case)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(ucb), np.isnan(ref)), label
        assert np.array_equal(np.isposinf(ucb), np.asarray(p) == 0.0), label
        if fin.any():
            worst = max(worst, float(np.max(np.abs(ucb[fin] - ref[fin]) / bound[fin])))
            assert np.all(np.abs(ucb[fin] - ref[fin]) <= bound[fin]), (label, worst)
        if np.isnan(ucb).all():
            assert best == 0, label
        else:
            assert best == int(np.nanargmax(ucb)) and not np.isnan(ucb[best]), (label, best)
            if not np.isnan(ucb).any():
                assert best == int(np.argmax(ucb)), label
            star = int(np.nanargmax(ref))
            assert np.isposinf(ref[best]) or ref[best] >= ref[star] - bound[best] - bound[star], label
        if want_best is not None:
            assert best == want_best, (label, best, want_best)
        if label == "dup":
            star, copies = S.UCB_DUP_ROWS[case.m]
            assert len({ucb[r].tobytes() for r in (star, *copies)}) == 1
        assert ucb_device(v, p, case, want_ucb=False)[1] == best, label
    print("SELECT_MATRIX %s ucb_kernel worst |ucb - ref| / bound = %.3f" % (case.name, worst))


def test_ucb_nan_policy(ssc):
    """A NaN score -- from a NaN value or a NaN density -- never wins, whichever wave and stride it sits in; when every score
    is NaN the result is index 0.  (np.argmax would return the first NaN: the kernel deliberately differs)"""
    case = S.UCB_CASE_BY_NAME["u1000"]
    v, p = (x.copy() for x in S.ucb_base(case))
    ref, _ = S.ucb_scale(v, p, case)
    order = np.argsort(-ref)
    v[order[:3]] = np.nan                      # the three best candidates drop out ...
    p[order[3]] = np.nan                       # ... and the fourth by its density
    v[[0, 63, 64, 255, 256, 999]] = np.nan     # and the corners of the thread layout
    keep = [i for i in order if not (np.isnan(v[i]) or np.isnan(p[i]))]
    ref2, A2 = S.ucb_scale(v, p, case)
    assert ref2[keep[0]] - ref2[keep[1]] > 8 * S.C_UCB * S.EPS32 * A2[keep[0]]        # premise: the survivor leads clearly
    ucb, best = ucb_device(v, p, case)
    assert best == keep[0] and np.array_equal(np.isnan(ucb), np.isnan(ref2))
    for m in (1, 64, 257):
        c = S.UCB_CASE_BY_NAME["u%d" % m]
        _, p0 = S.ucb_base(c)
        assert ucb_device(np.full(m, np.nan, np.float32), p0, c)[1] == 0
        assert ucb_device(np.full(m, np.nan, np.float32), p0, c, want_ucb=False)[1] == 0


# ------------------------------------------------------------------------------------------------------------ chain --
def ring_reference(replay, n_envs):
    """host copies of a device ring and the oracle's view of it: dict(count, cap, size, eps, valid, s, s2, all_states)"""
    count, cap = replay.count, replay.capacity
    size = min(count, cap)
    eps = replay.ep_steps.cpu().numpy()
    s, s2 = replay.s.cpu().numpy(), replay.s2.cpu().numpy()
    order = (np.arange(size) + count - size) % cap
    return dict(count=count, cap=cap, size=size, eps=eps, valid=O.smart_start_valid(eps, cap, count, n_envs), s=s, s2=s2,
                all_states=np.concatenate([s[order], s2[(count - 1) % cap][None]]))


def assert_chain_against_oracle(replay, agent, radii, n_ss, n_envs, seed, max_len=1001):
    """device_smart_start_path on ``replay`` (its first index query) against the oracle fed the ring's contents.

    Candidates and path are integer work: bit-equal to O.smart_start_indices / O.replay_episode_path.  The winner is
    decided by float32 scores, the reference's by fp64 ones; the device's is accepted when

        ucb_ref[chosen] >= ucb_ref.max() - bound[chosen] - bound[best],

    bound = S.chain_bound: ucb_kernel's own bound (C_UCB 2^-24 A) at inputs that differ from the reference's by the
    critic's tolerance tol_V = 2e-5 max(1, |V|max) and by the KDE bound delta_i = C_KDE 2^-24 A_i of each density, plus
    what those two move the score itself: d ucb / d V = alpha, and with bonus B = K pdf^-1/2, d B / d pdf = -B / (2 pdf),
    taken without linearising as B ((1 - delta / pdf)^-1/2 - 1).  (If the device ranks chosen above best, then
    X[chosen] >= X[best] with |X - ref| <= bound on both sides.)  The densities are the oracle's under the bandwidth
    kde_scott_bandwidth returns for the ring -- the kernel's input, itself held to O.kde_scott by test_kde_scott_bandwidth.
    -> (worst KDE |err| / bound over the candidates, margin used / margin allowed, margin allowed / |ucb[best]|)"""
    from smartstartcontinuous_amd import smartstart as SS
    assert replay._queries == 0
    path, chosen = SS.device_smart_start_path(replay, agent, radii, n_ss=n_ss)
    torch.cuda.synchronize()
    g = ring_reference(replay, n_envs)
    idx = O.smart_start_indices(g["valid"], n_ss, seed ^ 0x5353, 0)
    idx = idx[idx >= 0]
    replay._queries = 0                        # the same key again: the candidate set itself, bit for bit
    assert np.array_equal(replay.get_possible_smart_start_indices(n_ss).cpu().numpy(), idx) and len(idx) >= n_ss // 2
    cand = g["s2"][(idx + g["count"] - g["size"]) % g["cap"]]
    wh, norm = SS.kde_scott_bandwidth(torch.as_tensor(g["all_states"], device="cuda"))
    k = S.kde_scale(g["all_states"], cand, wh, norm)
    pdf_bound = S.C_KDE * S.EPS32 * k["A"]
    pdf_dev = SS.kde_evaluate(torch.as_tensor(g["all_states"], device="cuda"), torch.as_tensor(cand, device="cuda"), wh, norm)
    kde_worst = float(np.max(np.abs(pdf_dev.cpu().numpy().astype(np.float64) - k["ref"]) / pdf_bound))
    assert kde_worst <= 1.0
    cw = {kk: v.cpu().numpy().astype(np.float64) for kk, v in agent.critic_weights.items()}
    aw = {kk: v.cpu().numpy().astype(np.float64) for kk, v in agent.weights.items()}
    c64 = cand.astype(np.float64)
    values = O.critic_forward(c64, O.actor_forward(c64, **aw, obs_clip=5.0), **cw, obs_clip=5.0)[:, 0]
    case = S.UcbCase("chain", len(idx), 1.0, 2.0, g["size"], O.hyperellipsoid_volume(radii))
    ucb, best = O.smart_start_ucb(values, k["ref"], case.buffer_len, case.volume, case.alpha, case.beta)
    bound = S.chain_bound(values, k["ref"], pdf_bound, case)
    pos = int(np.nonzero(idx == int(chosen.item()))[0][0])
    assert ucb[pos] >= ucb[best] - bound[pos] - bound[best], (ucb[pos], ucb[best], bound[pos], bound[best])
    want = O.replay_episode_path(g["s"], g["s2"], g["eps"], g["cap"], g["count"], n_envs, int(chosen.item()), max_len)
    assert np.array_equal(path.cpu().numpy(), want) and path.shape[0] >= 2
    return kde_worst, float((ucb[best] - ucb[pos]) / (bound[pos] + bound[best])), float((bound[pos] + bound[best]) / abs(ucb[best]))


@pytest.mark.parametrize("env_name,obs_dim,radii", [("MountainCarContinuous-v0", 2, (0.01, 0.002)), ("Pendulum-v1", 3, (0.05, 0.05, 0.4))])
def test_chain_against_oracle(ssc, env_name, obs_dim, radii):
    """device_smart_start_path end to end on a ring of 64 envs x 2 chunks x 40 steps (5120 records: the KDE's n = 5121 is
    a trip, a full slot and one point): MountainCar runs kde_kernel<2>, Pendulum kde_kernel<3> on ring data"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    n, K = 64, 40
    env = ssc.VecEnv(env_name, n, seed=21, max_episode_steps=25)
    one = ssc.SingleEnvView(ssc.VecEnv(env_name, 1, seed=21))
    agent = DDPG_Baselines_agent(one, None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=2)
    replay = DeviceReplayBuffer(6000, obs_dim, 1, seed=4, track_episodes=True, n_envs=n)
    for _ in range(2):
        replay.append_chunk(env.rollout(K, ssc.RandomPolicy()))
    kde_worst, margin, rel = assert_chain_against_oracle(replay, agent, np.array(radii), 200, n, 4)
    print("SELECT_MATRIX chain %s kde worst |pdf - ref| / bound = %.3f, decision margin used = %.3f of the allowed, "
          "allowed margin / |ucb| = %.1e" % (env_name, kde_worst, margin, rel))


# --------------------------------------------------------------------------------------------------- index sampler --
def _fake_ring(ssc, obs_dim, n, K, done, cap, max_path_len=1001, seed=9, chunks=1):
    """a DeviceReplayBuffer fed K steps of n envs in ``chunks`` equal appends, with recognisable content:
    obs = (step, env, step + env / 1024)[:obs_dim], obs2 = the same one step on"""
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    replay = DeviceReplayBuffer(cap, obs_dim, 1, seed=seed, track_episodes=True, n_envs=n, max_path_len=max_path_len)
    Kc = K // chunks
    assert Kc * chunks == K and Kc * n <= cap
    for c0 in range(0, K, Kc):
        chunk = ssc.TransitionChunk(obs_dim, Kc, n, "cuda")
        k = (torch.arange(Kc, dtype=torch.float32, device="cuda")[:, None] + float(c0)).expand(Kc, n)
        e = torch.arange(n, dtype=torch.float32, device="cuda")[None, :].expand(Kc, n)
        cols = [k, e, k + e / 1024.0]
        for c in range(obs_dim):
            chunk.obs[c].copy_(cols[c])
            chunk.obs2[c].copy_(cols[c] + (1.0 if c != 1 else 0.0))
        chunk.act.zero_()
        chunk.rew.zero_()
        chunk.done.copy_(torch.as_tensor(done[c0:c0 + Kc], dtype=torch.uint8, device="cuda"))
        chunk.step0 = c0
        replay.append_chunk(chunk)
    return replay


@pytest.mark.parametrize("n_ss", [1025, 4096])
def test_sampler_slots_beyond_the_first_per_thread(ssc, n_ss):
    """n_ss > 1024: slots 1..3 of smart_start_indices_kernel's four-slots-per-thread layout run (1025: one thread holds a
    second slot; 4096: every thread holds four), on a ring with more than 4096 valid records"""
    n, K = 100, 60
    done = (np.random.default_rng(n_ss).random((K, n)) < 0.05).astype(np.uint8)
    replay = _fake_ring(ssc, 2, n, K, done, 8192)
    g = ring_reference(replay, n)
    assert g["valid"].sum() > 4096
    got = replay.get_possible_smart_start_indices(n_ss).cpu().numpy()
    want = O.smart_start_indices(g["valid"], n_ss, 9 ^ 0x5353, 0)
    assert np.array_equal(got, want[want >= 0]) and len(got) == n_ss and len(set(got.tolist())) == n_ss and g["valid"][got].all()


def test_sampler_runs_out_of_rounds(ssc):
    """three valid records, 64 slots: after the 64 rounds three slots hold the three records, every other slot is -1"""
    from smartstartcontinuous_amd import _ffi
    n, K, cap = 1, 40, 30                                   # the ring keeps records 10..39: episodes that began before are invalid
    done = np.zeros((K, n), np.uint8)
    done[36, 0] = 1                                         # ... and records 37, 38, 39 open the one episode that starts inside
    replay = _fake_ring(ssc, 2, n, K, done, cap, chunks=2)
    g = ring_reference(replay, n)
    assert np.nonzero(g["valid"])[0].tolist() == [27, 28, 29]
    want = O.smart_start_indices(g["valid"], 64, 9 ^ 0x5353, 0)
    assert sorted(want[want >= 0].tolist()) == [27, 28, 29] and (want < 0).sum() == 61
    idx = torch.full((64,), -9, dtype=torch.int32, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    nb = _ffi.lib().ssc_replay_smart_start_workspace_bytes(64)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ring = replay.ring_struct()
    _ffi.check(_ffi.lib().ssc_replay_smart_start_indices(ctypes.byref(ring), replay.count, n, 64, 9 ^ 0x5353, 0, _ffi.ptr(idx),
                                                         _ffi.ptr(n_out), _ffi.ptr(ws), nb, _ffi.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want) and int(n_out.item()) == 3
    assert replay.get_possible_smart_start_indices(64).cpu().numpy().tolist() == want[want >= 0].tolist()


@pytest.mark.parametrize("obs_dim", [2, 3])
def test_episode_path_truncated_to_max_path_len(ssc, obs_dim):
    """max_path_len = 4 against episodes of 10+ steps: 5 rows, the newest four states and the record's s2; obs_dim 3 is the
    Pendulum layout of the ring"""
    n, K = 7, 30
    done = np.zeros((K, n), np.uint8)
    done[11, :] = 1
    short = _fake_ring(ssc, obs_dim, n, K, done, 1000, max_path_len=4)
    full = _fake_ring(ssc, obs_dim, n, K, done, 1000)
    g = ring_reference(short, n)
    for k_rec, e in [(10, 3), (11, 0), (29, 6), (14, 2), (12, 5)]:       # episode steps 11, 12, 18, 3, 1
        bi = k_rec * n + e
        L = int(g["eps"][bi])
        assert L == (k_rec + 1 if k_rec <= 11 else k_rec - 11)
        path = short.get_episodic_path_to_buffer_index(bi).cpu().numpy()
        want = O.replay_episode_path(g["s"], g["s2"], g["eps"], g["cap"], g["count"], n, bi, 4)
        assert np.array_equal(path, want) and path.shape == (min(L, 4) + 1, obs_dim)
        whole = full.get_episodic_path_to_buffer_index(bi).cpu().numpy()
        assert np.array_equal(whole, O.replay_episode_path(g["s"], g["s2"], g["eps"], g["cap"], g["count"], n, bi, 1001))
        assert whole.shape[0] == L + 1 and np.array_equal(path, whole[-path.shape[0]:])      # the NEWEST steps
