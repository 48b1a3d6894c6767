"""The six population-selection calls over ``ssc_select_many_item`` (ssc_replay_smart_start_indices_many,
ssc_kde_scott_bandwidth_many, ssc_critic_forward_many, ssc_kde_evaluate_many, ssc_ucb_topk_many,
ssc_replay_episode_path_many), stage by stage, in guarded buffers compared whole:

(a) every output of item p in a call of P items (an empty item in the middle) equals, bit for bit, the same call with that
    item alone;
(b) every stage but the bandwidth equals today's per-pair call on the same input, bit for bit: indices and n_cand
    (ssc_replay_smart_start_indices), candidates (``replay.s2[replay.physical(idx)]``), values (``state_value_device``), pdf
    (``kde_evaluate`` on the materialised ``get_all_states()[::stride]`` with the grouped path's own wh / norm), ucb and
    argmax (``ucb_argmax``), paths (``get_episodic_path_to_buffer_index``);
(c) the bandwidth against O.kde_scott at the tolerances tests/test_gpu_select_matrix.py::test_kde_scott_bandwidth holds the
    host function to, on the same cases, and the chosen list of the MountainCar and Pendulum rings of that file's chain test
    as a valid top-k under select_cases' bounds (tests/select_many_cases.py: topk_valid).
The table of items: tests/select_many_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import select_cases as S
from tests import select_many_cases as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = 8
VOLUME, ALPHA, BETA = 0.37, 1.0, 2.0
STAGES = ("indices", "bandwidth", "actor", "critic", "kde", "topk", "paths")
OUTPUTS = ("idx", "n_cand", "cand", "wh", "norm", "status", "value", "pdf", "ucb", "chosen", "path", "len")


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


@functools.lru_cache(maxsize=None)
def _agent(net, env_name="MountainCarContinuous-v0"):
    import smartstartcontinuous_amd as ssc
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    one = ssc.make(env_name)
    if net == "small":
        return DDPG_Baselines_agent(one, None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=2,
                                    training=False, precision="f32")
    a = DDPG_Baselines_agent(one, None, actor_h1=200, actor_h2=100, critic_h1=200, critic_h2=100, lastLayerTanh=False, seed=3,
                             training=False, precision="f32", layer_norm=True, normalize_observations=True)
    a.obs_rms.update_rows(np.random.default_rng(3).normal(0.2, 1.5, (50, 2)).astype(np.float32))
    return a


def _ring_from(arr, d, cap, n_envs, max_len, seed=7):
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    r = DeviceReplayBuffer(cap, d, 1, "cuda", seed=seed, track_episodes=True, n_envs=n_envs, max_path_len=max_len)
    r.s.copy_(torch.as_tensor(arr["s"]))
    r.s2.copy_(torch.as_tensor(arr["s2"]))
    r.ep_steps.copy_(torch.as_tensor(arr["ep_steps"]))
    r.count = int(arr["count"])
    return r


@functools.lru_cache(maxsize=None)
def _ring(name, d):
    item = {it.name: it for it in M.ITEMS_2D + [x for v in M.ITEMS_ND.values() for x in v]}[name]
    return _ring_from(M.ring_arrays(item, d, seed=len(name) + 31 * d), d, item.cap, item.n_envs, item.max_len)


class Entry:
    """one item of a call: its spec, ring, agent and guarded output buffers"""

    def __init__(self, item, ring, agent, counter=5):
        self.item, self.ring, self.agent, self.counter = item, ring, agent, counter
        d, n_ss, k = ring.obs_dim, item.n_ss, item.n_plans
        f = lambda n, dt, fill: torch.full((n + PAD,), fill, dtype=dt, device="cuda")
        nan = float("nan")
        self.buf = dict(idx=f(n_ss, torch.int32, -9), n_cand=f(1, torch.int32, -9), cand=f(n_ss * d, torch.float32, nan),
                        wh=f(d * d, torch.float32, nan), norm=f(1, torch.float64, nan), status=f(1, torch.int32, -9),
                        value=f(n_ss, torch.float32, nan), pdf=f(n_ss, torch.float32, nan), ucb=f(n_ss, torch.float32, nan),
                        chosen=f(k, torch.int32, -9), path=f(k * (item.max_len + 1) * d, torch.float32, nan),
                        len=f(k, torch.int32, -9))
        from smartstartcontinuous_amd import _ffi
        self.ws_bytes = int(_ffi.lib().ssc_replay_smart_start_workspace_bytes(n_ss))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device="cuda")

    @property
    def size(self):
        return len(self.ring)

    @property
    def n_data(self):
        return -(-(self.size + 1) // self.item.stride)

    def fill(self, it, row0):
        from smartstartcontinuous_amd import _ffi
        item, r, d = self.item, self.ring, self.ring.obs_dim
        it.ring, it.count, it.n = r.ring_struct(), r.count, r.n_envs
        it.n_ss, it.n_plans, it.max_len = item.n_ss, item.n_plans, item.max_len
        it.seed, it.counter = r.seed ^ 0x5353, self.counter
        it.stride, it.n_data = item.stride, self.n_data
        it.scott = (max(self.n_data, 1) ** (-1.0 / (d + 4))) ** 2
        if self.agent is not None:
            rms = getattr(self.agent, "obs_rms", None)
            it.actor, it.critic = self.agent._desc, self.agent._critic_desc
            it.d_rms = None if rms is None else rms.block.data_ptr()
        it.alpha, it.beta, it.volume, it.row0 = ALPHA, BETA, VOLUME, row0
        for k in OUTPUTS:
            setattr(it, "d_n_cand" if k == "n_cand" else "d_" + k, self.buf[k].data_ptr())
        it.d_workspace, it.workspace_bytes = self.ws.data_ptr(), self.ws_bytes

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.buf.items()}


def run(entries, stages=STAGES):
    """the stages over one table of ``entries`` -> per entry a dict of whole guarded buffers (numpy)"""
    from smartstartcontinuous_amd import _ffi
    from smartstartcontinuous_amd.population import DeviceItems
    lib, P = _ffi.lib(), len(entries)
    table = DeviceItems(_ffi.SelectManyItem, P, "cuda")
    row0, rows = [], 0
    for e in entries:
        row0.append(rows)
        rows += e.item.n_ss
    for it, e, r0 in zip(table.items, entries, row0):
        e.fill(it, r0)
    table.upload()
    act = torch.full((rows + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    st = _ffi.stream()
    args = (table.h_ptr, table.d_ptr, P)
    for stage in stages:
        if stage == "indices":
            _ffi.check(lib.ssc_replay_smart_start_indices_many(*args, st))
        elif stage == "bandwidth":
            _ffi.check(lib.ssc_kde_scott_bandwidth_many(*args, st))
        elif stage == "actor":
            for e, r0 in zip(entries, row0):
                if e.size == 0:
                    continue
                rms = getattr(e.agent, "obs_rms", None)
                obs, out = e.buf["cand"].data_ptr(), act.data_ptr() + 4 * r0
                if rms is None:
                    _ffi.check(lib.ssc_actor_forward(ctypes.byref(e.agent._desc), e.item.n_ss, obs, out, st))
                else:
                    _ffi.check(lib.ssc_actor_forward_rms(ctypes.byref(e.agent._desc), e.item.n_ss, obs, out, st, _ffi.ptr(rms.block)))
        elif stage == "critic":
            _ffi.check(lib.ssc_critic_forward_many(*args, rows, _ffi.ptr(act), st))
        elif stage == "kde":
            _ffi.check(lib.ssc_kde_evaluate_many(*args, st))
        elif stage == "topk":
            _ffi.check(lib.ssc_ucb_topk_many(*args, st))
        elif stage == "paths":
            _ffi.check(lib.ssc_replay_episode_path_many(*args, st))
    torch.cuda.synchronize()
    assert np.isnan(act[rows:].cpu().numpy()).all()
    return [e.host() for e in entries]


def _same(a, b, what):
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _guards(e, out):
    n_ss, k, d = e.item.n_ss, e.item.n_plans, e.ring.obs_dim
    lens = dict(idx=n_ss, n_cand=1, cand=n_ss * d, wh=d * d, norm=1, status=1, value=n_ss, pdf=n_ss, ucb=n_ss, chosen=k,
                path=k * (e.item.max_len + 1) * d, len=k)
    for name, n in lens.items():
        tail = out[name][n:]
        assert (np.isnan(tail).all() if tail.dtype.kind == "f" else (tail == -9).all()), (e.item.name, name)


@functools.lru_cache(maxsize=None)
def _all_2d():
    """the one call over the whole 2-d table -> (entries, outputs); read-only"""
    entries = [Entry(it, _ring(it.name, 2), _agent(it.net)) for it in M.ITEMS_2D]
    return entries, run(entries)


# ------------------------------------------------------------------------------------------------------------- (a) --
@pytest.mark.parametrize("item", M.ITEMS_2D, ids=lambda it: it.name)
def test_an_item_alone_gives_the_bits_of_its_grid_row(ssc, item):
    entries, outs = _all_2d()
    p = [it.name for it in M.ITEMS_2D].index(item.name)
    _guards(entries[p], outs[p])
    alone = Entry(item, _ring(item.name, 2), _agent(item.net))
    _same(outs[p], run([alone])[0], item.name)
    if item.ring == "empty":                                   # skipped: nothing of it is written
        for k in OUTPUTS:
            v = outs[p][k]
            assert np.isnan(v).all() if v.dtype.kind == "f" else (v == -9).all()


def test_three_items_with_an_empty_one_in_the_middle(ssc):
    by = {it.name: it for it in M.ITEMS_2D}
    entries, outs = _all_2d()
    names = [it.name for it in M.ITEMS_2D]
    three = [Entry(by[n], _ring(n, 2), _agent(by[n].net)) for n in ("rows65", "empty", "fresh_n5")]
    for e, o in zip(three, run(three)):
        _same(o, outs[names.index(e.item.name)], e.item.name)


# ------------------------------------------------------------------------------------------------------------- (b) --
def _reference_checks(ssc, e, out):
    """every stage of ``out`` against today's per-pair calls on the same input"""
    from smartstartcontinuous_amd import _ffi
    from smartstartcontinuous_amd import smartstart as SS
    item, r, d = e.item, e.ring, e.ring.obs_dim
    n_ss, k = item.n_ss, item.n_plans
    lib = _ffi.lib()
    # indices and n_cand: the single call into a buffer of its own, whole
    idx = torch.full((n_ss,), -9, dtype=torch.int32, device="cuda")
    n_out = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    ws = torch.zeros(e.ws_bytes, dtype=torch.uint8, device="cuda")
    ring = r.ring_struct()
    _ffi.check(lib.ssc_replay_smart_start_indices(ctypes.byref(ring), r.count, r.n_envs, n_ss, r.seed ^ 0x5353, e.counter,
                                                  _ffi.ptr(idx), _ffi.ptr(n_out), _ffi.ptr(ws), e.ws_bytes, _ffi.stream()))
    idx = idx.cpu().numpy()
    assert np.array_equal(out["idx"][:n_ss], idx) and out["n_cand"][0] == int(n_out.item()) == (idx >= 0).sum()
    live = idx >= 0
    r._queries = e.counter
    got = r.get_possible_smart_start_indices(n_ss)
    assert (got is None and not live.any()) or np.array_equal(got.cpu().numpy(), idx[live])
    # candidates
    cand = out["cand"][:n_ss * d].reshape(n_ss, d)
    want = np.zeros((n_ss, d), np.float32)
    if live.any():
        want[live] = r.s2[r.physical(torch.as_tensor(idx[live], device="cuda").long())].cpu().numpy()
    assert cand.tobytes() == want.tobytes()
    if e.agent is None:
        values = None
    else:
        values = e.agent.state_value_device(torch.as_tensor(cand, device="cuda")).cpu().numpy()
        assert out["value"][:n_ss].tobytes() == values.tobytes()
    status = int(out["status"][0])
    if status != 0:
        assert np.isnan(out["pdf"][:n_ss]).all()                                        # writes nothing
        assert (out["chosen"][:k] == -1).all() and (out["len"][:k] == 0).all()
        return status
    wh, norm = out["wh"][:d * d].reshape(d, d), float(out["norm"][0])
    data = r.get_all_states()[::item.stride].contiguous()
    assert data.shape[0] == e.n_data
    pdf = SS.kde_evaluate(data, torch.as_tensor(cand, device="cuda"), wh, norm).cpu().numpy()
    assert out["pdf"][:n_ss].tobytes() == pdf.tobytes()
    if values is None:
        return status
    ucb = out["ucb"][:n_ss]
    assert np.isnan(ucb[~live]).all()
    chosen = out["chosen"][:k]
    assert np.array_equal(chosen, M.topk_rule(ucb, idx, k))
    if live.any():
        u_ref, best = SS.ucb_argmax(torch.as_tensor(values[live], device="cuda"), torch.as_tensor(pdf[live], device="cuda"),
                                    e.size, VOLUME, ALPHA, BETA)
        assert ucb[live].tobytes() == u_ref.cpu().numpy().tobytes()
        assert chosen[0] == idx[live][int(best.item())]                                 # the argmax, for any n_plans
    else:
        assert (chosen == -1).all()
    paths = out["path"][:k * (item.max_len + 1) * d].reshape(k, item.max_len + 1, d)
    for j in range(k):
        rows = int(out["len"][j])
        if chosen[j] < 0:
            assert rows == 0
            continue
        want = r.get_episodic_path_to_buffer_index(int(chosen[j])).cpu().numpy()
        assert rows == want.shape[0] <= item.max_len + 1 and paths[j, :rows].tobytes() == want.tobytes()
        assert np.isnan(paths[j, rows:]).all()
    return status


@pytest.mark.parametrize("item", [it for it in M.ITEMS_2D if it.ring != "empty"], ids=lambda it: it.name)
def test_every_stage_equals_todays_per_pair_call(ssc, item):
    entries, outs = _all_2d()
    p = [it.name for it in M.ITEMS_2D].index(item.name)
    status = _reference_checks(ssc, entries[p], outs[p])
    n_cand = int(outs[p]["n_cand"][0])
    if item.ring == "flat":
        assert status == 1
    elif item.name != "two_states":                # (two points in two dimensions: a singular covariance up to rounding)
        assert status == 0
    if item.ring == "gone":
        assert n_cand == 0 and (outs[p]["cand"][:item.n_ss * 2] == 0).all()
    if item.ring == "few":
        assert n_cand == 3 and (outs[p]["chosen"][:4] >= 0).sum() == 3 and outs[p]["chosen"][3] == -1
    if item.name == "wrapped_1025":
        assert n_cand == 1025 and (outs[p]["len"][:3] == item.max_len + 1).any()       # a path cut by max_len


@pytest.mark.parametrize("d", sorted(M.ITEMS_ND))
def test_other_state_dimensions(ssc, d):
    """d = 1, 3 and 4 (kde_kernel<1>, <3> and the D = 0 body): candidates, bandwidth and KDE, (a) and (b)"""
    stages = ("indices", "bandwidth", "kde")
    entries = [Entry(it, _ring(it.name, d), None) for it in M.ITEMS_ND[d]]
    outs = run(entries, stages)
    for e, o in zip(entries, outs):
        _guards(e, o)
        _same(o, run([Entry(e.item, e.ring, None)], stages)[0], e.item.name)
        assert _reference_checks(ssc, e, o) == 0


# ------------------------------------------------------------------------------------------------------------- (c) --
SCOTT_CASES = [c for c in S.KDE_CASES if c.n >= c.d + 2]


def _cpu_order_spread(data):
    """tests/test_gpu_select_matrix.py's measure: O.kde_scott against the two-pass form summed in reverse row order"""
    x = np.asarray(data, np.float64)[::-1]
    n, d = x.shape
    xc = x - np.cumsum(x, axis=0)[-1] / n
    cov = np.cumsum(xc[:, :, None] * xc[:, None, :], axis=0)[-1] / (n - 1) * (n ** (-1.0 / (d + 4))) ** 2
    wh = np.linalg.cholesky(np.linalg.inv(cov)).T
    norm = 1.0 / (n * np.sqrt(np.linalg.det(2 * np.pi * cov)))
    _, wh_ref, norm_ref = O.kde_scott(data)
    return float(np.abs(wh - wh_ref).max()), float(abs(norm / norm_ref - 1.0))


@functools.lru_cache(maxsize=None)
def _scott_outputs():
    """ONE bandwidth call over a ring per KDE case whose data set (states, then the newest s2) is the case's data"""
    entries = []
    for c in SCOTT_CASES:
        data = np.asarray(S.kde_case_data(c)["data"], np.float32)
        arr = dict(s=np.zeros((c.n, c.d), np.float32), s2=np.zeros((c.n, c.d), np.float32), ep_steps=np.ones(c.n, np.int32),
                   count=c.n - 1)
        arr["s"][:c.n - 1], arr["s2"][c.n - 2] = data[:-1], data[-1]
        item = M.Item(c.name, "fresh", 1, c.n - 1, c.n, 1, 1, 1, 4, None)
        entries.append(Entry(item, _ring_from(arr, c.d, c.n, 1, 4), None))
    return entries, run(entries, ("bandwidth",))


@pytest.mark.parametrize("case", SCOTT_CASES, ids=lambda c: c.name)
def test_bandwidth_against_the_oracle(ssc, case):
    entries, outs = _scott_outputs()
    p = [c.name for c in SCOTT_CASES].index(case.name)
    out, d = outs[p], case.d
    data = S.kde_case_data(case)["data"]
    assert np.array_equal(entries[p].ring.get_all_states().cpu().numpy(), np.asarray(data, np.float32))
    _guards(entries[p], out)
    wh, norm = out["wh"][:d * d].reshape(d, d), float(out["norm"][0])
    _, wh_ref, norm_ref = O.kde_scott(data)
    wh_spread, norm_spread = _cpu_order_spread(data)
    want = wh_ref.astype(np.float32)
    tol = np.maximum(np.spacing(np.abs(want)).astype(np.float64), wh_spread)
    print("SELECT_MANY scott %s device |wh - f32(ref)| / ulp = %.2f, |norm / ref - 1| = %.1e (cpu spread %.1e)" % (
        case.name, float((np.abs(wh.astype(np.float64) - want) / np.spacing(np.abs(want) + 1e-30)).max()), abs(norm / norm_ref - 1.0),
        norm_spread))
    assert int(out["status"][0]) == 0
    assert np.all(np.abs(wh.astype(np.float64) - want.astype(np.float64)) <= tol)
    assert np.all(wh[np.tril_indices(d, -1)] == 0.0)
    assert abs(norm / norm_ref - 1.0) <= max(1e-12, 4.0 * norm_spread)
    # the same bits run to run
    again = run([Entry(entries[p].item, entries[p].ring, None)], ("bandwidth",))[0]
    assert again["wh"].tobytes() == out["wh"].tobytes() and again["norm"].tobytes() == out["norm"].tobytes()


@pytest.mark.parametrize("env_name,obs_dim,radii", [("MountainCarContinuous-v0", 2, (0.01, 0.002)), ("Pendulum-v1", 3, (0.05, 0.05, 0.4))])
def test_chosen_list_is_a_valid_top_k_against_the_oracle(ssc, env_name, obs_dim, radii):
    """the rings of tests/test_gpu_select_matrix.py::test_chain_against_oracle (64 envs x 2 chunks x 40 steps), n_ss = 200,
    n_plans = 3: the chosen slots under the fp64 scores and select_cases.chain_bound"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    global VOLUME
    n, K, n_ss, k = 64, 40, 200, 3
    env = ssc.VecEnv(env_name, n, seed=21, max_episode_steps=25)
    one = ssc.SingleEnvView(ssc.VecEnv(env_name, 1, seed=21))
    agent = DDPG_Baselines_agent(one, None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=2)
    replay = DeviceReplayBuffer(6000, obs_dim, 1, seed=4, track_episodes=True, n_envs=n)
    for _ in range(2):
        replay.append_chunk(env.rollout(K, ssc.RandomPolicy()))
    volume = float(O.hyperellipsoid_volume(np.array(radii)))
    item = M.Item("chain", "fresh", n, len(replay), 6000, 1, n_ss, k, 1001, "small")
    old, VOLUME = VOLUME, volume
    try:
        e = Entry(item, replay, agent, counter=0)
        out = run([e])[0]
        assert _reference_checks(ssc, e, out) == 0
    finally:
        VOLUME = old
    idx = out["idx"][:n_ss]
    live = idx >= 0
    assert live.sum() >= n_ss // 2
    cand = out["cand"][:n_ss * obs_dim].reshape(n_ss, obs_dim)[live]
    wh, norm = out["wh"][:obs_dim ** 2].reshape(obs_dim, obs_dim), float(out["norm"][0])
    data = replay.get_all_states().cpu().numpy()
    kk = S.kde_scale(data, cand, wh, norm)
    pdf_bound = S.C_KDE * S.EPS32 * kk["A"]
    cw = {x: v.cpu().numpy().astype(np.float64) for x, v in agent.critic_weights.items()}
    aw = {x: v.cpu().numpy().astype(np.float64) for x, v in agent.weights.items()}
    c64 = cand.astype(np.float64)
    values = O.critic_forward(c64, O.actor_forward(c64, **aw, obs_clip=5.0), **cw, obs_clip=5.0)[:, 0]
    case = S.UcbCase("chain", int(live.sum()), ALPHA, BETA, len(replay), volume)
    ref, _best = O.smart_start_ucb(values, kk["ref"], case.buffer_len, case.volume, case.alpha, case.beta)
    bound = S.chain_bound(values, kk["ref"], pdf_bound, case)
    pos = {int(b): i for i, b in enumerate(idx[live])}
    chosen = [pos[int(c)] for c in out["chosen"][:k]]
    assert len(chosen) == k and M.topk_valid(chosen, ref, bound, np.ones(len(ref), bool))
