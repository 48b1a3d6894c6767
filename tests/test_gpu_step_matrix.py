"""mpc_rollout_step_kernel (csrc/rollout.hip) launch by launch: its six instantiations behind ssc_mpc_rollout_step,
ssc_smartstart_rollout_step and ssc_smartstart_rollout_step_many, called through ctypes on state this module owns, every
env put into the branch tests/step_cases.py wants and everything a launch writes held to the fp64 oracle by
step_cases.check_step (exact where the kernel decides or copies, the project's tolerances where it computes).  Then the
forms against each other, bit for bit: ``ss`` with every env navigating and eta = 0 against ``mpc``, every pair of ``many``
against its own ``ss`` launch, a strided log against no log.

Measured on an MI355X (worst error per asserted quantity and instantiation, as a fraction of its tolerance): NOTEBOOK §32."""
import ctypes

import numpy as np
import pytest

from tests import step_cases as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_VIEW = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


@pytest.fixture(scope="module")
def ffi():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def _up(a):
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a.view(_VIEW.get(a.dtype, a.dtype)).copy(), device="cuda")


def _down(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def _upload(dev):
    return {k: _up(v) for k, v in dev.items()}


def _readback(T, dev):
    torch.cuda.synchronize()
    return {k: _down(T[k], dev[k]) for k in dev}


def _at(t, elems=0):
    """device address of element ``elems`` of a tensor (None -> NULL)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _params(ffi, case, opts):
    p = ffi.default_params(ffi.SSC_ENV_MOUNTAINCAR if case.env == "mc" else ffi.SSC_ENV_PENDULUM, 1.0, S.MAX_STEPS)
    p.pend_v1_order = int(opts["v1"])
    return p


def _observe(ffi, case, opts, T, dev):
    """[n_alloc, OBS] observation of the state in T through the library's own observe (Pendulum: the kernels' sincosf)"""
    n = len(dev["s0"])
    out = torch.empty((S.OBS[case.env], n), device="cuda")
    ffi.check(ffi.lib().ssc_env_observe(ctypes.byref(_params(ffi, case, opts)), n, _at(T["s0"]), _at(T["s1"]), _at(out), ffi.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().T.copy()


def _launch(ffi, case, T, form=None, opts=None, env0=0, n=None, slot0=0, stats_row=0, pair_table=None):
    """one launch of the form's entry point on the tensors T; (env0, n, slot0): the slice of the envs and of the plan pool the
    call sees (a pair of the population as its own single launch)"""
    form, o = form or case.form, opts or case.opts
    n = case.n if n is None else n
    d = S.case_data(case)
    dim = S.OBS[case.env]
    rs, ds, ms = S.strides(case)
    packed = case.opts["log"] != "strided" and n == case.n           # (the arrays' layout is the case's, whatever ``opts`` leaves out)
    p = _params(ffi, case, o)
    pr = ffi.MpcProblems(n_problems=n, n_samples=S.N_SAMPLES, horizon=S.HORIZON, state_dim=dim, wp=_at(T["wp"]), left=_at(T["left"]),
                         wp_off=_at(T["wp_off"], slot0), cur_idx=_at(T["cur_idx"], env0), radii=_at(T["radii"], slot0 * dim),
                         theta=S.THETA, gamma=0.75, horizontal_penalty_factor=0.5, per_row_projection=0,
                         plan_of=_at(T["plan_of"], env0), wp_len=_at(T["wp_len"], slot0))
    nav = ffi.MpcNavState(cur_idx=_at(T["cur_idx"], env0), start_idx=_at(T["start_idx"], env0), actions_done=_at(T["actions_done"], env0),
                          at_goal=_at(T["at_goal"], env0) if o["at_goal"] else None, give_up_after=S.GIVE_UP, final_steps=S.FINAL_STEPS)
    st = ffi.RolloutState(s0=_at(T["s0"], env0), s1=_at(T["s1"], env0), steps=_at(T["steps"], env0), ep_ret=_at(T["ep_ret"], env0),
                          ou_x=_at(T["ou_x"], env0) if (form != "mpc" or o["ou_col"]) else None)
    log = None
    if o["log"] != "none":
        rows = S.log_rows(case)
        log = ffi.TransitionLog(act=_at(T["log_act"], env0), rew=_at(T["log_rew"], env0), done=_at(T["log_done"], env0),
                                row_stride=0 if packed else rs, done_row_stride=0 if packed else ds)
        for c in range(dim):
            log.obs[c] = T["log_obs"].data_ptr() + (c * rows * rs + env0) * 4
            log.obs2[c] = T["log_obs2"].data_ptr() + (c * rows * rs + env0) * 4
    ring = None
    if o["ring"] != "none":
        ring = ffi.EpisodeRing(env_id=_at(T["ring_env_id"]), length=_at(T["ring_length"]), ret=_at(T["ring_ret"]),
                               cursor=_at(T["ring_cursor"]), capacity=S.ring_capacity(case))
    stats = _at(T["stats"], 4 * stats_row) if o["stats"] else None
    tail = (_at(T["A"], env0 * S.N_SAMPLES * S.HORIZON), _at(T["best_idx"], env0), ctypes.c_float(o["noise"]), S.NOISE_SEED, S.PROBLEM_ID0 + env0,
            ctypes.byref(st), ctypes.byref(log) if log else None, ctypes.byref(ring) if ring else None, stats, S.ENV_SEED,
            int(d["env_id0"]) + env0, _at(T["d_t"]), _at(T["d_k"]), _at(T["ticket"]), _at(T["plan_state"], env0 * dim), ffi.stream())
    lib = ffi.lib()
    if form == "mpc":
        ffi.check(lib.ssc_mpc_rollout_step(ctypes.byref(p), ctypes.byref(pr), ctypes.byref(nav), *tail))
        return
    low, high = S.BOUNDS[case.env]
    ss = ffi.SmartStartStep(mode=_at(T["mode"], env0), plan_of=_at(T["plan_of"], env0), d_actor_out=_at(T["actor_out"], env0),
                            d_eta=_at(T["eta"]), d_ou_epsilon=_at(T["eps"]), d_pool=_at(T["pool"]),
                            ou=ffi.OuDesc(mu=S.OU["mu"], sigma=S.OU["sigma"], theta=S.OU["theta"], dt=S.OU["dt"], epsilon=0.0, d_epsilon=None),
                            act_low=low, act_high=high, d_mode_log=_at(T["mode_log"], env0) if o["mode_log"] else None,
                            mode_log_stride=0 if packed else ms, d_n_live=_at(T["n_live"]) if o["n_live"] else None)
    if form == "ss":
        ffi.check(lib.ssc_smartstart_rollout_step(ctypes.byref(p), ctypes.byref(pr), ctypes.byref(nav), ctypes.byref(ss), *tail))
        return
    ss.d_eta = ss.d_ou_epsilon = ss.d_pool = None                    # the population form reads its pair table instead
    h_pairs, d_pairs = pair_table
    ffi.check(lib.ssc_smartstart_rollout_step_many(ctypes.byref(p), ctypes.byref(pr), ctypes.byref(nav), ctypes.byref(ss), h_pairs,
                                                   _at(d_pairs), len(h_pairs), *tail))


def _pair_table(ffi, case):
    pairs = S.pairs_of(case)
    h = (ffi.SmartStartPair * len(pairs))()
    for y, q in enumerate(pairs):
        h[y] = ffi.SmartStartPair(env0=q["env0"], n_envs=q["n_envs"], slot0=q["slot0"], pool_first=q["first"], pool_count=q["count"],
                                  pool_slots=q["slots"], eta=q["eta"], ou_epsilon=q["eps"],
                                  ou=ffi.OuDesc(mu=S.OU["mu"], sigma=S.OU["sigma"], theta=S.OU["theta"], dt=S.OU["dt"], epsilon=0.0,
                                                d_epsilon=None))
    return h, torch.as_tensor(np.frombuffer(bytes(h), np.uint8).copy(), device="cuda")


def _run(ffi, case, launches=S.LAUNCHES, form=None, opts=None, dev0=None, check=True, report=None):
    """``launches`` launches in a row on one stream, inputs refreshed from the schedule in between; the read-backs"""
    dev = dev0 if dev0 is not None else S.initial_device_state(case)
    T = _upload(dev)
    table = _pair_table(ffi, case) if (form or case.form) == "many" else None
    outs = []
    for j in range(launches):
        if j:
            S.apply_inputs(case, j, dev)
            for k in S.PER_ENV_REFRESH:
                T[k].copy_(_up(dev[k]))
        before = dev
        obs_before = _observe(ffi, case, opts or case.opts, T, dev)
        _launch(ffi, case, T, form=form, opts=opts, pair_table=table)
        dev = _readback(T, before)
        got = dict(dev, before=before, obs_before=obs_before, obs_after=_observe(ffi, case, opts or case.opts, T, dev))
        if check:
            S.check_step(case, got, S.expected_step(case, j), report)
        outs.append(got)
    return outs


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_every_launch_against_the_oracle(ffi, case):
    print(S.census_line(case))
    report = {}
    try:
        _run(ffi, case, report=report)
    finally:
        print("STEPFRAC %s %s" % (case.name, " ".join("%s=%.3f" % kv for kv in sorted(report.items()))))


def _ring(got, sel=None):
    """the written ring entries as a sorted list of (env id, length, bits of the return)"""
    n = int(got["ring_cursor"][0])
    sel = np.arange(len(got["ring_env_id"])) < n if sel is None else sel
    return sorted(zip(got["ring_env_id"][sel].tolist(), got["ring_length"][sel].tolist(), got["ring_ret"][sel].view(np.int32).tolist()))


_STATE = ("s0", "s1", "steps", "ep_ret", "ou_x", "cur_idx", "actions_done", "at_goal", "plan_state", "plan_of")
_LOG = ("log_obs", "log_obs2", "log_act", "log_rew", "log_done")


@pytest.mark.parametrize("env", S.ENVS)
def test_smartstart_step_with_every_env_navigating_is_the_mpc_step(ffi, env):
    """mode = 1 everywhere and eta = 0: the log, the state, the navigator state and the statistics of ``mpc``, bit for bit"""
    case = S.CASE_BY_NAME["%s_mpc_n257" % env]
    d = S.case_data(case)
    for j in range(S.LAUNCHES):                                      # premise: no finishing env draws the coin 0.0 <= eta = 0
        e = S.expected_step(case, j)
        ids = np.uint64(d["env_id0"]) + np.nonzero(e["done"])[0].astype(np.uint64)
        assert (S.O.u01(S.O.rng_words(S.ENV_SEED, ids, np.uint64(e["t"]), S.O.TAG_SS_EPISODE)[0]) > 0).all()
    a = _run(ffi, case, check=False)
    dev0 = S.initial_device_state(case)
    dev0["eta"][0] = 0.0
    assert (dev0["mode"][d["live"]] == 1).all()
    b = _run(ffi, case, form="ss", dev0=dev0, check=False)
    for j in range(S.LAUNCHES):
        for k in _STATE + _LOG + ("stats", "ring_cursor", "d_t", "d_k", "ticket"):
            assert np.array_equal(a[j][k].view(np.uint8), b[j][k].view(np.uint8)), (j, k)
        assert _ring(a[j]) == _ring(b[j]), j                         # (the ring fills in any order)
        took_over = a[j]["at_goal"][d["live"]] == 1
        done = S.expected_step(case, j)["done"][d["live"]]
        assert np.array_equal(b[j]["mode"][d["live"]] == 0, took_over | done), j


@pytest.mark.parametrize("env", S.ENVS)
def test_every_pair_of_the_population_is_its_own_single_launch(ffi, env):
    case = S.CASE_BY_NAME["%s_many_a" % env]
    d = S.case_data(case)
    whole = _run(ffi, case, launches=1, check=False)[0]
    rs = S.strides(case)[0]
    for y, q in enumerate(d["pairs"]):
        dev = S.initial_device_state(case)
        dev["eta"][0], dev["eps"][0], dev["pool"][:] = q["eta"], q["eps"], (q["first"], q["count"], q["slots"])
        dev["plan_of"][d["live"]] -= q["slot0"]                      # the single launch counts plan slots from its window
        T = _upload(dev)
        _launch(ffi, case, T, form="ss", env0=q["env0"], n=q["n_envs"], slot0=q["slot0"], stats_row=y)
        one = _readback(T, dev)
        sl = slice(q["env0"], q["env0"] + q["n_envs"])
        one["plan_of"][d["live"]] += q["slot0"]
        for k in _STATE + ("mode",):
            assert np.array_equal(one[k][sl].view(np.uint8), whole[k][sl].view(np.uint8)), (y, k)
        for k in _LOG + ("mode_log",):
            assert np.array_equal(one[k][..., sl].view(np.uint8), whole[k][..., sl].view(np.uint8)), (y, k)
        assert np.array_equal(one["stats"][y].view(np.uint8), whole["stats"][y].view(np.uint8)), y
        mine = (whole["ring_env_id"] >= d["env_id0"] + q["env0"]) & (whole["ring_env_id"] < d["env_id0"] + q["env0"] + q["n_envs"])
        nw = int(one["ring_cursor"][0])
        assert nw == int(mine.sum())
        assert _ring(one) == _ring(whole, mine), y
        assert int(one["d_t"][0]) == int(whole["d_t"][0]) and int(one["ticket"][0]) == 0
    assert rs == case.n


@pytest.mark.parametrize("name", ["mc_ss_n255", "pend_ss_n255", "mc_mpc_n255", "pend_many_c"])
def test_a_strided_log_and_no_log_leave_the_same_state(ffi, name):
    case = S.CASE_BY_NAME[name]
    assert case.opts["log"] == "strided"
    a = _run(ffi, case, check=False)
    b = _run(ffi, case, opts=dict(case.opts, log="none"), check=False)
    for j in range(S.LAUNCHES):
        for k in _STATE + ("mode", "mode_log", "stats", "ring_cursor", "d_t", "d_k", "ticket"):
            assert np.array_equal(a[j][k].view(np.uint8), b[j][k].view(np.uint8)), (j, k)
        for k in _LOG:
            assert np.array_equal(b[j][k].view(np.uint8), b[j]["before"][k].view(np.uint8)), (j, k)
