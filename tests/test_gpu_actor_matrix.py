"""Every bf16 MFMA actor kernel and every rollout policy dispatch_policy() can launch, against the fp64 oracle under the
bound that follows the bf16 arithmetic (tests/actor_cases.py): e = max |emulation - fp64| at the case's own inputs, accepted:
|X - emu| <= C_ACT e and |X - ref| <= (1 + C_ACT) e with C_ACT = 1 and the emulation O.actor_forward_bf16emu(fold=True).
tests/test_actor_cases_cpu.py shows on the CPU that this bound rejects every listed way an actor kernel goes wrong at every
case below, and that the two lists cover exactly what the dispatchers can reach.

Standalone: ssc_actor_forward and ssc_actor_forward_rms, 27 cases x last_layer_tanh x m in (1, 33, 64, 65, 321).  A launch
of fewer rows is held to the case's e on its rows AND is bit for bit the first rows of the 321-row launch.

Fused rollout: one teacher-forced run (O.replay_rollout) per policy instantiation and per branch inside one, n = 321 envs,
11 steps from t = 3 with the time-limit reset inside the window; n = 1 and n = 33 are bit for bit the first envs of that
run.  The logged action is scale(scale(clip(net + eps * ou_x))): the bound is asserted on the steps where the kernel's
action and both oracle actions are strictly inside the action bounds, with e taken on that very quantity (the oracle's
logged actions, so Pendulum's scale(scale(.)) is inside e), and at least half of all steps must be such steps.  The
oracle's OU state is fp64 and the kernel's fp32: runs whose action carries noise get the project's fp32 action tolerance
(2e-5 (high - low) / 2, what the fp32 policies meet on the same replay) on top of the bound; noise-free runs the bare bound.

Measured on an MI355X, max |X - emu| / e (per case: NOTEBOOK section 20): standalone 0.000-0.001 at most cases, largest 0.240
(o2_224-128 on wide statistics); ActorPolicy<ActorMfma / ActorMfmaLds> at most 0.238; ActorPolicyFused 0.14-0.57 (largest:
64-32 without last_layer_tanh) -- ActorMfma2's layer 1 is a three-term bf16 split, not the exact fp32 MFMA the emulation
assumes.  Every step of every run was inside the action bounds.  C_ACT = 1 holds with no kernel or emulation change.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import actor_cases as AC
from tests.gpu_util import rms_edge_stats, x_hat64

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED, ID0 = AC.SEED, AC.ID0


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


@functools.lru_cache(maxsize=None)
def prepared(name):
    return AC.build_inputs(AC.case_by_name(name))


def _forward_gpu(ssc, dw, obs, llt, obs_clip, rms=None):
    """ssc_actor_forward / ssc_actor_forward_rms on the bf16 MFMA path; dw: the weights on the device"""
    ffi = ssc._ffi
    a = ffi.ActorDesc()
    a.obs_dim, a.h1 = dw["W1"].shape
    a.h2, a.act_dim = dw["W2"].shape[1], 1
    ffi.set_net_ptrs(a, dw)
    a.last_layer_tanh, a.precision, a.obs_clip = int(llt), ffi.SSC_PREC_BF16_MFMA, float(obs_clip or 0.0)
    o = torch.as_tensor(obs, dtype=torch.float32, device="cuda").contiguous()
    out = torch.full((o.shape[0], 1), float("nan"), dtype=torch.float32, device="cuda")
    if rms is None:
        ffi.check(ffi.lib().ssc_actor_forward(ctypes.byref(a), o.shape[0], ffi.ptr(o), ffi.ptr(out), None))
    else:
        ffi.check(ffi.lib().ssc_actor_forward_rms(ctypes.byref(a), o.shape[0], ffi.ptr(o), ffi.ptr(out), None, ffi.ptr(rms.block)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_standalone(ssc, what, w, x_dev, ref, emu, llt, obs_clip, rms=None):
    dw = {k: torch.as_tensor(v, device="cuda").contiguous() for k, v in w.items()}
    e = AC.bf16_error(ref, emu)
    full = _forward_gpu(ssc, dw, x_dev, llt, obs_clip, rms)
    for m in AC.STANDALONE_M:
        out = full if m == AC.ROWS else _forward_gpu(ssc, dw, x_dev[:m], llt, obs_clip, rms)
        assert out.shape == (m, 1)
        r = AC.bound_ratios(out, ref, emu, e, slice(0, m))
        print("ACTRATIO", *what, f"m={m} e={e:.3e} emu={r[0]:.3f} ref={r[1] / (1 + AC.C_ACT):.3f}", flush=True)
        assert AC.within_bound(r), (what, m, r, e)
        assert np.array_equal(out, full[:m]), (what, m)


@pytest.mark.parametrize("llt", [True, False])
@pytest.mark.parametrize("name", AC.CASE_IDS)
def test_actor_forward_vs_oracle(ssc, name, llt):
    inp = prepared(name)
    ref, emu = AC.references(inp, llt)
    _assert_standalone(ssc, (name, f"llt={int(llt)}", inp.case.kernel), inp.w, inp.obs, ref, emu, llt, inp.obs_clip)


@pytest.mark.parametrize("kind", ["wide", "floor"])
@pytest.mark.parametrize("llt", [True, False])
@pytest.mark.parametrize("name", AC.CASE_IDS)
def test_actor_forward_rms_vs_oracle(ssc, name, llt, kind):
    """The normalising kernels on RAW observations and the statistics block; the oracle is fed x_hat in fp64, e is taken on
    the normalised inputs.  "floor": every std on the 0.1 floor, some components on +clip and on -clip, at least half the
    rows clear; "wide": nothing clipped."""
    inp = prepared(name)
    rms, (lo, hi) = rms_edge_stats(inp.case.obs_dim, kind)
    rng = np.random.default_rng(AC.ROWS + inp.case.h1)
    raw = rng.uniform(lo, hi, size=(AC.ROWS, inp.case.obs_dim)).astype(np.float32)
    xh = x_hat64(raw, rms, AC.OBS_CLIP)
    if kind == "floor":
        assert (xh == AC.OBS_CLIP).any() and (xh == -AC.OBS_CLIP).any()
        assert np.mean((np.abs(xh) < AC.OBS_CLIP).all(axis=1)) >= 0.5
    else:
        assert np.abs(xh).max() < AC.OBS_CLIP
    ref, emu = AC.forward_ref(xh, inp.w, llt, AC.OBS_CLIP), AC.forward_emu(xh, inp.w, llt, AC.OBS_CLIP)
    _assert_standalone(ssc, (name, f"llt={int(llt)}", "rms_" + kind), inp.w, raw, ref, emu, llt, AC.OBS_CLIP, rms)


# ------------------------------------------------------------------------------------------------------- fused rollout --
class Recorded:
    """action_fn for O.replay_rollout that keeps what the inner policy returned at every step; ``pre``: what it sees"""

    def __init__(self, inner, pre=None):
        self.inner, self.pre, self.actions = inner, pre, []

    def __call__(self, k, t, obs, prev_done):
        a = self.inner(k, t, obs if self.pre is None else self.pre(obs), prev_done)
        self.actions.append(np.asarray(a, np.float64).copy())
        return a


def _log(chunk):
    return dict(obs=chunk.obs.cpu().numpy(), act=chunk.act.cpu().numpy(), rew=chunk.rew.cpu().numpy(),
                done=chunk.done.cpu().numpy(), obs2=chunk.obs2.cpu().numpy())


def _state(env):
    return {k: getattr(env, k).cpu().numpy().copy() for k in ("s0", "s1", "steps", "ep_ret", "ou_x", "stats")}


def _make_chunk(ssc, form, obs_dim, K, n):
    """packed: the default chunk (LOG, ONEBASE).  "columns": TransitionChunk.from_columns over ONE backing tensor with the act
    column BELOW obs[0] in memory, so the columns cannot be addressed from obs[0] (LOG without ONEBASE)."""
    if form == "packed":
        return None
    back = torch.full((2 * obs_dim + 2, K, n), float("nan"), dtype=torch.float32, device="cuda")
    act, obs, rew, obs2 = back[0], back[1:1 + obs_dim], back[1 + obs_dim], back[2 + obs_dim:]
    assert act.data_ptr() < obs[0].data_ptr()
    done = torch.empty((K, n), dtype=torch.uint8, device="cuda")
    from smartstartcontinuous_amd.vec_env import TransitionChunk
    return TransitionChunk.from_columns(obs, act, rew, obs2, done)


def _launch(ssc, run, n, form="packed"):
    """One rollout of the run on the device: (log or None, state after, obs0, rms)"""
    env_id, obs_dim, tmax, low, high = AC.ENV_OF[run.env]
    K = AC.ROLLOUT_K
    env = ssc.VecEnv(env_id, n, seed=SEED, env_id0=ID0)
    env.reset()
    s0, s1 = AC.initial_state(run, n)
    env.s0.copy_(torch.as_tensor(s0))
    env.s1.copy_(torch.as_tensor(s1))
    obs0 = env.observe().cpu().numpy().copy()
    env.steps.fill_(tmax - AC.ROLLOUT_STEPS_LEFT)         # the time-limit reset (and the OU reset) inside the window
    env.t = AC.ROLLOUT_T0
    rms = None
    if run.norm:
        from smartstartcontinuous_amd.obs_rms import ObsRms
        rms = ObsRms(obs_dim)
        rms.update_rows(AC.rollout_stat_rows(run))
    if run.precision == "random":
        pol = ssc.RandomPolicy()
    else:
        w = {k: torch.as_tensor(v) for k, v in AC.rollout_weights(run).items()}
        d_eps = torch.tensor([AC.DEV_EPS[run.eps]], dtype=torch.float32, device="cuda") if run.eps in AC.DEV_EPS else None
        pol = ssc.ActorPolicy(w, last_layer_tanh=run.llt, precision=run.precision, ou_epsilon=1.0 if run.eps == "host" else 0.0,
                              obs_clip=run.obs_clip, d_ou_epsilon=d_eps, d_obs_rms=rms.block if rms is not None else None)
    if form == "nolog":
        assert env.rollout(K, pol, log=False) is None
        log = None
    else:
        chunk = env.rollout(K, pol, out=_make_chunk(ssc, form, obs_dim, K, n))
        log = _log(chunk)
    torch.cuda.synchronize()
    return log, _state(env), obs0, (rms.mean_std() if rms is not None else None)


def _oracle_policy(run, n, mean_std, model, oracle_weights=None):
    """model: False = fp64, "fold" = the emulation of the MFMA kernels.  oracle_weights: the weights the ORACLE sees instead
    of the run's (a mutant, applied by hand to see the test fail)."""
    _, obs_dim, _, low, high = AC.ENV_OF[run.env]
    if run.precision == "random":
        return Recorded(O.OracleRandomPolicy(SEED, ID0, n, low, high))
    w = oracle_weights or AC.rollout_weights(run)
    w6 = {k: w[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")}
    clip = run.obs_clip or None
    fwd = None
    if run.ln:
        ln = ((w["ln1_g"], w["ln1_b"]), (w["ln2_g"], w["ln2_b"]))
        fwd = lambda x: O.actor_forward(x, **w6, last_layer_tanh=run.llt, layer_norm=ln, obs_clip=clip)
    eps = AC.DEV_EPS.get(run.eps, 1.0 if run.eps == "host" else 0.0)
    inner = O.OracleDDPGPolicy(w6, SEED, ID0, n, epsilon=eps, low=low, high=high, last_layer_tanh=run.llt, bf16=model,
                               obs_clip=clip, forward=fwd, device_epsilon=run.eps in AC.DEV_EPS)
    pre = None
    if mean_std is not None:
        pre = lambda obs: AC.x_hat64(obs, mean_std[0], mean_std[1], run.obs_clip)
    return Recorded(inner, pre)


def _replay(run, n, log, state, obs0, mean_std, oracle_weights=None):
    """The structural results of the replay (asserted here, as test_rollout_actor_mountaincar_teacher_forced does) and the
    per-step actions (kernel, emulation, fp64)."""
    _, obs_dim, tmax, low, high = AC.ENV_OF[run.env]
    kind, steps0 = run.env, np.full(n, tmax - AC.ROLLOUT_STEPS_LEFT)
    out = {}
    for model in (False, "fold"):
        pol = _oracle_policy(run, n, mean_std, model, oracle_weights)
        res = O.replay_rollout(kind, log, SEED, ID0, AC.ROLLOUT_T0, tmax, obs0, steps0, pol)
        out[model] = (np.stack(pol.actions), res, pol.inner)
        if run.precision != "bf16_mfma":
            break
    A_ref, res, inner = out[False]
    assert res["start_max_err"] == 0 and res["continuity_mismatch"] == 0 and res["done_mismatch"] == 0, res
    if kind == "mc":
        assert res["max_dobs2"][0] <= 2.4e-7 and res["max_dobs2"][1] <= 1e-8, res
        assert res["max_drew_rel"] <= 1e-6 and res["reset_max_err"] == 0, res
    else:
        assert (res["max_dobs2"] <= [3e-6, 3e-6, 3e-6]).all(), res
        assert res["max_drew_rel"] <= 2e-5 and res["reset_max_err"] <= 2e-6, res
    done = log["done"].astype(bool)
    assert done[AC.ROLLOUT_STEPS_LEFT - 1].all() and done.sum() == n                  # the time limit, once per env
    if run.precision != "random":
        assert np.max(np.abs(state["ou_x"] - inner.x)) < 2e-5                         # the OU state written back
        if run.eps != "none":
            assert np.abs(state["ou_x"]).min() > 0                                    # ... which ran, also under epsilon <= 0
        else:
            assert not state["ou_x"].any()
    assert state["stats"][2] == n * AC.ROLLOUT_K and state["stats"][3] == n
    A = log["act"].astype(np.float64)
    return A, (out["fold"][0] if "fold" in out else None), A_ref, res


@functools.lru_cache(maxsize=None)
def _full_run(name):
    """the n = 321 run of a rollout case: launched and replayed once, shared by the tests that compare against it"""
    import smartstartcontinuous_amd as pkg
    run, n = AC.run_by_name(name), max(AC.ROLLOUT_N)
    log, state, obs0, mean_std = _launch(pkg, run, n)
    return log, state, obs0, mean_std


@functools.lru_cache(maxsize=None)
def _full_e(name):
    """e of the n = 321 run, on its compared steps (None for the fp32 and random policies)"""
    run, n = AC.run_by_name(name), max(AC.ROLLOUT_N)
    if run.precision != "bf16_mfma":
        return None
    A, A_emu, A_ref, _ = _replay(run, n, *_full_run(name))
    lim = AC.action_limit(run)
    inside = (np.abs(A) < lim) & (np.abs(A_emu) < lim) & (np.abs(A_ref) < lim)
    return AC.bf16_error(A_ref[inside], A_emu[inside])


def _assert_actions(run, n, what, A, A_emu, A_ref, res, e=None):
    """the bound (bf16), the fp32 action tolerance (f32) or equality (random) on the logged actions.  ``e``: the full run's,
    for a launch of fewer envs (a handful of steps of one env say nothing about what the arithmetic costs)."""
    _, _, _, low, high = AC.ENV_OF[run.env]
    scale = (high - low) / 2
    if run.precision == "random":
        assert res["max_dact"] == 0, res
        return None
    if run.precision == "f32":
        assert res["max_dact"] <= AC.TOL_ACT_F32 * scale, res
        return None
    lim = AC.action_limit(run)
    oracle_inside = (np.abs(A_emu) < lim) & (np.abs(A_ref) < lim)
    inside = oracle_inside & (np.abs(A) < lim)
    assert oracle_inside.mean() >= 0.5 and inside.mean() >= 0.5, (what, oracle_inside.mean(), inside.mean())
    e = AC.bf16_error(A_ref[inside], A_emu[inside]) if e is None else e
    r = AC.bound_ratios(A, A_ref, A_emu, e, inside)
    noisy = (run.eps == "host") or AC.DEV_EPS.get(run.eps, 0.0) > 0
    extra = AC.TOL_ACT_F32 * scale / e if noisy else 0.0
    print("ACTRATIO", *what, f"n={n} inside={inside.mean():.2f} e={e:.3e} emu={r[0]:.3f} ref={r[1] / (1 + AC.C_ACT):.3f} "
          f"fp32_allowance={extra:.3f}e", flush=True)
    assert AC.within_bound(r, extra=extra), (what, r, e, extra)
    return e


@pytest.mark.parametrize("name", AC.ROLLOUT_IDS)
def test_rollout_policy_vs_oracle(ssc, name):
    run, n = AC.run_by_name(name), max(AC.ROLLOUT_N)
    log, state, obs0, mean_std = _full_run(name)
    A, A_emu, A_ref, res = _replay(run, n, log, state, obs0, mean_std)
    _assert_actions(run, n, (name, run.inst), A, A_emu, A_ref, res)
    assert run.precision != "bf16_mfma" or _full_e(name) > 0


@pytest.mark.parametrize("n", [k for k in AC.ROLLOUT_N if k != max(AC.ROLLOUT_N)])
@pytest.mark.parametrize("name", AC.ROLLOUT_IDS)
def test_rollout_policy_small_launches(ssc, name, n):
    """n = 1 (one lane of one wave) and n = 33 (one env in the wave's second tile): replayed like the full run, held to the
    full run's e, and bit for bit its first n envs (an env depends on nothing but its own id, state and step index)."""
    run = AC.run_by_name(name)
    full_log, full_state, full_obs0, mean_std = _full_run(name)
    log, state, obs0, _ = _launch(ssc, run, n)
    A, A_emu, A_ref, res = _replay(run, n, log, state, obs0, mean_std)
    for k, v in log.items():
        assert np.array_equal(v, full_log[k][..., :n]), (name, n, k)
    for k in ("s0", "s1", "steps", "ep_ret", "ou_x"):
        assert np.array_equal(state[k], full_state[k][:n]), (name, n, k)
    _assert_actions(run, n, (name, run.inst), A, A_emu, A_ref, res, e=_full_e(name))


@pytest.mark.parametrize("n", [33, 321])
@pytest.mark.parametrize("name", ["fused_64-32", "fused_48-24_norm_floor", "lds_mc", "lds_pend_norm"])
def test_rollout_launch_forms_agree(ssc, name, n):
    """The three forms launch_rollout() has for one policy -- a packed chunk (LOG, ONEBASE), columns that cannot be addressed
    from obs[0] (LOG without ONEBASE: set_one_base yields 0) and no log at all -- leave the same state and statistics bit
    for bit, and the two logged forms the same columns."""
    run = AC.run_by_name(name)
    packed, st_p, _, _ = _launch(ssc, run, n, "packed")
    cols, st_c, _, _ = _launch(ssc, run, n, "columns")
    nolog, st_n, _, _ = _launch(ssc, run, n, "nolog")
    assert nolog is None
    for k in ("obs", "act", "rew", "done", "obs2"):
        assert np.isfinite(cols[k]).all() and np.array_equal(packed[k], cols[k]), (name, n, k)
    for other in (st_c, st_n):
        for k in ("s0", "s1", "steps", "ep_ret", "ou_x"):
            assert np.array_equal(st_p[k], other[k]), (name, n, k)
        assert np.array_equal(st_p["stats"][1:], other["stats"][1:]), (name, n)
    assert st_p["ou_x"].any() and st_p["stats"][2] == n * AC.ROLLOUT_K
