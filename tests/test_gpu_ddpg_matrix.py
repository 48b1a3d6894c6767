"""Every learner kernel a DDPG_Baselines_agent.train_on call can launch -- the sixteen ddpg_train_fixed_kernel<O, TANH2,
TILED, Rms...> instantiations, the step interpreter ddpg_train_kernel, ddpg_wide_grad_kernel<> / <const double *> with
ddpg_wide_apply_kernel<false | true> and ddpg_wide_prepare_kernel (tests/ddpg_cases.py: CASES, each with the kernels it
claims) -- held to the fp64 oracle by the derived bound of tests/ddpg_cases.py.

ONE iteration is launched alone on a fresh agent (zero Adam moments and counters), so the device gradient of every actor
and critic parameter can be read back from m = c1 g (Adam's scale invariance hides its size from the parameters):
|g - g64| <= C_GRAD * 2^-24 * A for every element, v against c2 g64^2 with the bound that follows, the parameters inside
the interval the fp64 Adam step maps the gradient bound to, the targets as the soft update of the NEW parameters (at
tau = 0.001 and 0.3), both losses, adam_t == [1, 1], and a second execution from the same start with the same bits.
Both constants are fixed on the CPU from a float32 emulation (tests/test_ddpg_cases_cpu.py); the six-iteration checks of
tests/test_gpu_agents.py (moments rtol 1e-3, about 10^4 roundings) stay beside this.

Measured on an MI355X (largest err / allowed over the 54 cases; the per-case table is NOTEBOOK section 21): gradient 0.156
(op_l2, critic W2; 0.010 .. 0.075 at the LayerNorm cases), v 0.150, targets 0.54, losses 0.090; every parameter inside its interval.

Populations have no rows here: tests/test_gpu_ddpg_many.py and tests/test_gpu_ddpg_many_wide.py hold them bit for bit
(torch.equal) to the single-agent calls this matrix checks, mixed shapes included."""
import ctypes

import numpy as np
import pytest

from tests import ddpg_cases as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _execute(ssc, case):
    """a fresh agent on the case's networks, one iteration on the case's batch: dict of host arrays"""
    from smartstartcontinuous_amd import _ffi
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.obs_rms import ObsRms
    from tests.test_gpu_agents import _BoxEnv
    d = D.case_data(case)
    env = ssc.make("MountainCarContinuous-v0") if case.obs == 2 else _BoxEnv(case.obs)
    agent = DDPG_Baselines_agent(env, None, actor_h1=case.ah[0], actor_h2=case.ah[1], critic_h1=case.ch[0], critic_h2=case.ch[1],
                                 lastLayerTanh=case.llt, actor_lr=D.LR, critic_lr=D.LR, gamma=D.GAMMA, tau=case.tau, batch_size=case.B,
                                 seed=5, training=False, layer_norm=case.ln, critic_l2_reg=case.l2, clip_norm=d["clip_norm"])
    agent.set_weights({k: np.array(v) for k, v in d["actor"].items()})
    agent.set_critic_weights({k: np.array(v) for k, v in d["critic"].items()})
    agent.target_actor_flat.copy_(torch.from_numpy(D.flat(d["target_actor"])))
    agent.target_critic_flat.copy_(torch.from_numpy(D.flat(d["target_critic"])))
    assert agent.actor_flat.cpu().numpy().tobytes() == D.flat(d["actor"]).tobytes()
    assert agent.critic_flat.cpu().numpy().tobytes() == D.flat(d["critic"]).tobytes()
    # the library sends this call where the table says
    assert agent.lib.ssc_ddpg_learner_path(ctypes.byref(agent.ddpg_desc()), 1, int(case.stats is not None)) == case.path
    dev = lambda x, dt: torch.as_tensor(np.array(x), dtype=dt, device="cuda").contiguous()
    rows = (dev(d["s"], torch.float32), dev(d["a"], torch.float32), dev(d["r"], torch.float32), dev(d["t"], torch.uint8),
            dev(d["s2"], torch.float32))
    idx = dev(d["idx"], torch.int32)
    kw = {}
    if case.stats:
        rms = ObsRms(case.obs)
        rms.block.copy_(torch.from_numpy(np.array(d["block"])))
        mean, std = rms.mean_std()
        assert mean.tobytes() == d["mean"].tobytes() and std.tobytes() == d["std"].tobytes()
        kw["obs_rms"] = rms
    losses = agent.train_on(*rows, idx, 1, **kw)
    torch.cuda.synchronize()
    host = lambda x: x.cpu().numpy().copy()
    out = dict(loss=host(losses)[0], adam_t=agent._adam_t.cpu().tolist())
    for net, theta, target, mv, like in (("actor", agent.actor_flat, agent.target_actor_flat, agent._adam_actor, d["actor"]),
                                         ("critic", agent.critic_flat, agent.target_critic_flat, agent._adam_critic, d["critic"])):
        out[net] = dict(theta=D.unflat(host(theta), like), target=D.unflat(host(target), like), m=D.unflat(host(mv[0]), like),
                        v=D.unflat(host(mv[1]), like))
    # the inputs are untouched
    for t, k in zip(rows, ("s", "a", "r", "t", "s2")):
        assert host(t).tobytes() == d[k].tobytes(), k
    return out


_RUNS = {}


def _run(ssc, monkeypatch, case, again=False):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)
    if case.env:
        monkeypatch.setenv(case.env, "1")
    if again:
        return _execute(ssc, case)
    if case.name not in _RUNS:
        _RUNS[case.name] = _execute(ssc, case)
    return _RUNS[case.name]


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_one_iteration_within_the_float32_gradient_bound(ssc, monkeypatch, case):
    d, ref, run = D.case_data(case), D.reference(case), _run(ssc, monkeypatch, case)
    worst, where = np.zeros(4), [""] * 4
    for net in ("actor", "critic"):
        got = run[net]
        for k, theta0 in d[net].items():
            r = D.step1_ratios(theta0, ref["g"][net][k], ref["A"][net][k], got["m"][k], got["v"][k], got["theta"][k])
            r += (D.target_ratio(d["target_" + net][k], got["theta"][k], got["target"][k], case.tau),)
            for i in range(4):
                if r[i] > worst[i]:
                    worst[i], where[i] = r[i], net + "." + k
    rl = [x / D.C_LOSS for x in D.loss_ratios(ref, run["loss"])]
    print("DDPG_MATRIX %-26s %-11s err / allowed: m %.3f (%s) v %.3f theta %.3f target %.3f loss %.3f %.3f   %s" % (
        case.name, D.PATH_NAME[case.path], worst[0], where[0], worst[1], worst[2], worst[3], rl[0], rl[1], " + ".join(case.kernels)))
    assert run["adam_t"] == [1, 1]
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (where[:2], worst[:2])          # the gradient, read back from m, and v
    assert worst[2] <= 1.0, (where[2], worst[2])                                # the parameters after the step
    assert worst[3] <= 1.0, (where[3], worst[3])                                # the targets: the soft update of the NEW parameters
    assert rl[0] <= 1.0 and rl[1] <= 1.0, (run["loss"], ref["loss"])


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_same_start_same_bits(ssc, monkeypatch, case):
    first, again = _run(ssc, monkeypatch, case), _run(ssc, monkeypatch, case, again=True)
    assert again["adam_t"] == first["adam_t"] and again["loss"].tobytes() == first["loss"].tobytes()
    for net in ("actor", "critic"):
        for part in ("theta", "target", "m", "v"):
            for k, v in first[net][part].items():
                assert again[net][part][k].tobytes() == v.tobytes(), (net, part, k)
