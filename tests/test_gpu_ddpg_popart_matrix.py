"""Every kernel a Pop-Art train_on call launches -- ddpg_wide_grad_kernel<PopTarget> / <PopGrad> and their <const double *, ...>
builds (pop_target_rows, pop_grad_rows), ddpg_popart_renorm_kernel (popart_renorm_body) and ddpg_wide_apply_kernel<false | true>
/ ddpg_wide_prepare_kernel on the gradient pass's partials (tests/popart_grad_cases.py: CASES, each with the kernels it
claims) -- held to the fp64 restatement by the derived bounds of tests/popart_grad_cases.py.

ONE iteration is launched alone on a fresh agent whose return block is set from the case, so the device gradient of every
actor and critic parameter can be read back from m = c1 g: |g - g64| <= C_GRAD * 2^-24 * A for every element, v, the parameters
inside the interval the fp64 Adam step maps that to -- for the critic from the fp64-rescaled W3' / b3', widened by their E --
both targets as the soft update of the new parameters (the target critic from its rescaled output layer), both losses, every y
and the block's sums within what E(y) allows, count exactly, the partials as the f64 butterfly sums of the device's own y, the
four scalars within C_STAT 2^-24 E and exactly float32(0.1) on the floor, adam_t == [1, 1], the inputs untouched, and a second
execution from the same start with the same bits.  Every constant is fixed on the CPU from a float32 emulation
(tests/test_popart_grad_cases_cpu.py); the six-iteration checks of tests/test_gpu_ddpg_popart.py stay beside this.

Measured on an MI355X (largest err / allowed over the 18 cases; the per-case table is NOTEBOOK section 23): gradient 0.172 (pa_l2,
critic W2; 0.001 .. 0.029 at the large-block cases), v 0.138, targets 0.544, losses 0.053, y 0.250, sum / sumsq 0.038, scalars 0.178
(one unit in the last place at pa_mixed_a128_c200, equal elsewhere); every parameter inside its interval, the partials bit for bit.

Populations have no rows here: tests/test_gpu_ddpg_many_popart.py holds the Pop-Art agents of a population bit for bit to the
single-agent calls this matrix checks."""
import numpy as np
import pytest

from tests import ddpg_cases as D
from tests import popart_grad_cases as P

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
    """a fresh Pop-Art agent on the case's networks and return block, one iteration on the case's batch: dict of host arrays"""
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    from smartstartcontinuous_amd.obs_rms import ObsRms
    from tests.test_gpu_agents import _BoxEnv
    d = P.case_data(case)
    env = ssc.make("MountainCarContinuous-v0") if case.obs == 2 else _BoxEnv(case.obs)
    agent = DDPG_Baselines_agent(env, None, actor_h1=case.ah[0], actor_h2=case.ah[1], critic_h1=case.ch[0], critic_h2=case.ch[1],
                                 lastLayerTanh=case.llt, actor_lr=D.LR, critic_lr=D.LR, gamma=D.GAMMA, tau=case.tau, batch_size=case.B,
                                 seed=5, training=False, layer_norm=case.ln, critic_l2_reg=case.l2, clip_norm=d["clip_norm"],
                                 normalize_returns=True, enable_popart=True)
    agent.set_weights({k: np.array(v) for k, v in d["actor"].items()})
    agent.set_critic_weights({k: np.array(v) for k, v in d["critic"].items()})
    agent.target_actor_flat.copy_(torch.from_numpy(D.flat(d["target_actor"])))
    agent.target_critic_flat.copy_(torch.from_numpy(D.flat(d["target_critic"])))
    assert agent.actor_flat.cpu().numpy().tobytes() == D.flat(d["actor"]).tobytes()
    assert agent.critic_flat.cpu().numpy().tobytes() == D.flat(d["critic"]).tobytes()
    agent.ret_rms.block.copy_(torch.from_numpy(np.array(d["ret_block"])))
    assert agent.ret_rms.block.cpu().numpy().tobytes() == d["ret_block"].tobytes()
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
    ws = agent.popart_workspace()
    out = dict(loss=host(losses)[0], adam_t=agent._adam_t.cpu().tolist(), y=host(ws["y"]), partials=host(ws["partials"]),
               scalars=host(ws["scalars"]), block=host(agent.ret_rms.block))
    for net, theta, target, mv, like in (("actor", agent.actor_flat, agent.target_actor_flat, agent._adam_actor, d["actor"]),
                                         ("critic", agent.critic_flat, agent.target_critic_flat, agent._adam_critic, d["critic"])):
        out[net] = dict(theta=D.unflat(host(theta), like), target=D.unflat(host(target), like), m=D.unflat(host(mv[0]), like),
                        v=D.unflat(host(mv[1]), like))
    # the inputs are untouched
    for t, k in zip(rows + (idx,), ("s", "a", "r", "t", "s2", "idx")):
        assert host(t).tobytes() == d[k].tobytes(), k
    if case.stats:
        assert host(kw["obs_rms"].block).tobytes() == d["block"].tobytes()
    return out


_RUNS = {}


def _run(ssc, monkeypatch, case, again=False):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)
    if again:
        return _execute(ssc, case)
    if case.name not in _RUNS:
        _RUNS[case.name] = _execute(ssc, case)
    return _RUNS[case.name]


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_one_popart_iteration_within_the_float32_bounds(ssc, monkeypatch, case):
    d, ref, run = P.case_data(case), P.reference(case), _run(ssc, monkeypatch, case)
    ch = P.checks(d, ref, run)
    # the partials: the f64 sums of the device's own float32 y per 16-row workgroup, in the butterfly's order
    want = P.partial_sums(run["y"])
    assert run["partials"].shape == want.shape == ((case.B + 15) // 16, 2)
    part = float(np.max(np.abs(run["partials"] - want) / np.maximum(np.abs(want), 1e-300)))
    print("POPART_MATRIX %-22s %-6s err / allowed: m %.3f (%s) v %.3f theta %.3f target %.3f (%s) loss %.3f %.3f y %.3f sum %.3f sumsq %.3f "
          "scalars %.3f partials %.1e   %s" % (case.name, case.block, ch["m"], ch["where"].get("m", "-"), ch["v"], ch["theta"], ch["target"],
                                               ch["where"].get("target", "-"), ch["loss_c"], ch["loss_a"], ch["y"], ch["sum"], ch["sumsq"],
                                               ch["stat"], part, " + ".join(case.kernels)))
    assert run["adam_t"] == [1, 1]
    assert ch["y"] <= 1.0, ch["y"]                                              # every y of the target pass
    assert part <= 1e-15, part
    assert ch["count"] == 0.0 and ch["sum"] <= 1.0 and ch["sumsq"] <= 1.0, (run["block"], ref["block"])
    assert ch["stat"] <= 1.0, (run["scalars"], ref["scalars"], ref["E_scalars"])
    for j, state in ((1, ref["floor_state"][0]), (3, ref["floor_state"][1])):
        if state == "floor":
            assert run["scalars"][j] == P.FLOOR32
    assert ch["m"] <= 1.0 and ch["v"] <= 1.0, (ch["where"], ch["m"], ch["v"])   # the gradient, read back from m, and v
    assert ch["theta"] <= 1.0, (ch["where"], ch["theta"])                       # the parameters: rescaled, then stepped
    assert ch["target"] <= 1.0, (ch["where"], ch["target"])                     # the targets: rescaled, then the soft update
    assert ch["loss_c"] <= 1.0 and ch["loss_a"] <= 1.0, (run["loss"], ref["loss"])


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_same_start_same_bits(ssc, monkeypatch, case):
    first, again = _run(ssc, monkeypatch, case), _run(ssc, monkeypatch, case, again=True)
    assert again["adam_t"] == first["adam_t"]
    for k in ("loss", "y", "partials", "scalars", "block"):
        assert again[k].tobytes() == first[k].tobytes(), k
    for net in ("actor", "critic"):
        for part in ("theta", "target", "m", "v"):
            for k, v in first[net][part].items():
                assert again[net][part][k].tobytes() == v.tobytes(), (net, part, k)
