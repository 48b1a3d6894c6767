"""DDPG return normalisation and Pop-Art on the multi-workgroup learner (``ssc_ddpg_train_ws_popart``) against the fp64
restatement of tests/popart_cases.py, and the properties around it: preserved outputs, the identities of the two switches
on their own, reproducibility, statistics carried across calls, workspace guards and the denormalising read-outs.
The derived float32 bound on ONE iteration of every Pop-Art kernel is tests/test_gpu_ddpg_popart_matrix.py."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import popart_cases as PC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 5e-6          # parameters and targets: 6 Adam steps of ~1e-3, fp32 kernel vs fp64 restatement (_ddpg_kernel_vs_oracle)


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


class BoxEnv:
    def __init__(self, obs_dim):
        from smartstartcontinuous_amd import spaces
        self.observation_space = spaces.Box(low=-np.ones(obs_dim, np.float32), high=np.ones(obs_dim, np.float32))
        self.action_space = spaces.Box(low=np.array([-1.0], np.float32), high=np.array([1.0], np.float32))


def make_agent(case, normalize_returns=True, enable_popart=True, **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    kw = dict(dict(actor_lr=PC.LR, critic_lr=PC.LR, gamma=PC.GAMMA, tau=PC.TAU), **kw)
    h1, h2 = case["h1"], case["h2"]
    agent = DDPG_Baselines_agent(BoxEnv(case["obs_dim"]), None, actor_h1=h1, actor_h2=h2, critic_h1=h1, critic_h2=h2,
                                 lastLayerTanh=True, batch_size=case["B"], seed=5, training=False, layer_norm=case["layer_norm"],
                                 normalize_returns=normalize_returns, enable_popart=enable_popart, **kw)
    agent.set_weights(case["actor"])
    agent.set_critic_weights(case["critic"])
    agent.target_actor_flat.copy_(torch.as_tensor(O.flatten_params(case["target_actor"]).astype(np.float32)))
    agent.target_critic_flat.copy_(torch.as_tensor(O.flatten_params(case["target_critic"]).astype(np.float32)))
    return agent


def device_rows(case):
    s, a, r, t, s2 = case["rows"]
    dev = lambda x, dt: torch.as_tensor(x, dtype=dt, device="cuda").contiguous()
    return dev(s, torch.float32), dev(a, torch.float32), dev(r, torch.float32), dev(t, torch.uint8), dev(s2, torch.float32)


def train(agent, case, first=0, last=None, rows=None, **kw):
    idx = torch.as_tensor(case["idx"][first:last], dtype=torch.int32, device="cuda").contiguous()
    return agent.train_on(*(rows or device_rows(case)), idx, idx.shape[0], **kw)


def state_of(agent):
    """every array the learner writes, as host copies"""
    out = dict(actor=agent.actor_flat, critic=agent.critic_flat, target_actor=agent.target_actor_flat,
               target_critic=agent.target_critic_flat, m_actor=agent._adam_actor[0], v_actor=agent._adam_actor[1],
               m_critic=agent._adam_critic[0], v_critic=agent._adam_critic[1], adam_t=agent._adam_t)
    if agent.ret_rms is not None:
        out["block"] = agent.ret_rms.block
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def assert_bit_equal(a, b, keys=None):
    for k in keys or a:
        assert a[k].tobytes() == b[k].tobytes(), k


CASES = {
    "64-32-b64-moving": dict(shape=(2, 64, 32, 64), reward="moving"),     # the shape that leaves the one-workgroup kernel
    "64-32-b64-floor": dict(shape=(2, 64, 32, 64), reward="floor"),
    "64-32-b50-floor": dict(shape=(3, 64, 32, 50), reward="floor"),       # ragged 16-row tile
    "37-19-b77-moving": dict(shape=(8, 37, 19, 77), reward="moving"),
    "200-100-b256-moving": dict(shape=(3, 200, 100, 256), reward="moving"),
    "64-32-b4096-moving": dict(shape=(2, 64, 32, 4096), reward="moving"),  # 256 partials
    "64-64ln-b256-moving": dict(shape=(3, 64, 64, 256), reward="moving", layer_norm=True, critic_l2_reg=1e-2, clip_norm=0.05),
    "128-64-b64-floor-obs": dict(shape=(3, 128, 64, 64), reward="floor", obs_stats=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_vs_restatement(ssc, name):
    """Six Pop-Art iterations: actor, critic and both targets within 5e-6, all four moment arrays and both losses per
    iteration within the bounds of _ddpg_kernel_vs_oracle; count exact; sum / sumsq within 2e-6 of sum |y| / sum y^2.
    y of the last iteration: q' = W3 . a2 + b3 of the target critic carries the parameter tolerance of its h2 + 1 output
    parameters (5e-6 each, independent roundings: in quadrature, twice over for the layers below), scaled by sigma_old,
    plus four fp32 roundings of y itself -- 1e-5 sqrt(h2 + 1) sigma_old + 4 * 2^-24 |y|."""
    from tests.gpu_util import rms_edge_stats, x_hat64
    c = CASES[name]
    od, h1, h2, B = c["shape"]
    obs_rms = obs_range = net_inputs = None
    if c.get("obs_stats"):
        obs_rms, obs_range = rms_edge_stats(od, "wide")
    case = PC.make_case(od, h1, h2, B, c["reward"], layer_norm=c.get("layer_norm", False), obs_range=obs_range)
    l2, clip = c.get("critic_l2_reg", 0.0), c.get("clip_norm")
    if obs_rms is not None:
        net_inputs = (x_hat64(case["rows"][0], obs_rms), x_hat64(case["rows"][4], obs_rms))
    ref = PC.run_restatement(case, critic_l2_reg=l2, clip_norm=clip, net_inputs=net_inputs)
    agent = make_agent(case, critic_l2_reg=l2, clip_norm=clip)
    losses = train(agent, case, **({} if obs_rms is None else dict(obs_rms=obs_rms)))
    torch.cuda.synchronize()
    got = state_of(agent)
    ws = {k: v.cpu().numpy() for k, v in agent.popart_workspace().items()}
    assert got["adam_t"].tolist() == [PC.N_ITERS, PC.N_ITERS]
    err = {k: float(np.max(np.abs(got[k] - O.flatten_params(ref[k])))) for k in ("actor", "critic", "target_actor", "target_critic")}
    print(name, "max parameter errors", err, "block", got["block"].tolist(), "ref", ref["block"].tolist())
    got_l = losses.cpu().numpy()
    assert np.allclose(got_l, ref["losses"], rtol=2e-4, atol=1e-6), (got_l, ref["losses"])
    for k, e in err.items():
        assert e <= TOL, (k, e)
    for net in ("actor", "critic"):
        assert np.allclose(got["m_" + net], ref["adam"]["m_" + net], rtol=1e-3, atol=1e-7), "m_" + net
        assert np.allclose(got["v_" + net], ref["adam"]["v_" + net], rtol=2e-3, atol=1e-9), "v_" + net
    # the block
    count = 1e-2
    for _ in range(PC.N_ITERS):
        count += float(B)
    assert got["block"][2] == count
    all_y = np.concatenate(ref["y"])
    assert abs(got["block"][0] - ref["block"][0]) <= 2e-6 * np.sum(np.abs(all_y))
    assert abs(got["block"][1] - ref["block"][1]) <= 2e-6 * np.sum(np.square(all_y))
    # y and the scalars of the last iteration
    sg_old = ref["scalars"][-1][1]
    y_tol = 1e-5 * np.sqrt(h2 + 1) * sg_old + 4 * 2.0 ** -24 * np.abs(ref["y"][-1])
    assert np.all(np.abs(ws["y"] - ref["y"][-1]) <= y_tol), float(np.max(np.abs(ws["y"] - ref["y"][-1]) / y_tol))
    # the scalars: mu within the sums' bound (2e-6 of the mean |y|) plus one fp32 rounding; sigma^2 is a difference of two
    # terms each within 2e-6 of the mean square, and the moving cases keep it above a fifth of that: 1e-5 + rounding on
    # sigma^2, half of it on sigma; the floor cases sit on the floor exactly
    want_sc = np.asarray(ref["scalars"][-1])
    for j in (0, 2):
        assert abs(ws["scalars"][j] - want_sc[j]) <= 2e-6 * np.mean(np.abs(all_y)) + 2.0 ** -23 * abs(want_sc[j]), j
    if c["reward"] == "floor":
        assert ws["scalars"][1] == ws["scalars"][3] == np.float32(0.1)
    else:
        assert np.allclose(ws["scalars"][[1, 3]], want_sc[[1, 3]], rtol=1e-5, atol=0)
    # the partials of the last iteration add up to its y
    assert np.allclose(ws["partials"].sum(0), [ws["y"].astype(np.float64).sum(), np.square(ws["y"].astype(np.float64)).sum()],
                       rtol=1e-12, atol=0)


def critic_desc_over(agent, flat):
    """the agent's critic descriptor over another flat array of the same layout (the target critic)"""
    from smartstartcontinuous_amd import _ffi
    views, o = {}, 0
    for k, v in agent.critic_weights.items():
        views[k] = flat[o:o + v.numel()].view(v.shape)
        o += v.numel()
    d = _ffi.CriticDesc.from_buffer_copy(agent._critic_desc)
    d.W1, d.b1, d.W2, d.b2, d.W3, d.b3 = (views[k].data_ptr() for k in ("W1", "b1", "W2", "b2", "W3", "b3"))
    return d


def raw_q(agent, desc, s, a):
    from smartstartcontinuous_amd import _ffi
    q = torch.empty(s.shape[0], dtype=torch.float32, device="cuda")
    _ffi.check(agent.lib.ssc_critic_forward(ctypes.byref(desc), s.shape[0], _ffi.ptr(s), _ffi.ptr(a), _ffi.ptr(q),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return q.cpu().numpy().astype(np.float64)


def test_preserved_outputs_on_the_device(ssc):
    """One iteration with both learning rates and tau at zero, from statistics away from (0, 1): on 256 probe rows
    sigma_new q_new + mu_new stays within 8 * 2^-24 (|sigma q| + |mu|) of sigma_old q_old + mu_old, for the critic and for
    the target critic's flat array (this fails when the target critic is not rescaled, or with the wrong statistics).
    The rescaling leaves the Adam moments alone: the moments of W3 and b3 after the iteration are those of the
    iteration's own gradient -- (1 - beta) g and (1 - beta2) g^2 of the restatement -- not scaled with the layer.  (They
    cannot stay zero: the gradient step of the same iteration adds its gradient to them even at a zero learning rate.)"""
    case = PC.make_case(3, 64, 32, 128, "moving")
    block0 = np.array([130.0, 9100.0, 64.01])
    agent = make_agent(case, actor_lr=0.0, critic_lr=0.0, tau=0.0)
    agent.ret_rms.block.copy_(torch.as_tensor(block0))
    rows = device_rows(case)
    s, a = rows[0][:256].contiguous(), rows[1][:256].contiguous()
    descs = dict(critic=agent._critic_desc, target_critic=critic_desc_over(agent, agent.target_critic_flat))
    before = {k: raw_q(agent, d, s, a) for k, d in descs.items()}
    train(agent, case, 0, 1, rows=rows)
    torch.cuda.synchronize()
    mu_o, sg_o, mu_n, sg_n = (float(x) for x in agent.popart_workspace()["scalars"].cpu().numpy())
    assert (mu_o, sg_o) == PC.ret_mean_std(block0) and abs(mu_n - mu_o) > 0.1 and abs(sg_n - sg_o) > 0.1
    for k, d in descs.items():
        after = raw_q(agent, d, s, a)
        old, new = sg_o * before[k] + mu_o, sg_n * after + mu_n
        bound = 8 * 2.0 ** -24 * (np.abs(sg_o * before[k]) + abs(mu_o))
        assert np.all(np.abs(new - old) <= bound), (k, float(np.max(np.abs(new - old) / bound)))
    ref = PC.run_restatement(case, n_iters=1, actor_lr=0.0, critic_lr=0.0, tau=0.0, block=block0)
    tail = slice(-(case["h2"] + 1), None)                      # [W3 | b3] end the flat critic vector
    assert np.allclose(agent._adam_critic[0].cpu().numpy()[tail], ref["adam"]["m_critic"][tail], rtol=1e-3, atol=1e-7)
    assert np.allclose(agent._adam_critic[1].cpu().numpy()[tail], ref["adam"]["v_critic"][tail], rtol=2e-3, atol=1e-9)
    assert np.max(np.abs(agent.critic_flat.cpu().numpy() - O.flatten_params(ref["critic"]))) <= TOL
    assert np.max(np.abs(agent.target_critic_flat.cpu().numpy() - O.flatten_params(ref["target_critic"]))) <= TOL


@pytest.mark.parametrize("shape", [(2, 64, 32, 64), (3, 200, 100, 256)])
def test_null_block_is_the_plain_step(ssc, shape):
    """ssc_ddpg_train_ws_popart with d_ret_rms == NULL is ssc_ddpg_train_ws_rms: parameters, targets, moments and losses
    bit-equal to the plain agent's train_on (64-32 x 64 then runs the one-workgroup kernel, as the plain call does); the
    plain agent's get_stats has no ret_rms entries.  (One switch without the other -- the plain step in the reference --
    is refused by the constructor: tests/test_ddpg_popart_host.py.)"""
    from smartstartcontinuous_amd import _ffi
    case = PC.make_case(*shape, "moving")
    rows = device_rows(case)
    plain = make_agent(case, normalize_returns=False, enable_popart=False)
    l_plain = train(plain, case, rows=rows).cpu().numpy()
    want = state_of(plain)
    other = make_agent(case, normalize_returns=False, enable_popart=False)
    d = other.ddpg_desc()
    need = int(other.lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx = torch.as_tensor(case["idx"], dtype=torch.int32, device="cuda").contiguous()
    losses = torch.empty((idx.shape[0], 2), dtype=torch.float32, device="cuda")
    rv = _ffi.ReplayView(*(x.data_ptr() for x in rows), rows[0].shape[0])
    _ffi.check(other.lib.ssc_ddpg_train_ws_popart(ctypes.byref(d), ctypes.byref(rv), _ffi.ptr(idx), idx.shape[0], _ffi.ptr(losses),
                                                  _ffi.ptr(ws), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                                  None, None))
    assert losses.cpu().numpy().tobytes() == l_plain.tobytes()
    assert_bit_equal(want, state_of(other))
    plain.set_stats_sample(case["rows"][0][:64], case["rows"][1][:64])
    stats = plain.get_stats()
    assert "ret_rms_mean" not in stats and "ret_rms_std" not in stats


def test_same_bits_run_to_run(ssc):
    case = PC.make_case(3, 200, 100, 256, "moving")
    rows = device_rows(case)
    runs = []
    for _ in range(2):
        agent = make_agent(case)
        l = train(agent, case, rows=rows).cpu().numpy()
        runs.append((l, state_of(agent), agent.popart_workspace()["y"].cpu().numpy().copy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()
    assert_bit_equal(runs[0][1], runs[1][1])


def test_statistics_carried_across_calls(ssc):
    """3 + 3 iterations in two train_on calls equal 6 in one, bit for bit"""
    case = PC.make_case(2, 64, 32, 64, "moving")
    rows = device_rows(case)
    one, two = make_agent(case), make_agent(case)
    l1 = train(one, case, rows=rows).cpu().numpy()
    l2 = np.concatenate([train(two, case, 0, 3, rows=rows).cpu().numpy(), train(two, case, 3, 6, rows=rows).cpu().numpy()])
    assert l1.tobytes() == l2.tobytes()
    assert_bit_equal(state_of(one), state_of(two))


def test_workspace_guards(ssc):
    """a workspace of exactly ssc_ddpg_train_popart_workspace_bytes between 4 KiB canaries, canaries around d_losses and
    around the block: all intact after two iterations; one byte less is SSC_EINVAL before any launch"""
    from smartstartcontinuous_amd import _ffi
    case = PC.make_case(3, 64, 32, 50, "moving")
    agent = make_agent(case)
    rows = device_rows(case)
    d = agent.ddpg_desc()
    need = int(agent.lib.ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d)))
    G, n_iters = 4096, 2

    def guarded(nbytes):
        buf = torch.full((G + nbytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[G:G + nbytes]
    ws_buf, ws = guarded(need)
    l_buf, l_mid = guarded(n_iters * 2 * 4)
    b_buf, b_mid = guarded(3 * 8)
    b_mid.view(torch.float64).copy_(agent.ret_rms.block)
    idx = torch.as_tensor(case["idx"][:n_iters], dtype=torch.int32, device="cuda").contiguous()
    rv = _ffi.ReplayView(*(x.data_ptr() for x in rows), rows[0].shape[0])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ws_bytes):
        return agent.lib.ssc_ddpg_train_ws_popart(ctypes.byref(d), ctypes.byref(rv), _ffi.ptr(idx), n_iters, _ffi.ptr(l_mid),
                                                  _ffi.ptr(ws), ws_bytes, stream, None, _ffi.ptr(b_mid))
    before = state_of(agent)
    assert call(need - 1) == _ffi.SSC_EINVAL and b"workspace" in agent.lib.ssc_last_error()
    torch.cuda.synchronize()
    assert_bit_equal(before, state_of(agent))                       # nothing ran
    assert b_mid.view(torch.float64).cpu().tolist() == [0.0, 1e-2, 1e-2]
    _ffi.check(call(need))
    torch.cuda.synchronize()
    for buf, n in ((ws_buf, need), (l_buf, n_iters * 8), (b_buf, 24)):
        host = buf.cpu().numpy()
        assert np.all(host[:G] == 0xA5) and np.all(host[G + n:] == 0xA5)
    assert b_mid.view(torch.float64)[2].item() == 1e-2 + 50.0 + 50.0
    # the same two iterations through the agent's own workspace
    other = make_agent(case)
    l = train(other, case, 0, n_iters, rows=rows)
    assert l_mid.view(torch.float32).cpu().numpy().tobytes() == l.cpu().numpy().tobytes()
    assert b_mid.view(torch.float64).cpu().numpy().tobytes() == other.ret_rms.block.cpu().numpy().tobytes()


def test_read_outs(ssc):
    """state_value_device = sigma * raw + mu of mean_std_device(), bit for bit; mean_std_device() = the kernel's scalars,
    bit for bit; the Q slots of get_stats_device and eval/Q, eval/Q_std of evaluate_device = the affine map, applied in
    f64, of what an agent with the same networks and no return statistics reads, within 4 * 2^-53 relative"""
    case = PC.make_case(2, 64, 32, 64, "moving")
    agent = make_agent(case)
    train(agent, case, 0, 3)
    mean, std = agent.ret_rms.mean_std_device()
    sc = agent.popart_workspace()["scalars"].cpu().numpy()
    assert mean.cpu().numpy().tobytes() == sc[2:3].tobytes() and std.cpu().numpy().tobytes() == sc[3:4].tobytes()
    assert sc[3] > 3.0
    host_mean, host_std = agent.ret_rms.mean_std()
    assert host_mean.tobytes() == sc[2:3].tobytes() and host_std.tobytes() == sc[3:4].tobytes()
    states = torch.as_tensor(case["rows"][0][:300], device="cuda")
    raw = agent.state_value_device(states, raw=True)
    assert agent.state_value_device(states).cpu().numpy().tobytes() == (raw * std + mean).cpu().numpy().tobytes()
    assert np.array_equal(agent.get_state_value(states), (raw * std + mean).reshape(-1, 1).double().cpu().numpy())
    assert np.array_equal(agent.get_state_value(states, raw=True), raw.reshape(-1, 1).double().cpu().numpy())
    # a plain agent over the same networks
    plain = make_agent(case, normalize_returns=False, enable_popart=False)
    plain.actor_flat.copy_(agent.actor_flat)
    plain.critic_flat.copy_(agent.critic_flat)
    sample = (case["rows"][0][100:164], case["rows"][1][100:164])
    agent.set_stats_sample(*sample)
    plain.set_stats_sample(*sample)
    got, base = agent.get_stats_device().cpu().numpy(), plain.get_stats_device().cpu().numpy()
    mu, sg = float(sc[2]), float(sc[3])
    eps = 4 * 2.0 ** -53
    for j in (2, 4):
        assert abs(got[j] - (base[j] * sg + mu)) <= eps * (abs(base[j] * sg) + abs(mu))
    for j in (3, 5):
        assert abs(got[j] - base[j] * sg) <= eps * abs(base[j] * sg)
    rest = [j for j in range(len(got)) if j not in (2, 3, 4, 5)]
    assert np.array_equal(got[rest], base[rest], equal_nan=True)
    stats = agent.get_stats()
    assert list(stats)[:2] == ["ret_rms_mean", "ret_rms_std"] and stats["ret_rms_mean"] == mu and stats["ret_rms_std"] == sg
    assert stats["reference_Q_mean"] == got[2]
    # evaluation: two env sets with the same seed
    K, n = 8, 64
    envs = [ssc.VecEnv("MountainCarContinuous-v0", n, seed=3, env_id0=1000) for _ in range(2)]
    q = [torch.empty((K, n), dtype=torch.float32, device="cuda") for _ in range(2)]
    ev = agent.evaluate_device(envs[0], K, q=q[0]).cpu().numpy()
    ev0 = plain.evaluate_device(envs[1], K, q=q[1]).cpu().numpy()
    assert abs(ev[3] - (ev0[3] * sg + mu)) <= eps * (abs(ev0[3] * sg) + abs(mu))
    assert abs(ev[4] - ev0[4] * sg) <= eps * abs(ev0[4] * sg)
    others = [j for j in range(len(ev)) if j not in (3, 4)]
    assert np.array_equal(ev[others], ev0[others], equal_nan=True)
    assert q[0].cpu().numpy().tobytes() == (q[1] * std + mean).cpu().numpy().tobytes()
