"""The fp64 restatement of the Pop-Art iteration (tests/popart_cases.py) checked on the CPU: its gradients against torch
autograd, the output-preserving rescaling, and the conditions the shared cases are built to meet."""
import numpy as np
import pytest
import torch

from oracle import ssc_oracle as O
from tests import popart_cases as PC


def _torch_net(p):
    return {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}


def _t_ln(z, p, which):
    if which + "_g" not in p:
        return z
    mean = z.mean(dim=-1, keepdim=True)
    var = ((z - mean) ** 2).mean(dim=-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + 1e-12) * p[which + "_g"] + p[which + "_b"]


def _t_actor(p, s):
    u1 = torch.relu(_t_ln(s @ p["W1"] + p["b1"], p, "ln1"))
    u2 = torch.tanh(_t_ln(u1 @ p["W2"] + p["b2"], p, "ln2"))
    return torch.tanh(u2 @ p["W3"] + p["b3"])


def _t_critic(p, s, a):
    a1 = torch.relu(_t_ln(s @ p["W1"] + p["b1"], p, "ln1"))
    a2 = torch.tanh(_t_ln(torch.cat([a1, a], dim=1) @ p["W2"] + p["b2"], p, "ln2"))
    return a2 @ p["W3"] + p["b3"]


@pytest.mark.parametrize("obs_dim,h1,h2,B", [(2, 64, 32, 64), (8, 37, 19, 77)])
@pytest.mark.parametrize("layer_norm", [False, True])
def test_gradients_match_autograd(obs_dim, h1, h2, B, layer_norm):
    """critic and actor gradients of the restatement (normalised TD error, sigma-scaled actor delta, l2 term over the
    three dense kernels) against torch autograd in float64: 1e-10 relative"""
    case = PC.make_case(obs_dim, h1, h2, B, "moving", layer_norm=layer_norm)
    f64 = lambda p: {k: np.asarray(v, np.float64) for k, v in p.items()}
    actor, critic = f64(case["actor"]), f64(case["critic"])
    s, a, r, t, s2 = (x[case["idx"][1]] for x in case["rows"])
    rng = np.random.default_rng(3)
    y, mu, sg, l2 = rng.normal(20.0, 15.0, (B, 1)), 7.25, 11.5, 1e-2
    gc, ga, cl, al = PC.popart_losses_and_grads(actor, critic, (s, a), y, mu, sg, True, critic_l2_reg=l2)
    ta, tcr = _torch_net(actor), _torch_net(critic)
    ts = torch.tensor(np.clip(s.astype(np.float64), -5, 5))
    closs = ((_t_critic(tcr, ts, torch.tensor(a.astype(np.float64))) - torch.tensor((y - mu) / sg)) ** 2).mean()
    closs = closs + sum(0.5 * l2 * (tcr[k] ** 2).sum() for k in ("W1", "W2", "W3"))
    tgc = dict(zip(tcr, torch.autograd.grad(closs, list(tcr.values()))))
    aloss = -(_t_critic(tcr, ts, _t_actor(ta, ts)) * sg + mu).mean()
    tga = dict(zip(ta, torch.autograd.grad(aloss, list(ta.values()))))
    assert cl == pytest.approx(closs.item(), rel=1e-12) and al == pytest.approx(aloss.item(), rel=1e-12)
    for name, got, ref in (("critic", gc, tgc), ("actor", ga, tga)):
        for k in ref:
            g, w = np.asarray(got[k]).reshape(-1), ref[k].numpy().reshape(-1)
            assert np.max(np.abs(g - w)) <= 1e-10 * np.max(np.abs(w)), (name, k)


@pytest.mark.parametrize("obs_dim,h1,h2,B", [(2, 64, 32, 64), (3, 200, 100, 256)])
def test_rescaling_preserves_outputs(obs_dim, h1, h2, B):
    """after step 3, sigma_new q_new + mu_new equals sigma_old q_old + mu_old for the critic and the target critic"""
    case = PC.make_case(obs_dim, h1, h2, B, "moving")
    f64 = lambda p: {k: np.asarray(v, np.float64) for k, v in p.items()}
    s, a = case["rows"][0][:256], case["rows"][1][:256]
    block = np.array([130.0, 9100.0, 64.01])                 # mu about 2, sigma about 11.7: away from the initial (0, 1)
    mu_o, sg_o = PC.ret_mean_std(block)
    bi = case["idx"][2]
    y = PC.popart_targets(f64(case["target_actor"]), f64(case["target_critic"]), block, tuple(x[bi] for x in case["rows"]))
    mu_n, sg_n = PC.ret_mean_std(PC.update_block(block, y))
    assert abs(mu_n - mu_o) > 0.1 and abs(sg_n - sg_o) > 0.1
    for net in ("critic", "target_critic"):
        p = f64(case[net])
        before = sg_o * PC.q_of(p, s, a) + mu_o
        after = sg_n * PC.q_of(PC.rescale_output_layer(p, mu_o, sg_o, mu_n, sg_n), s, a) + mu_n
        assert np.max(np.abs(after - before)) <= 1e-12 * max(1.0, np.max(np.abs(before))), net


@pytest.mark.parametrize("obs_dim,h1,h2,B", [(2, 64, 32, 64), (3, 200, 100, 256)])
def test_case_conditions(obs_dim, h1, h2, B):
    """floor: the fp32 variance stays under 5e-3 at every iteration, so sigma sits on the floor; moving: sigma exceeds 3
    after the first iteration and then grows by more than 10 % per iteration, mu moves by more than 0.1 per iteration"""
    res = PC.run_restatement(PC.make_case(obs_dim, h1, h2, B, "floor"))
    for block, sc in zip(res["blocks"], res["scalars"]):
        mean = np.float32(block[0] / block[2])
        var = np.float32(block[1] / block[2]) - mean * mean
        assert var < 5e-3, var
        assert sc[3] == float(np.float32(0.1))
    res = PC.run_restatement(PC.make_case(obs_dim, h1, h2, B, "moving"))
    sg = [sc[3] for sc in res["scalars"]]
    mu = [0.0] + [sc[2] for sc in res["scalars"]]
    assert sg[0] > 3.0
    assert all(b > 1.1 * a for a, b in zip(sg, sg[1:])), sg
    assert all(abs(b - a) > 0.1 for a, b in zip(mu, mu[1:])), mu
