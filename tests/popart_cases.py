"""Pop-Art (normalize_returns + enable_popart) for the DDPG learner: the fp64 restatement of one iteration of
``DDPG_editted.train`` + ``update_target_net`` with return statistics (ddpg_editted.py:129-133, 140-149, 201-217,
291-301) and the shared cases of the CPU and GPU tests.

The restatement is built on the oracle's forwards (``actor_forward`` / ``critic_forward``), its backward helpers and the
MpiAdam of ``ddpg_train_step``; tests/test_popart_cases_cpu.py holds its gradients to torch autograd.  The statistics are
baselines' RunningMeanStd with one column, ``[sum | sumsq | count]`` in f64, and the mean / std derived from them in the
fp32 arithmetic of the reference's graph (``obs_rms.mean_std_f32``) -- the restatement uses those fp32 VALUES in fp64
arithmetic, so what it is compared with may differ by the roundings of fp32 operations only.
"""
import numpy as np

from oracle import ssc_oracle as O
from smartstartcontinuous_amd.obs_rms import mean_std_f32, rms_initial

GAMMA, TAU, LR, OBS_CLIP = 0.99, 0.001, 1e-3, 5.0
N_ROWS, N_ITERS = 5000, 6


def ret_mean_std(block):
    """(mu, sigma) of a one-column block: the fp32 values, as Python floats"""
    mean, std = mean_std_f32(block, 1)
    return float(mean[0]), float(std[0])


def _ln(p):
    return ((p["ln1_g"], p["ln1_b"]), (p["ln2_g"], p["ln2_b"])) if "ln1_g" in p else None


def pi_of(actor, s, llt=True):
    return O.actor_forward(s, *(actor[k] for k in O.ACTOR_KEYS), last_layer_tanh=llt, layer_norm=_ln(actor), obs_clip=OBS_CLIP)


def q_of(critic, s, a, llt=True):
    """the critic's own (normalised) output, [B, 1]"""
    return O.critic_forward(s, a, *(critic[k] for k in O.ACTOR_KEYS), last_layer_tanh=llt, obs_clip=OBS_CLIP, layer_norm=_ln(critic))


def rescale_output_layer(p, mu_old, sg_old, mu_new, sg_new):
    """setup_popart (:209-217): M <- M * old_std / new_std, b <- (b * old_std + old_mean - new_mean) / new_std"""
    q = dict(p)
    q["W3"] = np.asarray(p["W3"], np.float64) * sg_old / sg_new
    q["b3"] = (np.asarray(p["b3"], np.float64) * sg_old + mu_old - mu_new) / sg_new
    return q


def popart_targets(target_actor, target_critic, block, batch, llt=True, gamma=GAMMA):
    """step 1: y = r + (1 - t) gamma (q' sigma_old + mu_old), [B, 1]"""
    s, a, r, t, s2 = (np.asarray(x, np.float64) for x in batch)
    mu, sg = ret_mean_std(block)
    q1 = q_of(target_critic, s2, pi_of(target_actor, s2, llt), llt)
    return r.reshape(-1, 1) + (1.0 - t.reshape(-1, 1)) * gamma * (q1 * sg + mu)


def update_block(block, y):
    """step 2: RunningMeanStd.update (:297)"""
    y = np.asarray(y, np.float64).reshape(-1)
    return np.asarray(block, np.float64) + np.array([y.sum(), np.square(y).sum(), float(len(y))])


def popart_losses_and_grads(actor, critic, batch, y, mu, sg, llt=True, critic_l2_reg=0.0):
    """step 4 up to the optimiser: (critic gradients, actor gradients, critic loss, actor loss) with
    critic loss mean((q - (y - mu) / sg)^2) (+ l2) and actor loss -mean(q(s, pi(s)) sg + mu)"""
    s, a = O.clip_observation(np.asarray(batch[0], np.float64), OBS_CLIP), np.asarray(batch[1], np.float64)
    B = len(s)
    yn = (np.asarray(y, np.float64).reshape(B, 1) - mu) / sg
    q, cc = O._critic_fwd_cache(critic, s, a, llt)
    critic_loss = float(np.mean((q - yn) ** 2))
    gc, _ = O._critic_bwd(critic, cc, 2.0 * (q - yn) / B, llt)
    if critic_l2_reg:
        for k in ("W1", "W2", "W3"):
            critic_loss += 0.5 * critic_l2_reg * float(np.sum(np.square(critic[k])))
            gc[k] = gc[k] + critic_l2_reg * critic[k]
    pi, ac = O._actor_fwd_cache(actor, s, llt)
    qpi, cc2 = O._critic_fwd_cache(critic, s, pi, llt)
    actor_loss = float(-np.mean(qpi * sg + mu))
    _, dact = O._critic_bwd(critic, cc2, np.full((B, 1), -sg / B), llt, want_weights=False)
    ga = O._actor_bwd(actor, ac, dact, llt)
    return gc, ga, critic_loss, actor_loss


def popart_step(actor, critic, target_actor, target_critic, adam, block, batch, llt=True, gamma=GAMMA, tau=TAU, actor_lr=LR,
                critic_lr=LR, critic_l2_reg=0.0, clip_norm=None):
    """One Pop-Art iteration.  Returns (actor', critic', target_actor', target_critic', adam', block', critic_loss,
    actor_loss, y, (mu_old, sigma_old, mu_new, sigma_new))."""
    y = popart_targets(target_actor, target_critic, block, batch, llt, gamma)
    mu_o, sg_o = ret_mean_std(block)
    block2 = update_block(block, y)
    mu_n, sg_n = ret_mean_std(block2)
    critic = rescale_output_layer(critic, mu_o, sg_o, mu_n, sg_n)
    target_critic = rescale_output_layer(target_critic, mu_o, sg_o, mu_n, sg_n)
    gc, ga, cl, al = popart_losses_and_grads(actor, critic, batch, y, mu_n, sg_n, llt, critic_l2_reg)
    if clip_norm is not None:
        gc = {k: O.clip_by_norm(v, clip_norm) for k, v in gc.items()}
        ga = {k: O.clip_by_norm(v, clip_norm) for k, v in ga.items()}
    fa, ma, va, ta = O.adam_update(O.flatten_params(actor), O.flatten_params(ga), adam["m_actor"], adam["v_actor"], adam["t_actor"], actor_lr)
    fc, mc, vc, tc = O.adam_update(O.flatten_params(critic), O.flatten_params(gc), adam["m_critic"], adam["v_critic"], adam["t_critic"], critic_lr)
    actor2, critic2 = O.unflatten_params(fa, actor), O.unflatten_params(fc, critic)
    ta2 = {k: (1 - tau) * np.asarray(target_actor[k], np.float64) + tau * actor2[k] for k in O.param_keys(actor)}
    tc2 = {k: (1 - tau) * np.asarray(target_critic[k], np.float64) + tau * critic2[k] for k in O.param_keys(critic)}
    adam2 = dict(m_actor=ma, v_actor=va, t_actor=ta, m_critic=mc, v_critic=vc, t_critic=tc)
    return actor2, critic2, ta2, tc2, adam2, block2, cl, al, y, (mu_o, sg_o, mu_n, sg_n)


# ---- the cases --------------------------------------------------------------------------------------------------------
def make_case(obs_dim, h1, h2, B, reward, layer_norm=False, n_iters=N_ITERS, obs_range=None, seed=11):
    """A replay of N_ROWS rows drawn as tests/test_gpu_agents.py::_ddpg_kernel_vs_oracle draws them, fp32 networks with every
    parameter perturbed by 0.05 N(0, 1) and the targets shifted by +-0.01, and ``n_iters`` batches of ``B`` row indices.
      reward "floor":  r = 0.02 N(0, 1); every batch from all rows, without replacement: the variance of y stays under the
                       1e-2 floor, sigma sits on it;
      reward "moving": iteration k draws its batch from the k-th sixth of the rows, whose rewards are
                       (1 + 1.5 k) (5 N(0, 1) + 3): mean and std of the returns grow from one iteration to the next
                       (without replacement while a sixth holds B rows, with replacement above).
    Returns a dict: actor / critic / target_actor / target_critic (dicts of fp32 arrays), rows = (s, a, r, t, s2), idx."""
    import torch
    from smartstartcontinuous_amd.agents import init_actor_weights, init_critic_weights, with_layer_norm
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(5)
    aw, cw = init_actor_weights(obs_dim, h1, h2, 1, gen), init_critic_weights(obs_dim, h1, h2, 1, gen)
    if layer_norm:
        aw, cw = with_layer_norm(aw), with_layer_norm(cw)
    order = O.LN_KEYS if layer_norm else O.ACTOR_KEYS
    aw = {k: aw[k].numpy() + (0.05 * rng.normal(size=tuple(aw[k].shape))).astype(np.float32) for k in order}
    cw = {k: cw[k].numpy() + (0.05 * rng.normal(size=tuple(cw[k].shape))).astype(np.float32) for k in order}
    ta = {k: (v + np.float32(0.01)).astype(np.float32) for k, v in aw.items()}
    tc = {k: (v - np.float32(0.01)).astype(np.float32) for k, v in cw.items()}
    if reward == "floor":
        # q' = W3 . a2 + b3 over h2 units of size ~1: perturbed by 0.05 and shifted by 0.01 its spread over the rows, and its
        # mean through the (1 - t) factor, put Var(y) past the floor for the wider critics (4e-2 at 200-100).  The floor
        # cases scale both critics' output layers, perturbation and shift included, by 0.1.
        for p in (cw, tc):
            p["W3"], p["b3"] = (p["W3"] * np.float32(0.1)).astype(np.float32), (p["b3"] * np.float32(0.1)).astype(np.float32)
    cap = N_ROWS
    if obs_range is not None:
        s = rng.uniform(obs_range[0], obs_range[1], (cap, obs_dim)).astype(np.float32)
    else:
        s = rng.uniform(-1.2, 0.6, (cap, obs_dim)).astype(np.float32)
        if obs_dim == 3:
            s[:, 2] = rng.uniform(-8, 8, cap)                # observation_range (-5, 5) clips it
    a = rng.uniform(-1, 1, (cap, 1)).astype(np.float32)
    t = rng.random(cap) < 0.1
    s2 = (s + rng.normal(size=(cap, obs_dim)) * 0.01).astype(np.float32)
    if reward == "floor":
        r = (0.02 * rng.normal(size=cap)).astype(np.float32)
        idx = np.stack([rng.permutation(cap)[:B] for _ in range(n_iters)]).astype(np.int32)
    else:
        assert reward == "moving" and n_iters <= 6
        sixth = cap // 6
        r = np.zeros(cap, np.float32)
        idx = np.zeros((n_iters, B), np.int32)
        for k in range(6):
            r[k * sixth:(k + 1) * sixth] = ((1 + 1.5 * k) * (5 * rng.normal(size=sixth) + 3)).astype(np.float32)
        for k in range(n_iters):
            idx[k] = k * sixth + (rng.permutation(sixth)[:B] if B <= sixth else rng.integers(0, sixth, B))
    return dict(actor=aw, critic=cw, target_actor=ta, target_critic=tc, rows=(s, a, r, t, s2), idx=idx, B=B,
                layer_norm=layer_norm, obs_dim=obs_dim, h1=h1, h2=h2)


def run_restatement(case, n_iters=None, critic_l2_reg=0.0, clip_norm=None, net_inputs=None, actor_lr=LR, critic_lr=LR, tau=TAU,
                    block=None):
    """``n_iters`` Pop-Art iterations of the restatement on a case.  ``net_inputs`` = (s_hat, s2_hat): what the networks
    see in place of the raw observations (normalize_observations).  Returns a dict with the final state and the history
    (losses [n, 2], y of every iteration, block after every iteration, the four scalars of every iteration)."""
    f64 = lambda p: {k: np.asarray(v, np.float64) for k, v in p.items()}
    a, c, ta, tc = f64(case["actor"]), f64(case["critic"]), f64(case["target_actor"]), f64(case["target_critic"])
    na, nc = O.flatten_params(a).size, O.flatten_params(c).size
    adam = dict(m_actor=np.zeros(na), v_actor=np.zeros(na), t_actor=0, m_critic=np.zeros(nc), v_critic=np.zeros(nc), t_critic=0)
    block = rms_initial(1) if block is None else np.asarray(block, np.float64)
    s, act, r, t, s2 = case["rows"]
    if net_inputs is not None:
        s, s2 = net_inputs
    idx = case["idx"] if n_iters is None else case["idx"][:n_iters]
    losses, ys, blocks, scalars = [], [], [], []
    for bi in idx:
        a, c, ta, tc, adam, block, cl, al, y, sc = popart_step(a, c, ta, tc, adam, block, (s[bi], act[bi], r[bi], t[bi], s2[bi]),
                                                               actor_lr=actor_lr, critic_lr=critic_lr, tau=tau,
                                                               critic_l2_reg=critic_l2_reg, clip_norm=clip_norm)
        losses.append((cl, al)); ys.append(y.reshape(-1)); blocks.append(block); scalars.append(sc)
    return dict(actor=a, critic=c, target_actor=ta, target_critic=tc, adam=adam, block=block, losses=np.asarray(losses),
                y=ys, blocks=blocks, scalars=scalars)
