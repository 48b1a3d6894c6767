"""Case matrix of the Pop-Art learner (normalize_returns + enable_popart; csrc/ddpg_train_wide.hip: ddpg_wide_grad_kernel<...,
PopTarget> / <..., PopGrad>, ddpg_popart_renorm_kernel and the apply pass behind them): the derived float32 bound of
tests/ddpg_cases.py carried through ONE Pop-Art iteration from a given return block.  The case table with the kernels each
case launches, each case's inputs, ``popart_step1`` (the iteration in fp64 with the error sizes E, or in float32 one rounding
at a time), the checks the GPU test applies to what the device leaves, and the mutants those checks must reject.  Shared by
tests/test_popart_grad_cases_cpu.py and tests/test_gpu_ddpg_popart_matrix.py; numpy + tests/ddpg_cases.py only.

The iteration, in kernel order, from the f64 block [sum | sumsq | count]:
  1 target pass   (mu_o, sigma_o) from the block in the fp32 arithmetic of obs_rms.mean_std_f32 (``mean_std32`` restates it);
                  y = r + (1 - t) gamma (q' sigma_o + mu_o), q' the target critic's own (normalised) output
  2 block update  sum += sum y, sumsq += sum y^2, count += B in f64 on the float32 y; (mu_n, sigma_n) from the new block
  3 rescale       W3 <- (W3 sigma_o) / sigma_n, b3 <- ((b3 sigma_o + mu_o) - mu_n) / sigma_n for the critic and the target critic
  4 gradient pass on the rescaled critic: e = q - (y - mu_n) / sigma_n, dq = 2 e / B, the actor's seed -sigma_n / B; critic
                  loss mean(e^2) (+ l2), actor loss -mean(q_pi sigma_n + mu_n)

The error sizes E of tests/ddpg_cases.py (units of one float32 rounding; a sum rounds once at the size of its terms,
independent roundings add in quadrature) go through the new operations like this:
  old stats   (mu_o, sigma_o) are float32 values that the device and the restatement derive from the same f64 block by the same
              correctly rounded operations: exact inputs, like the observation mean (the check of the device's copies still
              allows them their own roundings: |mu_o|, and sigma_o's by the rule below with E(y) = 0)
  denormalise qd = q' sigma_o + mu_o:  E(qd) = sigma_o E(q') + |q' sigma_o| + |mu_o|
  y           E(y) = (1 - t) gamma (E(qd) + |qd|) + |y|               (the head rule with qd in the place of Q')
  block       the f64 sums of float32 y: sum y is off by the rows' independent errors, sqrt(sum E(y)^2); sum y^2 by
              sqrt(sum (2 |y| E(y))^2)
  mu_n        E(mu_n) = sqrt(sum E(y)^2) / count + |mu_n|              (the mean, then the conversion to float32)
  sigma_n     sq = float32(sumsq / count): E(sq) = sqrt(sum (2 |y| E(y))^2) / count + |sq|;  var = sq - mu_n mu_n -- the
              cancellation -- E(var) = E(sq) + 2 |mu_n| E(mu_n) + mu_n^2 + |var|;  sigma = sqrt(max(var, 1e-2)):
              E(sigma_n) = E(var) / (2 sigma_n) + |sigma_n|.  On the floor, when the fp64 variance is below 1e-2 by more than
              C_STAT 2^-24 E(var), sigma_n is float32(0.1) exactly and E(sigma_n) = 0; a case whose variance is within that
              margin of 1e-2 on either side is not admitted (``floor_state`` "near"; the CPU test asserts there is none)
  rescale     W3' = (W3 sigma_o) / sigma_n, two operations: E(W3') = |W3'| (2 + E(sigma_n) / sigma_n)
              b3' = ((b3 sigma_o + mu_o) - mu_n) / sigma_n with t2 = b3 sigma_o + mu_o, t3 = t2 - mu_n:
              E(t3) = (|b3 sigma_o| + |mu_o|) + E(mu_n) + (|t2| + |mu_n|),  E(b3') = E(t3) / sigma_n + |b3'| (E(sigma_n) / sigma_n + 1)
              The rescaled output layer enters the networks with its error (tests/ddpg_cases.py: _net_fwd / _net_bwd):
              E(q) += |a2| E(W3') + E(b3'), and |d| E(W3')^T on the way back through it; l2 adds l2 E(W3') to A_W3.
  yn          yn = (y - mu_n) / sigma_n: the difference and the quotient round once each at their own size (as the observation
              rule): E(yn) = (E(y) + E(mu_n)) / sigma_n + |yn| (E(sigma_n) / sigma_n + 2)
  dq, seed    E(dq) = 2 (E(q) + E(yn) + |e|) / B + |dq|;  seed = -sigma_n / B: E = E(sigma_n) / B + |seed|
  losses      critic against mean(2 |e| E(e) + e^2) + l2 / 2 sum W^2 with E(e) = E(q) + E(yn) + |e| (E(yn) is far above |yn| where
              the statistics cancel, and its square would let a loss on the unnormalised error through); actor against
              mean(E(q_pi) sigma_n + |q_pi| E(sigma_n) + |q_pi sigma_n| + |mu_n|) + E(mu_n)
  moments     unchanged: tests/ddpg_cases.py step1_ratios, with theta0 = the fp64-rescaled W3' / b3' for the critic and the
              interval widened by C_RESC 2^-24 E(W3') / E(b3'); the target critic's soft update starts from its rescaled layer

The device forms (mu_n, sigma_n) from its own f64 sums of its own float32 y, so its float32 scalars may sit one rounding from
the restatement's: E(mu_n) and E(sigma_n) carry that into everything downstream, and no scalar is read back from the kernel.

Constants (fixed on the CPU from the float32 emulation alone, tests/test_popart_grad_cases_cpu.py): r = max |emu32 - fp64| /
(2^-24 E) per group over the emulated cases, constant = 4 max r rounded up.  Two float32 values that differ by one unit in
the last place are up to two roundings apart, so no constant of a quantity that passes through a float32 conversion of an
f64 value (the scalars, and W3' / b3' through them) is below 2.
"""
import zlib
from collections import namedtuple

import numpy as np

from tests import ddpg_cases as D
from tests.ddpg_cases import EPS32, GAMMA, THR, _Ar, _inputs, _l2_terms, _net_bwd, _net_fwd, _shape_and_clip, row_margin

# 4 * max r over the emulated cases, rounded up (tests/test_popart_grad_cases_cpu.py recomputes every one and fails on a smaller literal)
C_GRAD_POP = D.C_GRAD   # gradients: max r 0.802, 4 r = 3.2 <= 4.5 -- the plain learner's constant, unchanged
C_LOSS_POP = D.C_LOSS   # losses: max r 0.349, 4 r = 1.4 <= 6.5 -- likewise
C_Y = 3.0               # |y - y64| <= C_Y 2^-24 E(y): max r 0.723
C_RESC = 3.5            # the rescaled W3' / b3' of both critics: max r 0.780
C_STAT = 2.0            # the four scalars, and the floor margin: max r 0.365, so one unit in the last place decides
MUTANT_MIN = D.MUTANT_MIN
FLOOR32 = np.float32(0.1)

BLOCKS = ("fresh", "floor", "moving", "large")

# name; obs_dim; actor / critic (h1, h2); batch; last_layer_tanh; block: the starting return block (BLOCKS, ``start_block``);
# stats / layer_norm / critic_l2_reg / clip / tau as tests/ddpg_cases.DdpgCase; kernels: what train_on launches per iteration
PopCase = namedtuple("PopCase", "name obs ah ch B llt block stats ln l2 clip tau kernels emulate")


def pop_kernels(stats, l2, clip):
    """Pop-Art has one path -- the multi-workgroup kernels, whatever the shape (agents.train_on -> ssc_ddpg_train_ws_popart ->
    ddpg_train_wide_popart): target pass, renormalise, gradient pass, apply (prepared with critic_l2_reg / clip_norm)"""
    rms = "const double *, " if stats else ""
    prepared = l2 != 0.0 or clip is not None
    return ("ddpg_wide_grad_kernel<%sPopTarget>" % rms, "ddpg_popart_renorm_kernel", "ddpg_wide_grad_kernel<%sPopGrad>" % rms) + \
        (("ddpg_wide_prepare_kernel", "ddpg_wide_apply_kernel<true>") if prepared else ("ddpg_wide_apply_kernel<false>",))


def _p(name, obs, ah, B, llt, block, ch=None, stats=None, ln=False, l2=0.0, clip=None, tau=0.001):
    ah = tuple(ah)
    ch = tuple(ch) if ch is not None else ah
    emulate = B < 4096 and not (B >= 1024 and max(ah + ch) >= 200)
    return PopCase(name, obs, ah, ch, B, bool(llt), block, stats, ln, float(l2), clip, tau, pop_kernels(stats, float(l2), clip), emulate)


CASES = [
    _p("pa_64_32_b64", 2, (64, 32), 64, True, "moving"),                         # the base shape
    _p("pa_b1", 2, (64, 32), 1, True, "floor"),                                  # Var(y) = 0, sigma on the floor, one partial
    _p("pa_b16", 2, (64, 32), 16, False, "fresh"),                               # exactly one workgroup
    _p("pa_b17", 3, (64, 32), 17, True, "moving", tau=0.3),                      # a ragged last workgroup of one row
    _p("pa_b50", 3, (64, 32), 50, True, "floor"),                                # a ragged batch
    _p("pa_37_19_o8_b77", 8, (37, 19), 77, False, "moving"),                      # odd sizes
    _p("pa_128_64_b256_relu", 2, (128, 64), 256, False, "large"),                # relu second layer
    _p("pa_200_100_b256", 3, (200, 100), 256, True, "moving"),                   # the wide shape
    _p("pa_mixed_a128_c200", 2, (128, 64), 128, True, "fresh", ch=(200, 100), tau=0.3),
    _p("pa_mixed_a200_c64", 2, (200, 100), 64, False, "moving", ch=(64, 32)),
    _p("pa_b4096", 2, (64, 32), 4096, True, "large") ,                           # 256 partials: sp[2 * 256] of the renormalise kernel
    _p("pa_ln_64_64_b256", 3, (64, 64), 256, True, "large", ln=True),
    _p("pa_l2", 2, (64, 32), 64, True, "moving", l2=1e-2, tau=0.3),              # the prepared apply pass
    _p("pa_clip_some", 2, (128, 64), 64, True, "moving", clip="some"),
    _p("pa_all_64_64", 3, (64, 64), 256, False, "moving", ln=True, l2=1e-2, clip="all"),
    # ---- ddpg_wide_grad_kernel<const double *, PopTarget | PopGrad>
    _p("pr_floor_stats", 3, (128, 64), 64, True, "floor", stats="floor"),
    _p("pr_wide_stats", 2, (64, 32), 50, False, "fresh", stats="wide"),
    _p("pr_o8_wide_stats", 8, (37, 19), 77, True, "floor", stats="wide", tau=0.3),
]
CASE_BY_NAME = {c.name: c for c in CASES}
EMULATED = [c for c in CASES if c.emulate]

ROW_MUTANTS = ("drop_last_row", "rows_16_31_twice", "bias_missing_tile", "terminal_ignored", "actor_grad_at_s_a")    # tests/ddpg_cases.py
MUTANTS = ROW_MUTANTS + ("seed_sigma_old", "seed_no_sigma", "y_norm_old_stats", "q_denorm_new_stats", "mu_left_out_of_y",
                         "b3_without_mu_shift", "W3_only", "target_not_rescaled", "last_partial_left_out", "count_16_blocks",
                         "padding_y_summed", "moments_rescaled", "loss_unnormalised")


# ---------------------------------------------------------------------------------------------------------- statistics --
def mean_std32(block):
    """(mu, sigma) of a one-column block as Python floats: obs_rms.mean_std_f32 / the kernels' ret_mean_std restated, one
    float32 rounding per operation, no fma"""
    b, f = np.asarray(block, np.float64), np.float32
    mean, sq = f(b[0] / b[2]), f(b[1] / b[2])
    var = f(sq - f(mean * mean))
    return float(mean), float(f(np.sqrt(np.maximum(var, f(1e-2)))))


def stat_sizes(block, y=None, Ey=None):
    """(E(mu), E(sigma), floor_state, fp64 variance, E(var)) of the statistics of ``block``; y / Ey: the float32 rows (and their
    sizes) whose f64 sums went into it last.  floor_state: "floor" / "off" when the fp64 variance is clear of 1e-2 by more than
    C_STAT 2^-24 E(var), else "near"."""
    b = np.asarray(block, np.float64)
    cnt = b[2]
    mu, sg = mean_std32(b)
    sq = float(np.float32(b[1] / cnt))
    e_sum = e_sumsq = 0.0
    if y is not None:
        e_sum, e_sumsq = float(np.sqrt(np.sum(Ey * Ey))), float(np.sqrt(np.sum((2 * np.abs(y) * Ey) ** 2)))
    E_mu = e_sum / cnt + abs(mu)
    E_var = (e_sumsq / cnt + abs(sq)) + 2 * abs(mu) * E_mu + mu * mu + abs(sq - mu * mu)
    var64 = b[1] / cnt - (b[0] / cnt) ** 2
    margin = C_STAT * EPS32 * E_var
    state = "floor" if var64 < 1e-2 - margin else "off" if var64 > 1e-2 + margin else "near"
    E_sg = 0.0 if state == "floor" else E_var / (2 * sg) + sg
    return E_mu, E_sg, state, var64, E_var


def start_block(kind, rng):
    """the four starting blocks [sum | sumsq | count] (f64):
      fresh   a new RunningMeanStd: (0, 1e-2, 1e-2), mu 0 and sigma 1
      floor   500 returns N(0.02, 0.03): variance 9e-4, sigma on the 0.1 floor
      moving  64 returns 5 N(0, 1) + 3, the first sixth of tests/popart_cases.make_case's "moving" rewards: sigma about 5
      large   10^6 returns of mean 40 and variance 4: |mu| = 20 sigma, sq - mu^2 = 1604 - 1600.  float32 leaves sigma_n a relative
              error of about 800 roundings there (5e-5), and a kernel that takes sigma_o for sigma_n cannot be told from the
              right one unless the batch moves sigma by a multiple of that: the block goes to batches of 256 rows and more,
              whose returns (``rewards``) sit 3 sigma above the block's mean with three times its spread"""
    init = np.array([0.0, 1e-2, 1e-2])
    if kind == "fresh":
        return init
    if kind == "large":
        return init + np.array([40.0 * 1e6, 1604.0 * 1e6, 1e6])
    y0 = (rng.normal(0.02, 0.03, 500) if kind == "floor" else 5 * rng.normal(size=64) + 3).astype(np.float32).astype(np.float64)
    return init + np.array([y0.sum(), (y0 * y0).sum(), float(len(y0))])


def rewards(kind, rng, t):
    """rewards of the rows with terminal flags t.  fresh: 0.5 N(0, 1) as the plain table; floor: 0.02 N(0, 1) (Var(y) stays under the floor); moving: 4 (5 N(0, 1) + 3), the
    third sixth of the "moving" rewards (the batch moves sigma by far more than 10 %); large: N(6.4, 6^2), so that y is about
    mu_o + (3 +- 3) sigma_o: (y - mu) / sigma cancels (|y| + |mu| is about 86, the difference about 6) -- N(46, 6^2) on the
    terminal rows, whose y is r alone and would otherwise pull the batch mean back to the block's"""
    z = rng.normal(size=len(t))
    return {"fresh": 0.5 * z, "floor": 0.02 * z, "moving": 4 * (5 * z + 3), "large": np.where(t, 46.0, 6.4) + 6 * z}[kind].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- generator --
_DATA = {}


def case_data(case):
    """tests/ddpg_cases.case_data for a Pop-Art case: the same dict (3 B candidate rows, the batch built from rows that pass
    the margin -- the rescaling touches the output layer only, so the margins of the critic are those of the rescaled critic --
    clip_norm from the case's own fp64 norms) plus ret_block, the case's starting block.  The floor cases scale both critics'
    output layers by 0.1 (tests/popart_cases.make_case: Var(q') alone passes the floor otherwise)."""
    if case.name in _DATA:
        return _DATA[case.name]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    B, obs, f = case.B, case.obs, np.float32
    actor = D.make_net(rng, obs, case.ah[0], case.ah[1], 1, 0, case.ln)
    critic = D.make_net(rng, obs, case.ch[0], case.ch[1], 1, 1, case.ln)
    target_actor = {k: (v + f(0.01)).astype(f) for k, v in actor.items()}
    target_critic = {k: (v - f(0.01)).astype(f) for k, v in critic.items()}
    if case.block == "floor":
        for p in (critic, target_critic):
            p["W3"], p["b3"] = (p["W3"] * f(0.1)).astype(f), (p["b3"] * f(0.1)).astype(f)
    n = max(3 * B, 48)
    block = mean = std = None
    if case.stats:
        block, mean, std, (lo, hi) = D.edge_stats(obs, case.stats)
        s = rng.uniform(lo, hi, (n, obs)).astype(f)
    else:
        s = rng.uniform(-1.2, 0.6, (n, obs)).astype(f)
        if obs == 3:
            s[:, 2] = rng.uniform(-8, 8, n)
    a = rng.uniform(-1, 1, (n, 1)).astype(f)
    t = (rng.random(n) < 0.1).astype(np.uint8)
    r = rewards(case.block, rng, t)
    s2 = (s + 0.01 * rng.normal(size=(n, obs))).astype(f)
    d = dict(actor=actor, critic=critic, target_actor=target_actor, target_critic=target_critic, s=s, a=a, r=r, t=t, s2=s2,
             block=block, mean=mean, std=std, clip_norm=None, llt=case.llt, l2=case.l2, B=B, ret_block=start_block(case.block, rng),
             tau=case.tau)
    good = np.nonzero(row_margin(d) >= THR)[0]
    assert good.size >= B, (case.name, good.size, n)
    d["good_share"] = good.size / n
    d["idx"] = rng.permutation(good)[:B].astype(np.int32)[None]
    ref = popart_step1(d)
    d["norms"] = ref["norms"]
    if case.clip:
        norms = np.sort(np.array([v for net in ("actor", "critic") for v in ref["norms"][net].values()]))
        if case.clip == "all":
            c = 0.5 * norms[0]
        elif case.clip == "none":
            c = 2.0 * norms[-1]
        else:
            k = 1 + int(np.argmax(norms[2:-1] / norms[1:-2]))
            c = np.sqrt(norms[k] * norms[k + 1])
        d["clip_norm"] = float(f(c))
    for v in d.values():
        for arr in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
    _DATA[case.name] = d
    return d


# ------------------------------------------------------------------------------------- the iteration, fp64 or float32 --
def _rescale(ar, p, mu_o, sg_o, mu_n, sg_n, E_mu_n, E_sg_n, mut=None):
    """step 3 on one critic in the pass's arithmetic, the device's operation order; with sizes: E_W3 / E_b3 beside them"""
    T = ar.t
    q = dict(p)
    if mut == "not_rescaled":
        return q
    q["W3"] = (p["W3"] * T(sg_o)) / T(sg_n)
    if mut == "b3_without_mu_shift":
        q["b3"] = (p["b3"] * T(sg_o)) / T(sg_n)
    elif mut != "W3_only":
        t1 = p["b3"] * T(sg_o)
        t2 = t1 + T(mu_o)
        q["b3"] = (t2 - T(mu_n)) / T(sg_n)
        if ar.sizes:
            E_t3 = (np.abs(t1) + abs(mu_o)) + E_mu_n + (np.abs(t2) + abs(mu_n))
            q["E_b3"] = E_t3 / sg_n + np.abs(q["b3"]) * (E_sg_n / sg_n + 1)
    if ar.sizes:
        q["E_W3"] = np.abs(q["W3"]) * (2 + E_sg_n / sg_n)
    return q


def popart_step1(d, f32=False, mut=None, sizes=True):
    """One Pop-Art iteration on the batch d["idx"][0] from d["ret_block"].  Returns a dict: g, A, loss, A_loss, relu_pre, norms,
    n_bound as tests/ddpg_cases.step; y / E_y [B]; block (the new one); scalars = (mu_o, sigma_o, mu_n, sigma_n) and E_scalars;
    floor_state (of the old and the new statistics), var64; critic / target_critic: the rescaled networks (W3 / b3 rescaled, with
    E_W3 / E_b3 beside them in the fp64 pass).  ``mut``: a wrong kernel -- ROW_MUTANTS as in tests/ddpg_cases.step, and
      seed_sigma_old         the actor's seed -sigma_o / B
      seed_no_sigma          the actor's seed -1 / B
      y_norm_old_stats       (y - mu_o) / sigma_o in the critic's error
      q_denorm_new_stats     q' sigma_n + mu_n in y (the scalars the renormalise launch leaves, read a pass too early)
      mu_left_out_of_y       y = r + (1 - t) gamma q' sigma_o
      b3_without_mu_shift    b3 <- b3 sigma_o / sigma_n
      W3_only                W3 rescaled, b3 not
      target_not_rescaled    the target critic's output layer left as it was
      last_partial_left_out  the last workgroup's (sum y, sum y^2) not added to the block
      count_16_blocks        count += 16 * workgroups
      padding_y_summed       the clamped last row's y summed for the padding rows of the last workgroup
      moments_rescaled       the W3 / b3 gradients (read back from the moments) scaled by sigma_o / sigma_n with the layer
      loss_unnormalised      the critic loss mean((sigma_n e)^2)"""
    assert mut is None or mut in MUTANTS
    ar = _Ar(f32, sizes)
    T, absd = ar.t, ar.sizes
    bi = d["idx"][0]
    B = len(bi)
    nb = (B + 15) // 16
    llt, l2, clip = d["llt"], d["l2"], d["clip_norm"]
    actor, critic0, tactor, tcritic0 = ({k: ar.arr(v) for k, v in d[n].items()} for n in ("actor", "critic", "target_actor", "target_critic"))
    s, Es = _inputs(ar, d, d["s"][bi], None)
    s2, Es2 = _inputs(ar, d, d["s2"][bi], None)
    a, r = ar.arr(d["a"][bi]), ar.arr(d["r"][bi]).reshape(B, 1)
    t = ar.arr(d["t"][bi]).reshape(B, 1)
    rows = np.arange(B)
    if mut == "drop_last_row":
        rows = rows[:-1]
    elif mut == "rows_16_31_twice":
        rows = np.concatenate([rows, rows[16:32]])
    brows = rows[rows >= 16] if mut == "bias_missing_tile" else rows
    zero = np.zeros((B, 1)) if absd else None
    block = np.asarray(d["ret_block"], np.float64)
    mu_o, sg_o = mean_std32(block)
    # 1: y = r + (1 - terminal) gamma (q' sigma_o + mu_o)
    pi1, Epi1, _ = _net_fwd(ar, tactor, s2, Es2, llt)
    q1, Eq1, _ = _net_fwd(ar, tcritic0, s2, Es2, llt, pi1, Epi1)
    dmu, dsg = popart_step1(d, f32, None, False)["scalars"][2:] if mut == "q_denorm_new_stats" else (mu_o, sg_o)
    qs = q1 * T(dsg)
    qd = qs if mut == "mu_left_out_of_y" else qs + T(dmu)
    live = T(1) if mut == "terminal_ignored" else (T(1) - t)
    y = r + live * T(GAMMA) * qd
    Ya = None
    if absd:
        Ya = (1.0 - t) * GAMMA * ((sg_o * Eq1 + np.abs(qs) + abs(mu_o)) + np.abs(qd)) + np.abs(y)
    # 2: the block in f64 on the float32 y, then the new statistics
    y64 = np.asarray(y, np.float64).reshape(-1)
    ys = y64
    if mut == "last_partial_left_out":
        ys = y64[:16 * (nb - 1)]
    elif mut == "padding_y_summed":
        ys = np.concatenate([y64, np.full(16 * nb - B, y64[-1])])
    block_n = block + np.array([ys.sum(), (ys * ys).sum(), float(16 * nb if mut == "count_16_blocks" else B)])
    mu_n, sg_n = mean_std32(block_n)
    E_sc = states = var64 = None
    E_mu_n = E_sg_n = 0.0
    if absd:
        E_mu_o, E_sg_o, st_o, _, _ = stat_sizes(block)
        E_mu_n, E_sg_n, st_n, var64, _ = stat_sizes(block_n, y64, Ya.reshape(-1))
        E_sc, states = (E_mu_o, E_sg_o, E_mu_n, E_sg_n), (st_o, st_n)
    # 3: both output layers
    critic = _rescale(ar, critic0, mu_o, sg_o, mu_n, sg_n, E_mu_n, E_sg_n, mut)
    tcritic = _rescale(ar, tcritic0, mu_o, sg_o, mu_n, sg_n, E_mu_n, E_sg_n, "not_rescaled" if mut == "target_not_rescaled" else mut)
    # 4: the critic on the normalised target
    nmu, nsg = (mu_o, sg_o) if mut == "y_norm_old_stats" else (mu_n, sg_n)
    yn = (y - T(nmu)) / T(nsg)
    q, Qa, cc = _net_fwd(ar, critic, s, Es, llt, a, zero)
    e = q - yn
    el = e * T(sg_n) if mut == "loss_unnormalised" else e
    loss_c = ar.colsum(el * el)[0] / T(B)
    dq = e * (T(2) / T(B))
    Edq = A_lc = None
    if absd:
        Eyn = (Ya + E_mu_n) / sg_n + np.abs(yn) * (E_sg_n / sg_n + 2)
        Edq = 2.0 * (Qa + Eyn + np.abs(e)) / B + np.abs(dq)
        A_lc = float(np.mean(2 * np.abs(e) * (Qa + Eyn + np.abs(e)) + e * e))
    gc, Ac, _, _ = _net_bwd(ar, critic, cc, dq, Edq, llt, True, None, rows, brows, False)
    loss_c, A_lc = _l2_terms(ar, critic, gc, Ac, loss_c, A_lc, l2, None)
    # the actor through the rescaled critic, seed -sigma_n / B (the device's -sigma_n * (1 / B))
    pi, Epi, ac = _net_fwd(ar, actor, s, Es, llt)
    qpi, Qpia, cc2 = _net_fwd(ar, critic, s, Es, llt, pi, Epi)
    loss_a = -(ar.colsum(qpi * T(sg_n) + T(mu_n))[0] / T(B))
    ssg = {"seed_sigma_old": sg_o, "seed_no_sigma": 1.0}.get(mut, sg_n)
    seed = np.full((B, 1), -(T(ssg) * (T(1) / T(B))), T)
    A_la = None
    if absd:
        A_la = float(np.mean(Qpia * sg_n + np.abs(qpi) * E_sg_n + np.abs(qpi * sg_n) + abs(mu_n))) + E_mu_n
    _, _, dact, Edact = _net_bwd(ar, critic, cc if mut == "actor_grad_at_s_a" else cc2, seed, E_sg_n / B + np.abs(seed) if absd else None,
                                 llt, False, None, rows, brows, False)
    ga, Aa, _, _ = _net_bwd(ar, actor, ac, dact, Edact, llt, True, None, rows, brows, True)
    ga, gc, Aa, Ac, norms, n_bound = _shape_and_clip(ar, actor, critic, ga, gc, Aa, Ac, clip, None)
    if mut == "moments_rescaled":
        for k in ("W3", "b3"):
            gc[k] = gc[k] * (T(sg_o) / T(sg_n))
    return dict(g=dict(actor=ga, critic=gc), A=dict(actor=Aa, critic=Ac) if absd else None, loss=(loss_c, loss_a),
                A_loss=(A_lc, A_la) if absd else None, relu_pre=ac["relu_pre"] + cc["relu_pre"] + cc2["relu_pre"], norms=norms,
                n_bound=n_bound, y=y.reshape(-1), E_y=Ya.reshape(-1) if absd else None, block=block_n,
                scalars=(mu_o, sg_o, mu_n, sg_n), E_scalars=E_sc, floor_state=states, var64=var64, critic=critic, target_critic=tcritic)


_REF = {}


def reference(case):
    """the fp64 iteration of the case with its sizes; computed once, never modified"""
    if case.name not in _REF:
        ref = popart_step1(case_data(case))
        for x in [v for net in ("actor", "critic") for part in ("g", "A") for v in ref[part][net].values()] + \
                [v for net in ("critic", "target_critic") for v in ref[net].values()] + [ref["y"], ref["E_y"], ref["block"]]:
            x.setflags(write=False)
        _REF[case.name] = ref
    return _REF[case.name]


# -------------------------------------------------------------------------------------------------------------- checks --
def raw_ratios(ref, x):
    """err / (2^-24 E) of an iteration ``x`` against the fp64 reference, per group, WITHOUT the constants (units of r_case):
    dict(grad, loss_c, loss_a, y, resc, stat)"""
    lc, la = D.loss_ratios(ref, x["loss"])
    resc = max(D.ratio(np.abs(np.asarray(x[net][k], np.float64) - ref[net][k]), EPS32 * ref[net]["E_" + k])
               for net in ("critic", "target_critic") for k in ("W3", "b3"))
    stat = D.ratio(np.abs(np.array(x["scalars"]) - np.array(ref["scalars"])), EPS32 * np.array(ref["E_scalars"]))
    return dict(grad=D.grad_ratio(ref, x["g"]), loss_c=lc, loss_a=la, resc=resc, stat=stat,
                y=D.ratio(np.abs(np.asarray(x["y"], np.float64) - ref["y"]), EPS32 * ref["E_y"]))


def as_device(d, x):
    """what the learner would leave after the iteration ``x`` (a popart_step1 result, fp64 or float32) and the Adam step of
    tests/ddpg_cases.py on it, in the arithmetic of x: the dict ``checks`` takes"""
    f32 = x["y"].dtype == np.float32
    tau = float(np.float32(d["tau"]))
    out = dict(loss=np.array([float(v) for v in x["loss"]]), y=x["y"], block=x["block"], scalars=np.array(x["scalars"]), adam_t=[1, 1])
    for net, theta0, target0 in (("actor", d["actor"], d["target_actor"]), ("critic", x["critic"], x["target_critic"])):
        o = dict(theta={}, target={}, m={}, v={})
        for k in D.keys_of(d[net]):
            g = x["g"][net][k]
            if f32:
                f = np.float32
                o["m"][k], o["v"][k], o["theta"][k] = D.adam1_32(theta0[k], g)
                o["target"][k] = (f(1) - f(d["tau"])) * np.asarray(target0[k], f) + f(d["tau"]) * o["theta"][k]
            else:
                th0 = np.asarray(theta0[k], np.float64)
                o["m"][k], o["v"][k], o["theta"][k] = D.C1 * g, D.C2 * g * g, th0 - D._u(g)
                o["target"][k] = (1.0 - tau) * np.asarray(target0[k], np.float64) + tau * o["theta"][k]
        out[net] = o
    return out


def checks(d, ref, got):
    """Every bound the GPU test holds the device to, as err / allowed (<= 1 accepted), from ``got`` = dict(actor / critic =
    dict(theta, target, m, v: dicts by key), loss [2], y [B], block [3], scalars [4]): dict(m, v, theta, target (the largest
    over all parameters; ``where`` names them), loss_c, loss_a, y, sum, sumsq, count, stat).  The critic's theta0 / target0 are
    the fp64-rescaled networks of ref, W3 / b3 with their C_RESC 2^-24 E."""
    out, where = dict(m=0.0, v=0.0, theta=0.0, target=0.0), {}
    for net, theta0, target0 in (("actor", d["actor"], d["target_actor"]), ("critic", ref["critic"], ref["target_critic"])):
        for k in D.keys_of(d[net]):
            e0 = C_RESC * EPS32 * theta0["E_" + k] if "E_" + k in theta0 else 0.0
            e1 = C_RESC * EPS32 * target0["E_" + k] if "E_" + k in target0 else 0.0
            r = D.step1_ratios(theta0[k], ref["g"][net][k], ref["A"][net][k], got[net]["m"][k], got[net]["v"][k], got[net]["theta"][k],
                               c_grad=C_GRAD_POP, theta0_err=e0)
            r += (D.target_ratio(target0[k], got[net]["theta"][k], got[net]["target"][k], d["tau"], target0_err=e1),)
            for name, v in zip(("m", "v", "theta", "target"), r):
                if v > out[name]:
                    out[name], where[name] = v, net + "." + k
    lc, la = D.loss_ratios(ref, got["loss"])
    out["loss_c"], out["loss_a"] = lc / C_LOSS_POP, la / C_LOSS_POP
    y, Ey = ref["y"], ref["E_y"]
    dy = C_Y * EPS32 * Ey
    out["y"] = D.ratio(np.abs(np.asarray(got["y"], np.float64) - y), dy)
    # sum / sumsq: every row's y within its bound (the f64 additions themselves: 2^-50 of the terms)
    blk, rb = np.asarray(got["block"], np.float64), ref["block"]
    out["sum"] = abs(blk[0] - rb[0]) / (np.sum(dy) + 2.0 ** -50 * (abs(rb[0]) + np.sum(np.abs(y))))
    out["sumsq"] = abs(blk[1] - rb[1]) / (np.sum(2 * np.abs(y) * dy + dy * dy) + 2.0 ** -50 * rb[1])
    out["count"] = 0.0 if blk[2] == rb[2] else np.inf
    out["stat"] = D.ratio(np.abs(np.asarray(got["scalars"], np.float64) - np.array(ref["scalars"])), C_STAT * EPS32 * np.array(ref["E_scalars"]))
    out["where"] = where
    return out


GROUPS = ("m", "v", "theta", "target", "loss_c", "loss_a", "y", "sum", "sumsq", "count", "stat")


def worst(ch):
    """(largest err / allowed, its group)"""
    return max((ch[k], k) for k in GROUPS)


def partial_sums(y):
    """the target pass's per-workgroup (sum y, sum y^2) in f64 of float32 y, in the order of its xor butterfly over 16 lanes
    (8, 4, 2, 1): [ceil(B / 16), 2]; rows past the batch add zero"""
    y = np.asarray(y, np.float32).astype(np.float64)
    nb = (len(y) + 15) // 16
    p = np.zeros((nb * 16, 2))
    p[:len(y), 0], p[:len(y), 1] = y, y * y
    p = p.reshape(nb, 16, 2)
    for m in (8, 4, 2, 1):
        p = p[:, :m] + p[:, m:2 * m]
    return p[:, 0]
