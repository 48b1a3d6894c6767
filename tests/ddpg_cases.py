"""Case matrix of the DDPG learner (csrc/ddpg_train_fixed.hip, ddpg_train.hip, ddpg_train_wide.hip): the case table with
the kernels each case launches, each case's inputs, the fp64 gradients of one iteration with the size of the terms they
are made of, a float32 emulation of the iteration, the bound derived from the two, and the mutants that bound must reject.
Shared by the CPU test (tests/test_ddpg_cases_cpu.py) and the GPU test (tests/test_gpu_ddpg_matrix.py); numpy + oracle only.

Why gradients.  Adam is scale-invariant: from zero moments the first step is lr * sign(g) whatever |g| is, so a gradient
wrong in size (a batch row dropped, a 16-row tile missing from a bias sum) leaves the parameters where the oracle puts
them.  It shows in the moments only: after ONE iteration from zero moments m = c1 g and v = c2 g^2, and that is where the
device gradient is read back from.

The bound.  ``step(data)`` is the algebra of O.ddpg_train_step in fp64 on the float32 inputs the kernel receives (with
statistics: on clip((x - mean) / std, -5, 5) formed in fp64 from the fp32 mean / std); ``step(data, f32=True)`` is the same
iteration in float32 numpy, one rounding per operation (no fma), every sum strictly in index order, tanh by the kernels'
tanh_fast formula 1 - 2 / (2^(2 x log2 e) + 1).  Beside every fp64 value v the pass carries E(v) >= 0, the size of v's
float32 error in units of one rounding; A is E of a gradient element.  Values and error sizes are carried apart: a pass on
absolute values alone counts |xhat| <= rstd (|z| + mean |z|) at every LayerNorm and the forward sizes again in every
derivative, and leaves whole mutants inside the bound.  Two conventions hold throughout.  A sum of terms rounds ONCE, at
the size of its terms, whatever its length.  Errors that different units bring into a sum are independent roundings and
add like their root sum of squares.  With |.| elementwise:

  inputs    E(x) = 0; with statistics E(x_hat) = 2 |x_hat| (x and mean are exact float32: the kernel's difference and
            quotient round once each, at their own size); the clip passes E on
  dense     z = h W + b:  E(z) = sqrt(E(h)^2 W^2) + |h| |W| + |b|
  relu      E(u) = E(z) * mask (the fp64 mask)
  tanh      E(u) = (1 - u^2) E(z) + 2      (tanh_fast's own error is absolute: 1 - 2 / (..) loses it at size 1)
  LayerNorm ONE operation, xhat = (z - mean) rstd: the projection off (1, xhat) does not enlarge the error vector of z, a
            unit gets its own E(z) and its share sqrt(mean E(z)^2 / n) (1 + |xhat|) of the two common components, and the
            operation's own error counts once, at |xhat|:  E(xhat) = rstd (E(z) + share) + |xhat|;  rstd carries the relative
            size rho = sqrt(mean (xhat E(xhat))^2 / n);  n = xhat gamma + beta:  E(n) = E(xhat) |gamma| + |n|
  head      y = r + (1 - t) gamma Q'(s2) through the target networks: E(y) = (1 - t) gamma (E(Q') + |Q'|) + |y|
            dq = 2 (q - y) / B:  E(dq) = 2 (E(q) + E(y) + |q - y|) / B + |dq|
  backward  through W: sqrt(E(d)^2 (W^2)^T) + |d| |W|^T;  relu: * mask;  tanh: d' = d (1 - u^2), E(d') = E(d) (1 - u^2) +
            |d| (2 |u| E(u) + 1) + |d'| (the derivative, and what the forward error does to it), the actor's output alike
            LayerNorm, the same projection once: dz = rstd (dxh - mean dxh - xhat mean(dxh xhat)), dxh = d gamma,
            E(dz) = rstd (E(dxh) + share) + E(xhat) |mean(dxh xhat)| + |xhat| sqrt(mean (dxh E(xhat))^2 / n) + |dz| (rho + 1)
            A_gamma = sum_rows (E(d) |xhat| + |d| E(xhat) + |d xhat|),  A_beta = sum_rows (E(d) + |d|)
            g_W = h^T d:  A_W = E(h)^T |d| + |h|^T E(d) + R(h, d),  A_b = sum_rows E(d) + R(1, d), where R is the rounding of
            the batch sum itself: one rounding per partial sum s_k, independent, R = sqrt(sum_k s_k^2).  For terms that
            cancel that is about sum |terms|; for terms of one sign (a relu input times a delta, a bias delta) the partial
            sums of an in-order accumulation grow with k, and what they round off with them
            the actor's d starts from the critic's action-column d at (s, pi(s)) with seed -1 / B, and E(pi) enters the
            critic's second layer there
  options   critic_l2_reg: A_W += l2 |W| + |g|;  clip_norm on a variable it binds: g' = g s, s = clip / norm,
            A' = s A + |g'| (sum(|g| A) / norm^2 + 3) (the second term is the scale factor's own error); a variable it
            does not bind keeps its A

r_case = max |emu32 - g64| / (2^-24 A) is what float32 costs at a case, in units of one rounding of A.  A device gradient
g is accepted when |g - g64| <= C_GRAD * 2^-24 * A, for every element of every parameter (where A = 0 the gradient must be
exactly g64), with C_GRAD = 4 * max_cases r_case: the factor 4 is for fma contraction, the MFMA's internal order and the
tile / wave / workgroup partial sums.  With Qa = E(q) and Ya = E(y) (both at least the values' own size) the critic loss is
held to C_LOSS 2^-24 (mean((Qa + Ya)^2) + l2 / 2 sum W^2), the actor loss to C_LOSS 2^-24 mean(Qa(s, pi(s))).  Both
constants are fixed here, without the kernel.

Stability.  relu derivatives are the only discontinuity of the gradient (forward-only evaluations, the target networks,
the observation clip and max(norm, clip) are continuous).  The generator draws 3 B candidate rows and builds the batch
only from rows whose relu pre-activations -- actor at s, critic at (s, a), critic at (s, pi(s)) -- are all at least THR
from zero in fp64; after that no element is left out of any assertion.

Cases with batch 4096, and 200-100 at batch 1024, are kept out of the sequential emulation and of the constants (the
emulation's python loops run over the batch and the layer widths); their bound uses the constants of the other cases.
Mutants are applied to the fp64 algebra at all cases, these included, and must be MUTANT_MIN = 2.25 bounds out; at the
emulated cases they are applied to the float32 emulation as well and must be 2 bounds out.
"""
import zlib
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -24
THR = 1e-4              # smallest |relu pre-activation| a row of the bounded batch may have
C_GRAD = 4.5            # 4 * max r_case over the emulated cases, rounded up (tests/test_ddpg_cases_cpu.py recomputes it)
C_LOSS = 6.5            # the same for the two losses
MUTANT_MIN = 2.25       # bounds (C_GRAD included) the nearest fp64-stated mutant must be away
LR, BETA1, BETA2, EPSILON, GAMMA, OBS_CLIP = 1e-3, 0.9, 0.999, 1e-8, 0.99, 5.0
TAUS = (0.001, 0.3)

# the kernels' own float32 coefficients evaluated in fp64
C1 = float(np.float32(1.0) - np.float32(BETA1))
C2 = float(np.float32(1.0) - np.float32(BETA2))
# the bias-corrected step size of step 1 as adam_cfg computes it: in double from the float32 arguments, rounded to float32
LR1 = float(np.float32(float(np.float32(LR)) * np.sqrt(1.0 - float(np.float32(BETA2))) / (1.0 - float(np.float32(BETA1)))))

KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
LN_KEYS = ("W1", "b1", "ln1_b", "ln1_g", "W2", "b2", "ln2_b", "ln2_g", "W3", "b3")

# ---------------------------------------------------------------------------------------------------------- dispatch --
FIXED, FIXED_TILED, INTERPRETER, WIDE, NEEDS_WORKSPACE = range(5)        # ssc_ddpg_learner_path's answers
PATH_NAME = ("fixed", "fixed_tiled", "interpreter", "wide")
KB, KP = 64, 68
INTERP_LDS_FLOATS = (160 * 1024 - 128) // 4


def _net_total(i, h1, h2, out, extra, ln):
    return i * h1 + h1 + (2 * h1 if ln else 0) + (h1 + extra) * h2 + h2 + (2 * h2 if ln else 0) + h2 * out + out


def interp_carve_floats(obs, ah, ch, act=1):
    """the step interpreter's LDS carve (csrc/ddpg_layout.h: ddpg_interp_carve), in floats"""
    rows = (obs + 4 + (ch[0] + act) + max(ch[1], obs) + 1 + ch[1] + (ch[0] + act) + ah[0] + ah[1] + act + act + ah[0]
            + max(ch[1], ah[1]) + ch[1])
    p = rows * KP
    nA, nC = _net_total(obs, ah[0], ah[1], act, 0, False), _net_total(obs, ch[0], ch[1], 1, act, False)
    al4 = lambda x: (x + 3) & ~3
    ta = al4(p); tc = al4(ta + nA); tta = al4(tc + nC); ttc = al4(tta + nA)
    return ttc + nC


def learner_path(obs, ah, ch, B, ln, l2, clip, have_rms, want_interp, want_wide):
    """csrc/ddpg_layout.h: ddpg_learner_path restated for a call with a workspace (train_on always brings one)"""
    fixed_nets = obs in (2, 3) and tuple(ah) == (64, 32) and tuple(ch) == (64, 32)
    narrow = not ln and l2 == 0.0 and not clip and B == KB and max(ah + ch) <= 64
    if not want_wide and not want_interp and fixed_nets and not ln and B > KB and B % KB == 0 and B <= 4096:
        return FIXED_TILED
    if not narrow or want_wide:
        return WIDE
    if fixed_nets and not want_interp:
        return FIXED
    if have_rms:
        return WIDE
    if interp_carve_floats(obs, ah, ch) > INTERP_LDS_FLOATS:
        return WIDE
    return INTERPRETER


# name; obs_dim; actor / critic (h1, h2); batch; last_layer_tanh; stats: None | "floor" | "wide" (tests/gpu_util.rms_edge_stats);
# layer_norm; critic_l2_reg; clip: None | "all" | "some" | "none" (which variables the threshold binds; the value is chosen
# from the case's own fp64 norms, case_data); env: None | the switch set to 1; tau; path / kernels: what train_on launches
# (read off ddpg_learner_path and the launch code); emulate: part of the sequential float32 emulation
DdpgCase = namedtuple("DdpgCase", "name obs ah ch B llt stats ln l2 clip env tau path kernels emulate")


def _c(name, obs, ah, B, llt, ch=None, stats=None, ln=False, l2=0.0, clip=None, env=None, tau=0.001):
    ah = tuple(ah)
    ch = tuple(ch) if ch is not None else ah
    path = learner_path(obs, ah, ch, B, ln, l2, clip, stats is not None, env == "SSC_DDPG_INTERPRETER", env == "SSC_DDPG_WIDE")
    rms = "const double *" if stats else ""
    prepared = l2 != 0.0 or clip is not None
    apply_ = (("ddpg_wide_prepare_kernel", "ddpg_wide_apply_kernel<true>") if prepared else ("ddpg_wide_apply_kernel<false>",))
    if path in (FIXED, FIXED_TILED):
        k = "ddpg_train_fixed_kernel<%d, %s, %s%s>" % (obs, "true" if llt else "false", "true" if path == FIXED_TILED else "false",
                                                       ", " + rms if rms else "")
        kernels = (k,) + (apply_ if path == FIXED_TILED else ())
    elif path == INTERPRETER:
        kernels = ("ddpg_train_kernel",)
    else:
        kernels = ("ddpg_wide_grad_kernel<%s>" % rms,) + apply_
    emulate = B < 4096 and not (B >= 1024 and max(ah + ch) >= 200)
    return DdpgCase(name, obs, ah, ch, B, bool(llt), stats, ln, float(l2), clip, env, tau, path, kernels, emulate)


I_, W_ = "SSC_DDPG_INTERPRETER", "SSC_DDPG_WIDE"
CASES = [
    # ---- ddpg_train_fixed_kernel<O, TANH2, false, Rms...>: 64-32 at batch 64
    _c("fx_o2_tanh", 2, (64, 32), 64, True), _c("fx_o2_tanh_floor", 2, (64, 32), 64, True, stats="floor"),
    _c("fx_o2_relu", 2, (64, 32), 64, False, tau=0.3), _c("fx_o2_relu_wide", 2, (64, 32), 64, False, stats="wide"),
    _c("fx_o3_tanh", 3, (64, 32), 64, True), _c("fx_o3_tanh_wide", 3, (64, 32), 64, True, stats="wide", tau=0.3),
    _c("fx_o3_relu", 3, (64, 32), 64, False), _c("fx_o3_relu_floor", 3, (64, 32), 64, False, stats="floor"),
    # ---- ddpg_train_fixed_kernel<O, TANH2, true, Rms...> per 64-row tile, then the apply pass over 2 .. 64 partials
    _c("ft_o2_tanh_b128", 2, (64, 32), 128, True), _c("ft_o2_tanh_wide_b1024", 2, (64, 32), 1024, True, stats="wide"),
    _c("ft_o2_relu_b1024", 2, (64, 32), 1024, False), _c("ft_o2_relu_floor_b128", 2, (64, 32), 128, False, stats="floor"),
    _c("ft_o3_tanh_b4096", 3, (64, 32), 4096, True), _c("ft_o3_tanh_floor_b4096", 3, (64, 32), 4096, True, stats="floor"),
    _c("ft_o3_relu_b128", 3, (64, 32), 128, False, tau=0.3), _c("ft_o3_relu_wide_b1024", 3, (64, 32), 1024, False, stats="wide"),
    _c("ft_o3_relu_b1024", 3, (64, 32), 1024, False), _c("ft_o3_relu_b4096", 3, (64, 32), 4096, False),
    _c("ft_o2_tanh_b256_l2_clip", 2, (64, 32), 256, True, l2=1e-2, clip="some"),     # the prepared apply pass behind the tiles
    # ---- the step interpreter ddpg_train_kernel
    _c("in_24_20", 2, (24, 20), 64, True), _c("in_o8_64_32", 8, (64, 32), 64, False),
    _c("in_forced_o2", 2, (64, 32), 64, True, env=I_, tau=0.3), _c("in_forced_o3", 3, (64, 32), 64, False, env=I_),
    _c("in_actor_narrower", 2, (24, 20), 64, False, ch=(48, 24)),
    # ---- ddpg_wide_grad_kernel<> + ddpg_wide_apply_kernel<false>
    _c("wd_128_64_b64", 2, (128, 64), 64, True), _c("wd_128_64_b256", 2, (128, 64), 256, False),
    _c("wd_200_100_b64", 2, (200, 100), 64, False, tau=0.3), _c("wd_200_100_o3_b256", 3, (200, 100), 256, True),
    _c("wd_200_100_o3_b1024", 3, (200, 100), 1024, True),
    _c("wd_mixed_a128_c200", 2, (128, 64), 128, True, ch=(200, 100)), _c("wd_mixed_a200_c64", 2, (200, 100), 64, False, ch=(64, 32)),
    _c("wd_ragged_b50", 3, (64, 32), 50, True), _c("wd_37_19_o8_b77", 8, (37, 19), 77, False),
    _c("wd_b16", 2, (64, 32), 16, True), _c("wd_b17", 2, (64, 32), 17, False), _c("wd_b32", 2, (64, 32), 32, True),
    _c("wd_128_64_b4096", 2, (128, 64), 4096, True),
    _c("wd_forced_b64", 2, (64, 32), 64, True, env=W_), _c("wd_forced_o3_b1024", 3, (64, 32), 1024, False, env=W_),
    # ---- ddpg_wide_grad_kernel<const double *>: the shapes statistics re-route there, and wide shapes with statistics
    _c("wr_24_20", 2, (24, 20), 64, True, stats="wide"), _c("wr_o8_64_32", 8, (64, 32), 64, False, stats="floor"),
    _c("wr_forced_interp", 2, (64, 32), 64, True, stats="floor", env=I_),
    _c("wr_forced_wide_b1024", 2, (64, 32), 1024, True, stats="wide", env=W_),
    _c("wr_200_100_o3_b256", 3, (200, 100), 256, False, stats="floor"), _c("wr_37_19_o8_b77", 8, (37, 19), 77, True, stats="wide", tau=0.3),
    # ---- LayerNorm
    _c("ln_64_64_o3_b256", 3, (64, 64), 256, True, ln=True), _c("ln_128_64_o3_b64", 3, (128, 64), 64, False, ln=True),
    _c("ln_37_19_o8_b77_floor", 8, (37, 19), 77, True, ln=True, stats="floor"),
    # ---- ddpg_wide_prepare_kernel + ddpg_wide_apply_kernel<true>: critic_l2_reg alone, clip_norm alone, all three
    _c("op_l2", 2, (64, 32), 64, True, l2=1e-2, tau=0.3),
    _c("op_clip_all", 2, (64, 32), 64, False, clip="all"), _c("op_clip_some", 2, (128, 64), 64, True, clip="some"),
    _c("op_clip_none", 3, (64, 32), 50, True, clip="none"),
    _c("op_all_37_19", 8, (37, 19), 77, True, ln=True, l2=0.3, clip="some"),
    _c("op_all_64_64_wide", 3, (64, 64), 256, False, ln=True, l2=1e-2, clip="all", stats="wide"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
EMULATED = [c for c in CASES if c.emulate]

MUTANTS = ("drop_last_row", "rows_16_31_twice", "bias_missing_tile", "dq_1_over_B", "terminal_ignored", "y_from_critic",
           "actor_grad_at_s_a", "action_row_before", "no_output_tanh_derivative", "no_layer1_mask", "drop_last_unit_h1",
           "drop_last_unit_h2", "l2_on_biases", "clip_global_norm", "neighbour_mean", "no_obs_clip")


# ---------------------------------------------------------------------------------------------------------- generator --
RMS_EDGE_MEAN = np.array([0.2, -0.1, 0.5, -0.4, 0.3, -0.25, 0.15, -0.35])       # tests/gpu_util.rms_edge_stats, restated
RMS_EDGE_STD = np.array([0.5, 0.25, 2.0, 0.4, 0.8, 0.3, 1.2, 0.6])


def edge_stats(obs_dim, kind, seed=21):
    """The floor / wide statistics sets of tests/gpu_util.rms_edge_stats without the device: (block, mean, std, (low, high)),
    block = the f64 RunningMeanStd vector [sum | sumsq | count] after one update with the same rows, mean / std = the fp32
    values the kernels derive from it (obs_rms.mean_std_f32 restated: one float32 rounding per operation)."""
    mean = RMS_EDGE_MEAN[:obs_dim]
    rng = np.random.default_rng(seed + obs_dim)
    if kind == "floor":
        rows, half = rng.normal(mean, 0.02, size=(500, obs_dim)), 0.5 / 0.95
    else:
        rows, half = rng.normal(mean, RMS_EDGE_STD[:obs_dim], size=(400, obs_dim)), 3 * RMS_EDGE_STD[:obs_dim]
    rows = rows.astype(np.float32).astype(np.float64)
    block = np.concatenate([rows.sum(0), 1e-2 + (rows * rows).sum(0), [1e-2 + len(rows)]])
    m32 = (block[:obs_dim] / block[-1]).astype(np.float32)
    sq = (block[obs_dim:2 * obs_dim] / block[-1]).astype(np.float32)
    s32 = np.sqrt(np.maximum(sq - m32 * m32, np.float32(1e-2))).astype(np.float32)
    return block, m32, s32, (mean - half, mean + half)


def _glorot(rng, i, o):
    lim = np.sqrt(6.0 / (i + o))
    return rng.uniform(-lim, lim, size=(i, o))


def make_net(rng, i, h1, h2, out, extra, ln):
    """the agent's initial weights (glorot-uniform kernels, U(+-3e-3) output layer, zero biases, LayerNorm gamma 1 / beta 0)
    with EVERY parameter perturbed by 0.05 N(0, 1), float32"""
    p = dict(W1=_glorot(rng, i, h1), b1=np.zeros(h1), W2=_glorot(rng, h1 + extra, h2), b2=np.zeros(h2),
             W3=rng.uniform(-3e-3, 3e-3, size=(h2, out)), b3=np.zeros(out))
    if ln:
        p.update(ln1_b=np.zeros(h1), ln1_g=np.ones(h1), ln2_b=np.zeros(h2), ln2_g=np.ones(h2))
    return {k: (p[k] + 0.05 * rng.normal(size=p[k].shape)).astype(np.float32) for k in (LN_KEYS if ln else KEYS)}


def keys_of(p):
    return LN_KEYS if "ln1_g" in p else KEYS


_DATA = {}


def case_data(case):
    """dict(actor, critic, target_actor, target_critic (float32 dicts; the targets offset by +0.01 / -0.01), s, a, r, t, s2
    (3 B candidate rows), idx [1, B] int32 (the bounded batch: rows that pass the margin), block / mean / std (statistics or
    None), clip_norm (float or None), good_share, norms).  Deterministic in the case's name, computed once, read-only."""
    if case.name in _DATA:
        return _DATA[case.name]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    B, obs = case.B, case.obs
    actor = make_net(rng, obs, case.ah[0], case.ah[1], 1, 0, case.ln)
    critic = make_net(rng, obs, case.ch[0], case.ch[1], 1, 1, case.ln)
    f = np.float32
    target_actor = {k: (v + f(0.01)).astype(f) for k, v in actor.items()}
    target_critic = {k: (v - f(0.01)).astype(f) for k, v in critic.items()}
    n = 3 * B
    block = mean = std = None
    if case.stats:
        block, mean, std, (lo, hi) = edge_stats(obs, case.stats)
        s = rng.uniform(lo, hi, (n, obs)).astype(f)
    else:
        s = rng.uniform(-1.2, 0.6, (n, obs)).astype(f)
        if obs == 3:
            s[:, 2] = rng.uniform(-8, 8, n)              # Pendulum's theta-dot: the observation clip (-5, 5) binds
    a = rng.uniform(-1, 1, (n, 1)).astype(f)
    r = (0.5 * rng.normal(size=n)).astype(f)
    t = (rng.random(n) < 0.1).astype(np.uint8)
    s2 = (s + 0.01 * rng.normal(size=(n, obs))).astype(f)
    d = dict(actor=actor, critic=critic, target_actor=target_actor, target_critic=target_critic, s=s, a=a, r=r, t=t, s2=s2,
             block=block, mean=mean, std=std, clip_norm=None, llt=case.llt, l2=case.l2, B=B)
    margin = row_margin(d)
    good = np.nonzero(margin >= THR)[0]
    assert good.size >= B, (case.name, good.size, n)
    d["good_share"] = good.size / n
    d["idx"] = rng.permutation(good)[:B].astype(np.int32)[None]
    ref = step(d)
    d["norms"] = ref["norms"]
    if case.clip:
        norms = np.sort(np.array([v for net in ("actor", "critic") for v in ref["norms"][net].values()]))
        if case.clip == "all":
            c = 0.5 * norms[0]
        elif case.clip == "none":
            c = 2.0 * norms[-1]
        else:       # between the two neighbours furthest apart (in ratio) among the middle norms
            k = 1 + int(np.argmax(norms[2:-1] / norms[1:-2]))
            c = np.sqrt(norms[k] * norms[k + 1])
        d["clip_norm"] = float(np.float32(c))
    for v in d.values():
        for arr in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
    _DATA[case.name] = d
    return d


# ------------------------------------------------------------------------------------- the iteration, fp64 or float32 --
def _dot_seq(a, b):
    """a [M, K] @ b [K, N] in float32, one rounding per multiplication and per addition, k strictly in order"""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    return acc


class _Ar:
    """the arithmetic of one pass: fp64 with BLAS, or float32 one rounding at a time"""

    def __init__(self, f32, sizes=True):
        self.f32 = f32
        self.sizes = sizes and not f32          # carry E beside the values
        self.t = np.float32 if f32 else np.float64

    def arr(self, x):
        return np.asarray(x, self.t)

    def dot(self, a, b):
        return _dot_seq(np.ascontiguousarray(a), np.ascontiguousarray(b)) if self.f32 else a @ b

    def colsum(self, x):                      # over the batch rows
        if not self.f32:
            return x.sum(0)
        return _dot_seq(np.ones((1, x.shape[0]), np.float32), x)[0]

    def rowsum(self, x):                      # over the units of a layer
        if not self.f32:
            return x.sum(1)
        acc = np.zeros(x.shape[0], np.float32)
        for i in range(x.shape[1]):
            acc = acc + x[:, i]
        return acc

    def tanh(self, x):
        if not self.f32:
            return np.tanh(x)
        f = np.float32
        with np.errstate(over="ignore"):
            e = np.exp2(x * f(2.88539008177792681472)).astype(f)
        return f(1) - f(2) / (e + f(1))


# Every function below carries (value, E) pairs; E is None in the float32 pass (``ar.f32``), which has no use for it.
def _dense(ar, h, Eh, W, b):
    z = ar.dot(h, W) + b
    return z, (None if Eh is None else np.sqrt((Eh * Eh) @ (W * W)) + np.abs(h) @ np.abs(W) + np.abs(b))


def _back(ar, d, Ed, W):
    return ar.dot(d, W.T), (None if Ed is None else np.sqrt((Ed * Ed) @ (W * W).T) + np.abs(d) @ np.abs(W).T)


def _wgrad(ar, h, Eh, d, Ed, rows, brows):
    """(g_W, g_b, A_W, A_b) of a dense layer with input h and output delta d; rows / brows: the batch rows the weight / bias
    sums run over (all of them, in order, unless a mutant says otherwise)"""
    gW, gb = ar.dot(h[rows].T, d[rows]), ar.colsum(d[brows])
    if Ed is None:
        return gW, gb, None, None
    # the batch sums themselves: one rounding per partial sum s_k, independent of one another -- sqrt(sum_k s_k^2).  For terms
    # that cancel this is about sum |terms| (counted once, as in a dense layer); for terms of one sign, which a relu input
    # and a bias delta often are, the partial sums of an in-order accumulation grow with k and so does what they round off
    s, acc = np.zeros((h.shape[1], d.shape[1])), np.zeros((h.shape[1], d.shape[1]))
    for k in range(h.shape[0]):
        s += h[k][:, None] * d[k][None, :]
        acc += s * s
    cs = np.cumsum(d, axis=0)
    return gW, gb, Eh.T @ np.abs(d) + np.abs(h).T @ Ed + np.sqrt(acc), Ed.sum(0) + np.sqrt((cs * cs).sum(0))


def _ln_fwd(ar, z, Ez, p, which):
    """-> (n, E(n), cache); the identity without LayerNorm"""
    if which + "_g" not in p:
        return z, Ez, None
    T, n = ar.t, z.shape[1]
    mean = ar.rowsum(z) / T(n)
    d = z - mean[:, None]
    var = ar.rowsum(d * d) / T(n)
    rstd = T(1) / np.sqrt(var + T(1e-12))
    xhat = d * rstd[:, None]
    out = xhat * p[which + "_g"] + p[which + "_b"]
    if Ez is None:
        return out, None, (xhat, rstd, None, None)
    # ONE normalised operation: the projection (centre, scale) does not enlarge the error vector of z, and its own error
    # (mean, centre, variance, rstd, product) counts once, at the size of its result -- as a sum of terms counts once
    share = np.sqrt((Ez * Ez).mean(1, keepdims=True) / n)       # what the two common components (mean, xhat) pass on to a unit
    Exh = rstd[:, None] * (Ez + share * (1 + np.abs(xhat))) + np.abs(xhat)
    rho = np.sqrt(((xhat * Exh) ** 2).mean(1) / n)              # rstd's relative error: a mean of the units' independent errors
    return out, Exh * np.abs(p[which + "_g"]) + np.abs(out), (xhat, rstd, Exh, rho)


def _ln_bwd(ar, dn, Edn, cache, p, which, g, A, rows):
    """dn = dL/d(LN output) -> dL/dz; the gamma / beta gradients land in g (their sizes in A)"""
    if cache is None:
        return dn, Edn
    xhat, rstd, Exh, rho = cache
    T, n = ar.t, dn.shape[1]
    g[which + "_g"], g[which + "_b"] = ar.colsum((dn * xhat)[rows]), ar.colsum(dn[rows])
    dxh = dn * p[which + "_g"]
    m1 = ar.rowsum(dxh) / T(n)
    pr = dxh * xhat
    m2 = ar.rowsum(pr) / T(n)
    inner = dxh - m1[:, None] - xhat * m2[:, None]
    dz = rstd[:, None] * inner
    if Edn is None:
        return dz, None
    ax = np.abs(xhat)
    A[which + "_g"], A[which + "_b"] = (Edn * ax + np.abs(dn) * Exh + np.abs(dn * xhat)).sum(0), (Edn + np.abs(dn)).sum(0)
    Edxh = Edn * np.abs(p[which + "_g"]) + np.abs(dxh)
    # the same projection on the way back, once: E(dxh) scaled, what the errors of xhat and rstd do to the projection
    # itself, and one rounding at the size of the result
    share = np.sqrt((Edxh * Edxh).mean(1, keepdims=True) / n)
    Edz = (rstd[:, None] * (Edxh + share * (1 + ax)) + Exh * np.abs(m2)[:, None] + ax * np.sqrt(((dxh * Exh) ** 2).mean(1, keepdims=True) / n)
           + np.abs(dz) * (rho[:, None] + 1))
    return dz, Edz

def _tanh_fwd(ar, z, Ez):
    u = ar.tanh(z)
    return u, (None if Ez is None else (1 - u * u) * Ez + 2.0)


def _tanh_bwd(d, Ed, u, Eu):
    dd = d * (1 - u * u)
    return dd, (None if Ed is None else Ed * (1 - u * u) + np.abs(d) * (2 * np.abs(u) * Eu + 1) + np.abs(dd))


def _relu_E(n, En, band):
    """E behind a relu: E(z) under the fp64 mask; with ``band`` a unit whose |z| <= band 2^-24 E(z) keeps E(z) as well (the
    float32 value of such a unit may lie on the other side of zero: tests/forward_cases.py)"""
    if En is None:
        return None
    mask = n > 0
    if band is not None:
        mask = mask | (np.abs(n) <= band * EPS32 * En)
    return En * mask


def _hidden2(ar, n2, En2, llt, relu_band=None):
    """second hidden layer's activation: (u, E(u), relu pre-activation or None)"""
    if llt:
        return _tanh_fwd(ar, n2, En2) + (None,)
    return np.maximum(n2, ar.t(0)), _relu_E(n2, En2, relu_band), n2


def _hidden2_bwd(d, Ed, c, llt):
    if llt:
        return _tanh_bwd(d, Ed, c["a2"], c["Ea2"])
    return d * (c["n2"] > 0), (None if Ed is None else Ed * (c["n2"] > 0))


def _net_fwd(ar, p, x, Ex, llt, act=None, Eact=None, relu_band=None):
    """actor (act None: ends in tanh) or critic (the action joins the first hidden layer's output): (out, E(out), cache).
    ``relu_band``: None -- E passes a relu under the fp64 mask (the learner's batches keep their pre-activations THR from
    zero); a number -- see _relu_E"""
    z1, Ez1 = _dense(ar, x, Ex, p["W1"], p["b1"])
    n1, En1, l1 = _ln_fwd(ar, z1, Ez1, p, "ln1")
    a1, Ea1 = np.maximum(n1, ar.t(0)), _relu_E(n1, En1, relu_band)
    if act is not None:
        a1 = np.concatenate([a1, act], axis=1)
        Ea1 = None if Ea1 is None else np.concatenate([Ea1, Eact], axis=1)
    z2, Ez2 = _dense(ar, a1, Ea1, p["W2"], p["b2"])
    n2, En2, l2 = _ln_fwd(ar, z2, Ez2, p, "ln2")
    a2, Ea2, pre2 = _hidden2(ar, n2, En2, llt, relu_band)
    out, Eout = _dense(ar, a2, Ea2, p["W3"], p["b3"])
    if Eout is not None and "E_W3" in p:        # an output layer that is itself a float32 result (tests/popart_grad_cases.py)
        Eout = Eout + np.abs(a2) @ p["E_W3"] + p["E_b3"]
    c = dict(x=x, Ex=Ex, n1=n1, a1=a1, Ea1=Ea1, n2=n2, a2=a2, Ea2=Ea2, l1=l1, l2=l2, relu_pre=[n1] + ([pre2] if pre2 is not None else []))
    if act is None:
        out, Eout = _tanh_fwd(ar, out, Eout)
        c.update(out=out, Eout=Eout)
    return out, Eout, c


def _net_bwd(ar, p, c, dout, Edout, llt, want_weights, mut, rows, brows, actor):
    """O._critic_bwd / O._actor_bwd with the sizes beside the values: (g, A, dact, E(dact)); dact: the delta of the critic's
    action column (None for the actor)"""
    g, A = {}, {}
    h1 = p["W1"].shape[1]
    if actor and mut != "no_output_tanh_derivative":
        dout, Edout = _tanh_bwd(dout, Edout, c["out"], c["Eout"])
    if want_weights:
        g["W3"], g["b3"], A["W3"], A["b3"] = _wgrad(ar, c["a2"], c["Ea2"], dout, Edout, rows, brows)
    da2, Eda2 = _back(ar, dout, Edout, p["W3"])
    if Eda2 is not None and "E_W3" in p:
        Eda2 = Eda2 + np.abs(dout) @ p["E_W3"].T
    dn2, Edn2 = _hidden2_bwd(da2, Eda2, c, llt)
    if mut == "drop_last_unit_h2":
        dn2 = dn2.copy(); dn2[:, -1] = 0
    gl, Al = {}, {}
    dz2, Edz2 = _ln_bwd(ar, dn2, Edn2, c["l2"], p, "ln2", gl, Al, rows)
    if want_weights:
        g.update(gl); A.update(Al)
        g["W2"], g["b2"], A["W2"], A["b2"] = _wgrad(ar, c["a1"], c["Ea1"], dz2, Edz2, rows, brows)
    dx2, Edx2 = _back(ar, dz2, Edz2, p["W2"])
    col = slice(h1 - 1, h1) if mut == "action_row_before" else slice(h1, None)
    dact, Edact = (None, None) if actor else (dx2[:, col], None if Edx2 is None else Edx2[:, h1:])
    if want_weights:
        m1 = np.ones_like(c["n1"], bool) if mut == "no_layer1_mask" else c["n1"] > 0
        dn1, Edn1 = dx2[:, :h1] * m1, (None if Edx2 is None else Edx2[:, :h1] * (c["n1"] > 0))
        if mut == "drop_last_unit_h1":
            dn1 = dn1.copy(); dn1[:, -1] = 0
        gl, Al = {}, {}
        dz1, Edz1 = _ln_bwd(ar, dn1, Edn1, c["l1"], p, "ln1", gl, Al, rows)
        g.update(gl); A.update(Al)
        g["W1"], g["b1"], A["W1"], A["b1"] = _wgrad(ar, c["x"], c["Ex"], dz1, Edz1, rows, brows)
    return g, A, dact, Edact


def _inputs(ar, d, x, mut):
    """what the networks see of raw observations x: (x_hat, E(x_hat))"""
    T = ar.t
    x = ar.arr(x)
    E = np.zeros(x.shape) if ar.sizes else None
    if d["mean"] is not None:
        mean = np.roll(d["mean"], 1) if mut == "neighbour_mean" else d["mean"]
        x = (x - ar.arr(mean)) / ar.arr(d["std"])
        if ar.sizes:
            E = 2 * np.abs(x)       # x and mean are exact float32: the difference and the quotient round once each, at their own size
    if mut != "no_obs_clip":
        x = np.clip(x, T(-OBS_CLIP), T(OBS_CLIP))
    return x, E


def row_margin(d, rows=None):
    """smallest |relu pre-activation| of every candidate row in fp64: actor at s, critic at (s, a), critic at (s, pi(s))"""
    ar = _Ar(False)
    sel = slice(None) if rows is None else rows
    actor, critic = ({k: ar.arr(v) for k, v in d[n].items()} for n in ("actor", "critic"))
    x, Ex = _inputs(ar, d, d["s"][sel], None)
    pi, Epi, ac = _net_fwd(ar, actor, x, Ex, d["llt"])
    act = ar.arr(d["a"][sel])
    _, _, c1 = _net_fwd(ar, critic, x, Ex, d["llt"], act, np.zeros(act.shape))
    _, _, c2 = _net_fwd(ar, critic, x, Ex, d["llt"], pi, Epi)
    return np.min(np.concatenate([np.abs(p) for p in ac["relu_pre"] + c1["relu_pre"] + c2["relu_pre"]], axis=1), axis=1)


def _l2_terms(ar, critic, gc, Ac, loss_c, A_lc, l2, mut):
    """critic_l2_reg on the critic's gradients gc / sizes Ac (in place) -> (critic loss, its size)"""
    T, absd = ar.t, ar.sizes
    if l2:
        for k in ("W1", "W2", "W3") + (("b1", "b2", "b3") if mut == "l2_on_biases" else ()):
            if k[0] == "W":
                w = critic[k].reshape(-1)
                loss_c = loss_c + T(0.5) * T(l2) * ar.colsum((w * w)[:, None])[0]
            gc[k] = gc[k] + T(l2) * critic[k].reshape(gc[k].shape)
            if absd and k[0] == "W":
                Ac[k] = Ac[k] + l2 * np.abs(critic[k]) + np.abs(gc[k])
                if "E_" + k in critic:
                    Ac[k] = Ac[k] + l2 * critic["E_" + k].reshape(Ac[k].shape)
                A_lc += 0.5 * l2 * float(np.sum(critic[k] ** 2))
    return loss_c, A_lc


def _shape_and_clip(ar, actor, critic, ga, gc, Aa, Ac, clip, mut):
    """the gradients in their parameters' shapes, the per-variable norms BEFORE clip_norm, clip_norm applied:
    (ga, gc, Aa, Ac, norms, n_bound)"""
    T, absd = ar.t, ar.sizes
    ga = {k: ga[k].reshape(actor[k].shape) for k in keys_of(actor)}
    gc = {k: gc[k].reshape(critic[k].shape) for k in keys_of(critic)}
    if absd:
        Aa = {k: Aa[k].reshape(actor[k].shape) for k in keys_of(actor)}
        Ac = {k: Ac[k].reshape(critic[k].shape) for k in keys_of(critic)}
    norms = {n: {k: float(np.sqrt(np.sum(np.square(v.astype(np.float64))))) for k, v in g.items()} for n, g in (("actor", ga), ("critic", gc))}
    n_bound = 0
    if clip is not None:
        for g, A in ((ga, Aa), (gc, Ac)):
            if mut == "clip_global_norm":
                gn = T(np.sqrt(sum(float(np.sum(np.square(v.astype(np.float64)))) for v in g.values())))
            for k in g:
                v = g[k].reshape(-1)
                nrm = gn if mut == "clip_global_norm" else np.sqrt(ar.colsum((v * v)[:, None])[0])
                if nrm > T(clip):
                    sc = T(clip) / nrm
                    n_bound += 1
                    if absd:
                        A[k] = sc * A[k] + np.abs(sc * g[k]) * (float(np.sum(np.abs(g[k]) * A[k])) / float(nrm) ** 2 + 3.0)
                    g[k] = g[k] * sc
    return ga, gc, Aa, Ac, norms, n_bound


def step(d, f32=False, mut=None, idx=None, sizes=True):
    """One DDPG iteration's gradients and losses on the batch d["idx"][0]: dict g = {"actor": {key: array}, "critic": ..},
    A (the same shape; fp64 only), loss = (critic, actor), A_loss, relu_pre (list of arrays), norms = per-variable 2-norms
    BEFORE clip_norm, n_bound = variables clip_norm binds.  ``mut``: one of MUTANTS, a wrong kernel:
      drop_last_row              the last batch row left out of every gradient sum
      rows_16_31_twice           rows 16 .. 31 summed twice into every gradient
      bias_missing_tile          the bias gradients without rows 0 .. 15
      dq_1_over_B                the critic's output delta (q - y) / B
      terminal_ignored           y = r + gamma Q'(s2) on terminal rows too
      y_from_critic              y through the critic instead of the target critic
      actor_grad_at_s_a          dQ/da taken at (s, a) instead of (s, pi(s))
      action_row_before          dQ/da read from the row before the action row of W2
      no_output_tanh_derivative  the actor's output tanh taken as the identity on the way back
      no_layer1_mask             the relu mask of the first hidden layer omitted on the way back
      drop_last_unit_h1 / _h2    the delta of the last unit of the first / second hidden layer zero
      l2_on_biases               critic_l2_reg applied to the critic's biases as well
      clip_global_norm           clip_norm by the norm of the whole network's gradient
      neighbour_mean             the mean of component i - 1 in the normalisation of component i
      no_obs_clip                the observation clip not applied"""
    assert mut is None or mut in MUTANTS
    ar = _Ar(f32, sizes)
    T = ar.t
    bi = d["idx"][0] if idx is None else idx
    B = len(bi)
    llt, l2, clip = d["llt"], d["l2"], d["clip_norm"]
    actor, critic, tactor, tcritic = ({k: ar.arr(v) for k, v in d[n].items()} for n in ("actor", "critic", "target_actor", "target_critic"))
    s, Es = _inputs(ar, d, d["s"][bi], mut)
    s2, Es2 = _inputs(ar, d, d["s2"][bi], mut)
    a, r = ar.arr(d["a"][bi]), ar.arr(d["r"][bi]).reshape(B, 1)
    t = ar.arr(d["t"][bi]).reshape(B, 1)
    rows = np.arange(B)
    if mut == "drop_last_row":
        rows = rows[:-1]
    elif mut == "rows_16_31_twice":
        rows = np.concatenate([rows, rows[16:32]])
    brows = rows[rows >= 16] if mut == "bias_missing_tile" else rows
    absd = ar.sizes
    zero = np.zeros((B, 1)) if absd else None
    # y = r + (1 - terminal) gamma Q'(s2, pi'(s2))
    pi1, Epi1, _ = _net_fwd(ar, tactor, s2, Es2, llt)
    q1, Eq1, _ = _net_fwd(ar, critic if mut == "y_from_critic" else tcritic, s2, Es2, llt, pi1, Epi1)
    live = T(1) if mut == "terminal_ignored" else (T(1) - t)
    y = r + live * T(GAMMA) * q1
    Ya = (1.0 - t) * GAMMA * (Eq1 + np.abs(q1)) + np.abs(y) if absd else None
    # critic
    q, Qa, cc = _net_fwd(ar, critic, s, Es, llt, a, zero)
    e = q - y
    loss_c = ar.colsum(e * e)[0] / T(B)
    dq = e * (T(1 if mut == "dq_1_over_B" else 2) / T(B))
    Edq = 2.0 * (Qa + Ya + np.abs(e)) / B + np.abs(dq) if absd else None
    gc, Ac, _, _ = _net_bwd(ar, critic, cc, dq, Edq, llt, True, mut, rows, brows, False)
    A_lc = float(np.mean((Qa + Ya) ** 2)) if absd else None
    loss_c, A_lc = _l2_terms(ar, critic, gc, Ac, loss_c, A_lc, l2, mut)
    # actor
    pi, Epi, ac = _net_fwd(ar, actor, s, Es, llt)
    qpi, Qpia, cc2 = _net_fwd(ar, critic, s, Es, llt, pi, Epi)
    loss_a = -(ar.colsum(qpi)[0] / T(B))
    seed = np.full((B, 1), T(-1) / T(B), T)
    _, _, dact, Edact = _net_bwd(ar, critic, cc if mut == "actor_grad_at_s_a" else cc2, seed, np.abs(seed) if absd else None, llt,
                                 False, mut, rows, brows, False)
    ga, Aa, _, _ = _net_bwd(ar, actor, ac, dact, Edact, llt, True, mut, rows, brows, True)
    ga, gc, Aa, Ac, norms, n_bound = _shape_and_clip(ar, actor, critic, ga, gc, Aa, Ac, clip, mut)
    return dict(g=dict(actor=ga, critic=gc), A=dict(actor=Aa, critic=Ac) if absd else None, loss=(loss_c, loss_a),
                A_loss=(A_lc, float(np.mean(Qpia))) if absd else None, relu_pre=ac["relu_pre"] + cc["relu_pre"] + cc2["relu_pre"],
                norms=norms, n_bound=n_bound)


_REF = {}


def reference(case):
    """the fp64 iteration of the case's batch with the sizes A; computed once, never modified"""
    if case.name not in _REF:
        ref = step(case_data(case))
        for net in ("actor", "critic"):
            for x in list(ref["g"][net].values()) + list(ref["A"][net].values()):
                x.setflags(write=False)
        _REF[case.name] = ref
    return _REF[case.name]


# -------------------------------------------------------------------------------------------------------------- bounds --
def ratio(err, allowed):
    """max err / allowed over all elements; an element whose allowed error is zero (every term of it is zero) must be exact"""
    err, allowed = np.asarray(err, np.float64), np.asarray(allowed, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(allowed > 0, err / allowed, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q)) if q.size else 0.0


def grad_ratio(ref, g):
    """max |g - g64| / (2^-24 A) over every element of every parameter of both networks (units of r_case)"""
    return max(ratio(np.abs(g[n][k] - ref["g"][n][k]), EPS32 * ref["A"][n][k]) for n in ("actor", "critic") for k in ref["g"][n])


def loss_ratios(ref, loss):
    """(critic, actor): |loss - loss64| / (2^-24 A_loss)"""
    return tuple(abs(float(loss[i]) - float(ref["loss"][i])) / (EPS32 * ref["A_loss"][i]) for i in (0, 1))


def _u(g):
    """the fp64 Adam update of step 1 from zero moments, with the kernels' coefficients; monotone in g"""
    return LR1 * C1 * g / (np.sqrt(C2 * g * g) + EPSILON)


def step1_ratios(theta0, g64, A, m, v, theta1, c_grad=C_GRAD, theta0_err=0.0):
    """One parameter array after the iteration against the fp64 gradient: (m, v, theta), each the largest err / allowed over
    all elements, <= 1 accepted.  delta = C_GRAD 2^-24 A;
        |m - c1 g64| <= c1 delta + 2^-24 |c1 g64|            |v - c2 g64^2| <= c2 (2 |g64| delta + delta^2) + 3 2^-24 c2 g64^2
        theta1 in theta0 - [u(g64 + delta), u(g64 - delta)] widened by w = 8 2^-24 |u| + 2^-23 |theta0|
    (the single-workgroup kernels take the hardware rcp and sqrt; theta: 1 + the distance outside the interval in units of
    w, so that inside is <= 1 as well).  ``c_grad``: the constant in delta; ``theta0_err``: what theta0 itself may be off by
    where it is a float32 result (the Pop-Art rescaled output layer), added to w."""
    theta0, g64, A, m, v, theta1 = (np.asarray(x, np.float64) for x in (theta0, g64, A, m, v, theta1))
    delta = c_grad * EPS32 * A
    rm = ratio(np.abs(m - C1 * g64), C1 * delta + EPS32 * np.abs(C1 * g64))
    rv = ratio(np.abs(v - C2 * g64 * g64), C2 * (2 * np.abs(g64) * delta + delta * delta) + 3 * EPS32 * C2 * g64 * g64)
    u_hi, u_lo = _u(g64 + delta), _u(g64 - delta)
    w = 8 * EPS32 * np.maximum(np.abs(u_hi), np.abs(u_lo)) + 2 * EPS32 * np.abs(theta0) + theta0_err
    outside = np.maximum(np.maximum((theta0 - u_hi - w) - theta1, theta1 - (theta0 - u_lo + w)), 0.0)
    rt = ratio(np.where(outside > 0, outside + w, 0.0), w)
    return rm, rv, rt


def target_ratio(target0, theta1, target1, tau, target0_err=0.0):
    """the soft update of the NEW parameters: |target' - ((1 - tau) target + tau theta')| / (4 2^-24 (|target| + tau |theta'|));
    tau = the kernel's float32 value; ``target0_err``: what target0 itself may be off by (as theta0_err above), (1 - tau) of
    which is added to the allowed error"""
    target0, theta1, target1 = (np.asarray(x, np.float64) for x in (target0, theta1, target1))
    tau = float(np.float32(tau))
    return ratio(np.abs(target1 - ((1.0 - tau) * target0 + tau * theta1)),
                 4 * EPS32 * (np.abs(target0) + tau * np.abs(theta1)) + (1.0 - tau) * target0_err)


def adam1_32(theta, g):
    """step 1 of Adam from zero moments in float32, one rounding per operation: (m, v, theta1)"""
    f = np.float32
    theta, g = np.asarray(theta, f), np.asarray(g, f)
    m = f(BETA1) * f(0) + (f(1) - f(BETA1)) * g
    v = f(BETA2) * f(0) + (f(1) - f(BETA2)) * (g * g)
    return m, v, theta - f(LR1) * m / (np.sqrt(v) + f(EPSILON))


def flat(p):
    """a parameter dict as the learner's flat vector [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3]"""
    return np.concatenate([np.asarray(p[k]).reshape(-1) for k in keys_of(p)])


def unflat(v, like):
    out, o = {}, 0
    for k in keys_of(like):
        n = like[k].size
        out[k] = np.asarray(v[o:o + n]).reshape(like[k].shape)
        o += n
    return out
